"""The BGZF inflate kernel (fastplong_amd/csrc/bgzf_inflate.h) on the emulator, under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/emu_bgzf), against zlib's raw inflate, byte for byte.

Every payload lies at an odd offset with poisoned bytes around it and every output range has 64 guard bytes on each side (poisoned
while the kernel runs, compared afterwards), so the kernel's bounds rules are checked, not trusted.  The streams and the rules of
the comparison are tests/bgzf_cases.py, shared with the device test.

Not covered: a gzip member of the project's own device deflate recut into blocks.  That writer (csrc/gz_emit.h) gives its
distance code a single 1-bit code, an incomplete set, which this kernel refuses by its rule (see refuse/single_distance_code): such
a member is inflated by the host, so it cannot stand among the streams whose refused count must be 0."""
import os

import numpy as np
import pytest

from tests import bgzf_cases as bc
from tests.emu_bgzf import build as emu


def run(cases, seed=1, grid=0, parts=1):
    """the cases through the emulator, in `parts` sanitized processes side by side -> refused count (after bc.check)"""
    jobs, refused = [], 0
    for k in range(parts):
        part = cases[k::parts]
        if part:
            comp, blocks, out = bc.pack(part, seed + k)
            jobs.append((part, blocks, emu.start(comp, blocks, out, grid)))
    for part, blocks, job in jobs:
        out, done = emu.finish(job)
        for f in ("comp_off", "out_off", "comp_len", "isize", "crc32"):
            assert (done[f] == blocks[f]).all()
        refused += bc.check(part, blocks, out, done["status"])
    return refused


@pytest.fixture(scope="module", autouse=True)
def built():
    emu.build()


def test_writer_made_streams_are_all_taken():
    cases = bc.writer_cases()
    assert len(cases) >= 64
    assert run(cases, parts=min(8, os.cpu_count() or 1)) == 0


def test_shapes():
    assert run(bc.shape_cases(), seed=3, parts=4) == 0


def test_more_blocks_than_waves_and_outputs_out_of_order():
    """a grid of one workgroup (four waves) over 23 blocks: the work loop runs; pack() shuffles where the outputs go"""
    cases = [bc.Case("loop/%d" % i, bc.deflate(bc.payload("bam", 100 + 37 * i, i), 1)) for i in range(23)]
    assert run(cases, seed=9, grid=1) == 0


def test_hand_built_streams():
    cases = bc.hand_cases()
    assert all(c.zlib_ok for c in cases), [c.name for c in cases if not c.zlib_ok]
    assert run(cases, seed=4, parts=4) == 0


def test_must_refuse():
    cases = bc.refuse_cases()
    for c in cases:  # the yardstick agrees that these are bad, but for the one set this kernel is stricter about
        assert not c.may_pass or c.name == "refuse/single_distance_code", c.name
    assert run(cases, seed=5) == len(cases)


def test_distinct_refusal_codes():
    cases = {c.name: c for c in bc.refuse_cases()}
    pick = [cases["refuse/block_type_3"], cases["refuse/less_than_isize"], cases["refuse/crc"], cases["refuse/input_overrun_cut_in_data"]]
    comp, blocks, out = bc.pack(pick, 6)
    _, done = emu.inflate(comp, blocks, out)
    assert [int(s) for s in done["status"][:3]] == [1, 2, 3]
    assert int(done["status"][3]) != 0


def test_mutation_battery():
    """single-bit flips: the run ends clean under the sanitizers, the guards stay, and a status 0 means zlib's bytes and consent"""
    cases = bc.mutation_cases()
    assert len(cases) > 8000
    refused = run(cases, seed=7, parts=min(16, os.cpu_count() or 1))
    assert 0 < refused < len(cases)  # (some flips change nothing the decoder reads, or hit bytes of a stored block: CRC refuses those)


def test_range_checks_refuse_the_call():
    c = bc.Case("x", bc.deflate(b"abc", 6))
    comp, blocks, out = bc.pack([c], 1)
    for field, bad in (("comp_off", len(comp)), ("out_off", len(out)), ("isize", 65537), ("comp_len", len(comp))):
        b = blocks.copy()
        b[field][0] = bad
        with pytest.raises(RuntimeError, match="ended with 3"):
            emu.inflate(comp, b, out)
    assert np.dtype(bc.BLOCK_DTYPE).itemsize == 32


def test_recorded_mutation_statuses_are_the_emulator_s():
    """tests/golden/bgzf_mutation_status.json -- what the device test compares the device's statuses with -- is what this run gives"""
    import json

    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_mutation_status.json")))
    cases = {c.name: c for c in bc.mutation_cases()}
    pick = [cases[n] for n in want["names"]]
    comp, blocks, out = bc.pack(pick, 8)
    got, done = emu.inflate(comp, blocks, out)
    bc.check(pick, blocks, got, done["status"])
    assert len(pick) == 200 and len(set(want["names"])) == 200 and want["status"].count(0) >= 10
    assert [int(s) for s in done["status"]] == want["status"]
