"""-m gpu: BGZF blocks inflated on the device (fpl_inflate_bgzf through engine.Inflater; csrc/bgzf_inflate.h), against zlib's raw
inflate.  The streams and the rules of the comparison are tests/bgzf_cases.py, the same the emulator runs under the sanitizers
(tests/test_bgzf_inflate_emu.py); the guard bytes here check that the library brings back the blocks' ranges and nothing else.

What only a device shows: the lanes of a wave share one program counter, which the emulator's lanes do not, so the invariant of
the kernel's work loop (docs/kernels.md "k_bgzf_inflate": a convergent point between lane 0's status store and its next
atomicAdd) is covered here alone; every call goes round that loop at least once."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, build
from tests import bgzf_cases as bc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MUT_GOLDEN = os.path.join(HERE, "golden", "bgzf_mutation_status.json")


@pytest.fixture(scope="module")
def inflater():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    inf = engine.Inflater(0)
    yield inf
    inf.close()


def run(inflater, cases, seed=1):
    comp, blocks, out = bc.pack(cases, seed)
    got, status = inflater.inflate(comp, blocks, out)
    assert got is out
    return bc.check(cases, blocks, out, status), status


def test_the_battery_on_the_device(inflater):
    ok = bc.writer_cases() + bc.shape_cases() + bc.hand_cases()
    assert run(inflater, ok, 2)[0] == 0
    bad = bc.refuse_cases()
    assert run(inflater, bad, 3)[0] == len(bad)
    mixed = ok[::3] + bad  # good and bad blocks in one call
    assert run(inflater, mixed, 4)[0] == len(bad)


def test_refusal_codes(inflater):
    cases = {c.name: c for c in bc.refuse_cases()}
    pick = [cases["refuse/block_type_3"], cases["refuse/less_than_isize"], cases["refuse/crc"], cases["refuse/input_overrun_cut_in_data"]]
    _, status = run(inflater, pick, 6)
    assert [int(s) for s in status[:3]] == [abi.FPL_BGZF_MALFORMED, abi.FPL_BGZF_SIZE, abi.FPL_BGZF_CRC] and int(status[3]) != 0


def test_mutations_as_on_the_emulator(inflater):
    """200 single-bit flips whose statuses the emulator run recorded (tests/test_bgzf_inflate_emu.py keeps the record honest)"""
    want = json.load(open(MUT_GOLDEN))
    cases = {c.name: c for c in bc.mutation_cases()}
    pick = [cases[n] for n in want["names"]]
    assert len(pick) == 200 and len(set(want["names"])) == 200 and want["status"].count(0) >= 10
    _, status = run(inflater, pick, 8)  # (run() compares the bytes of every accepted flip with zlib's)
    assert [int(s) for s in status] == want["status"]


def test_a_large_call(inflater):
    """3000 blocks of 8 distinct level-1 payloads, about 190 MB out: more blocks than resident waves, the work loop runs"""
    base = [bc.Case("large/%d" % k, bc.deflate(bc.payload("bam", 65280 - 97 * k, 100 + k), 1)) for k in range(8)]
    n = 3000
    blocks = np.zeros(n, bc.BLOCK_DTYPE)
    comp = np.concatenate([np.frombuffer(c.payload, np.uint8) for c in base])
    starts = np.cumsum([0] + [len(c.payload) for c in base])
    at = 0
    for i in range(n):
        c = base[i % 8]
        blocks[i] = (starts[i % 8], at, len(c.payload), c.isize, c.crc, 7)
        at += c.isize
    out, status = inflater.inflate(comp, blocks)
    assert at > 185_000_000 and len(out) == at
    assert (status == 0).all(), np.flatnonzero(status)[:10]
    want = [np.frombuffer(c.data, np.uint8) for c in base]
    for i in range(n):
        o = int(blocks[i]["out_off"])
        assert np.array_equal(out[o:o + base[i % 8].isize], want[i % 8]), i


def test_handle_reuse(inflater):
    small = [bc.Case("reuse/a", bc.deflate(bc.payload("text", 900, 1), 6))]
    big = [bc.Case("reuse/%d" % k, bc.deflate(bc.payload("bam", 30000 + k, k), 1)) for k in range(40)]
    assert run(inflater, small)[0] == 0
    assert run(inflater, big)[0] == 0
    assert run(inflater, small)[0] == 0
    out, status = inflater.inflate(np.zeros(0, np.uint8), np.zeros(0, bc.BLOCK_DTYPE))
    assert len(out) == 0 and len(status) == 0


def test_bad_ranges_are_refused_before_anything_runs(inflater):
    from fastplong_amd import engine

    c = bc.Case("x", bc.deflate(b"abc", 6))
    comp, blocks, out = bc.pack([c], 1)
    for field, bad in (("comp_off", len(comp)), ("out_off", len(out)), ("isize", 65537), ("comp_len", len(comp))):
        b = blocks.copy()
        b[field][0] = bad
        with pytest.raises(engine.FplError, match="invalid argument"):
            inflater.inflate(comp, b, out)
    assert (out == bc.FILL).all()


@pytest.mark.parametrize("chunk", [None, "20000"])
def test_whole_run_with_device_inflate(inflater, tmp_path, chunk):
    """bin/fastplong_amd on the real library: the same outputs and reports with and without --device_inflate, nothing refused"""
    from tests.test_cli_bamgz_stub import case_bam, flags_of, reports

    build.build_all()
    bam, _ = case_bam(tmp_path, "c3_full")
    env = dict(os.environ)
    if chunk:
        env["FPLH_CHUNK_BYTES"] = chunk

    def cli(d, extra=()):
        d.mkdir(exist_ok=True)
        cmd = [build.CLI, "-i", str(bam), "-o", str(d / "out.fq"), "--failed_out", str(d / "failed.fq"), "-j", str(d / "out.json"), "-h",
               str(d / "out.html"), "-V"] + flags_of("c3_full") + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stderr

    err0 = cli(tmp_path / "host")
    err1 = cli(tmp_path / "dev", ["--device_inflate"])
    assert b"BGZF blocks inflated on the device" not in err0
    m = re.search(rb"input: BGZF blocks inflated on the device: (\d+) \((\d+) refused, inflated by the host\)", err1)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, err1.decode()[-2000:]
    for f in ("out.fq", "failed.fq"):
        assert (tmp_path / "dev" / f).read_bytes() == (tmp_path / "host" / f).read_bytes()
    assert len((tmp_path / "dev" / "out.fq").read_bytes()) > 1000
    assert reports(tmp_path / "dev") == reports(tmp_path / "host")
