"""The emit kernels (fastplong_amd/csrc/emit.h: k_emit_count, k_emit_scan, k_emit_fill, k_emit_gather) on the CPU emulator, in the
order fpl_emit_batch_device launches them.  What must come out is a numpy gather over the hand-made records
(tests/emit_cases.py), never anything the kernels made; every comparison is exact, and every byte, offset and index behind the
output -- the guard items behind the exact capacities among them -- must be as it was.  tests/test_gpu_emit.py runs the same
cases through Engine.emit_device (the argument and state errors of the C call need a context and are tested there)."""
import numpy as np
import pytest

from tests import emit_cases as ec
from tests.emu_emit import build as emu


def run(seq, qual, off, res, cap_bytes, cap_reads, shift, src=True, kind=True, gather_blocks=3):
    """the backend of tests/emit_cases.py"""
    def shifted(n):  # n bytes of pattern that start `shift` bytes behind a 16-byte boundary
        raw = np.full(n + 32, ec.PAT, np.uint8)
        at = (-raw.ctypes.data) % 16 + shift
        return raw[at:at + n]
    gs, gq = shifted(cap_bytes + ec.GUARD), shifted(cap_bytes + ec.GUARD)
    goff = np.full(cap_reads + 1 + ec.GUARD, ec.PAT64, np.uint64)
    gsrc = np.full(cap_reads + ec.GUARD, ec.PAT32, np.uint32)
    gkind = np.full(cap_reads + ec.GUARD, ec.PAT, np.uint8)
    rc, info = emu.emit(seq, qual, off, np.ascontiguousarray(res), gs, gq, cap_bytes, goff, cap_reads, gsrc if src else None,
                        gkind if kind else None, gather_blocks)
    return rc, info, gs, gq, goff, gsrc, gkind


def test_lengths_at_every_source_and_destination_alignment():
    tile = emu.tile()
    seq, qual, off, res = ec.case_lengths_and_alignments(tile)
    info, want = ec.check(run, seq, qual, off, res)
    s, d = ec.alignments(off, res, want)
    assert s == set(range(16)) and d == set(range(16)), (s, d)
    assert info["max_len"] == tile + 1


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_output_arrays_at_any_address(shift):
    seq, qual, off, res = ec.case_tiles(emu.tile())
    ec.check(run, seq, qual, off, res, shift=shift)


def test_tiles_of_many_reads_and_a_read_over_many_tiles():
    tile = emu.tile()
    seq, qual, off, res = ec.case_tiles(tile)
    info, want = ec.check(run, seq, qual, off, res)
    woff = want[2]
    # the first tile holds parts of five reads with bytes, and one read lies in four tiles
    last = np.searchsorted(woff, tile - 1, "right") - 1
    assert (np.diff(woff)[:last + 1] > 0).sum() == 5
    assert ((woff[1:] - 1) // tile - woff[:-1] // tile)[np.diff(woff) > 0].max() >= 3
    # one wave alone walks all the tiles; spare capacity changes nothing
    ec.check(lambda *a: run(*a, gather_blocks=1), seq, qual, off, res, spare_bytes=1000, spare_reads=5)


def test_an_output_shorter_than_sixteen_bytes():
    seq, qual, off, res = ec.case_tiny()
    info, _ = ec.check(run, seq, qual, off, res)
    assert info["n_bytes"] == 7 and info["n_out"] == 3


def test_record_kinds():
    seq, qual, off, res = ec.case_record_kinds()
    info, want = ec.check(run, seq, qual, off, res)
    assert info["n_out"] == 2 * (1 + 2 + 1 + 1 + 2)
    assert set(want[4].tolist()) == {0, 1, 2}
    # d_src / d_kind may be left out, each alone
    for s, k in ((False, True), (True, False), (False, False)):
        rc, info2, gs, gq, goff, gsrc, gkind = run(seq, qual, off, res, info["n_bytes"], info["n_out"], 0, src=s, kind=k)
        assert rc == 0 and info2 == info
        assert np.array_equal(gs[:info["n_bytes"]], want[0]) and np.array_equal(goff[:info["n_out"] + 1].astype(np.int64), want[2])
        assert (gsrc == ec.PAT32).all() if not s else np.array_equal(gsrc[:info["n_out"]], want[3])
        assert (gkind == ec.PAT).all() if not k else np.array_equal(gkind[:info["n_out"]], want[4])


def test_every_read_fails_and_no_reads():
    seq, qual, off, res = ec.case_all_fail()
    info, _ = ec.check(run, seq, qual, off, res)
    assert info["n_out"] == 0 and info["n_bytes"] == 0
    z = np.zeros(0, np.uint8)
    rc, info, gs, gq, goff, gsrc, gkind = run(z, z, np.zeros(1, np.uint64), ec.records(0), 0, 0, 0)
    assert rc == 0 and info == dict(n_bytes=0, n_out=0, max_len=0, status=0)
    assert goff[0] == 0 and (goff[1:] == np.uint64(ec.PAT64)).all() and (gs == ec.PAT).all()


def test_more_reads_than_a_layout_block_and_more_blocks_than_a_scan_step():
    per_block, per_step = emu.layout_reads(), emu.scan_blocks()
    seq, qual, off, res = ec.case_random(3 * per_block + 17, seed=31)
    ec.check(run, seq, qual, off, res)
    n = per_block * per_step + 2 * per_block + 5  # the scan block goes round twice; the second round is not full
    seq, qual, off, res = ec.case_random(n, seed=32)
    info, _ = ec.check(run, seq, qual, off, res, shift=3)
    assert info["n_out"] > n // 2


def test_a_window_past_its_read_is_refused():
    seq, qual, off, res = ec.case_random(700, seed=33)
    want = ec.reference(seq, qual, off, res)
    n_bytes, n_out = len(want[0]), len(want[3])
    lens = np.diff(off.astype(np.int64))
    i = int(np.nonzero((res["dropped"] == 0) & (res["n_frag"] == 2) & (res["code"][:, 1] == ec.PASS))[0][-1])
    bad = res.copy()
    bad["frag_start"][i, 1] = lens[i] - bad["frag_len"][i, 1] + 1  # one byte past the read's end
    assert ec.reference(seq, qual, off, bad) is None
    ec.check_refused(run, seq, qual, off, bad, n_bytes, n_out, status=1)
    ec.check_refused(run, seq, qual, off, bad, n_bytes + 100, n_out + 100, status=1)
    # ... in a fragment that is not put out it is nobody's business
    bad["code"][i, 1] = 16
    assert ec.reference(seq, qual, off, bad) is not None
    ec.check(run, seq, qual, off, bad)
    # a start far outside, a length that wraps 32 bits
    bad = res.copy()
    bad["frag_start"][i, 1], bad["frag_len"][i, 1] = 0xFFFFFFFF, 2
    ec.check_refused(run, seq, qual, off, bad, n_bytes + 2, n_out, status=1)  # (room for the two bytes: bit 1 stays clear)
    ec.check_refused(run, seq, qual, off, bad, n_bytes - 40, n_out, status=3)


def test_capacities_one_short_are_refused_and_exact_ones_pass():
    seq, qual, off, res = ec.case_random(700, seed=34)
    want = ec.reference(seq, qual, off, res)
    n_bytes, n_out = len(want[0]), len(want[3])
    ec.check_refused(run, seq, qual, off, res, n_bytes - 1, n_out, status=2)
    ec.check_refused(run, seq, qual, off, res, n_bytes, n_out - 1, status=2)
    ec.check_refused(run, seq, qual, off, res, 0, 0, status=2)
    ec.check(run, seq, qual, off, res)
    # the capacities that always suffice
    rc, info, *_ = run(seq, qual, off, res, int(off[-1]), 2 * (len(off) - 1), 0)
    assert rc == 0 and info["status"] == 0 and info["n_bytes"] == n_bytes and info["n_out"] == n_out
