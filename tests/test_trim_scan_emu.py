"""The window scans of k_trim_ends_batched (ham_scan_lanes: bit-sliced, one read per lane) on the emulator against the oracle, on
reads where the scan's hit or candidate decides the trim (tests/trim_scan_cases.py: the builders assert on the CPU that every read does
what it is for before a kernel sees it).  tests/test_gpu_trim_scan.py runs the same batteries on an MI355X; docs/kernels.md lists the
one-line mutants of the scan that this file stops, each with the first test that fails."""
import pytest

from tests import parity, trim_scan_cases as tc
from tests.emu import emu

MODES = ["start", "end"]


def _run(orc, key, make, n=None):
    """battery (its first n reads) -> the oracle's records, after the emulated kernels gave the same records and counters"""
    b, want_res, want_cnt = tc.verified(orc, key, make)
    if n is not None:
        b, want_res, want_cnt = tc.verified(orc, (key, n), lambda: b.head(n))
    got_res, got_cnt = emu.process_batch(b.config(orc), b.seq, b.qual, b.off, b.C, n_cu=2)
    parity.assert_results_equal(got_res, want_res, b.seq, b.off)
    parity.assert_counters_equal(got_cnt, want_cnt, b.C, 2)
    return b, want_res


def _trimmed(b, res):
    """the reads whose recipe ends in a full match were trimmed (Battery.verify checked where)"""
    full = [i for i, r in enumerate(b.recipes) if r.expect[0] in ("hit", "cand_ok")]
    lens = [b.recipes[i].L - b.front - b.tail for i in full]
    assert len(full) > 0 and all(int(res["r1_len"][i]) < l for i, l in zip(full, lens))
    return full


@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_every_position(orc, mode):
    """a copy at the threshold at every residue mod 32 in words 0, 3 and the last, at position 0, the last tested one and one past it"""
    b, res = _run(orc, ("positions", mode), lambda: tc.positions_battery(mode))
    assert len(_trimmed(b, res)) >= 80 and b.recipes[-1].expect == ("none",)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_threshold(orc, mode):
    """the threshold's mismatches hit; one more leave a candidate, whose edit distance decides: one passes (an indel), one fails"""
    b, res = _run(orc, ("threshold", mode), lambda: tc.threshold_battery(mode))
    kinds = [r.expect[0] for r in b.recipes]
    assert kinds.count("hit") >= 9 and kinds.count("cand_fail") >= 9 and kinds.count("cand_ok") >= 7
    _trimmed(b, res)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_order(orc, mode):
    """two hits: the start takes the right one, the end the left one; two equal minima: the start the left one, the end the right one"""
    b, res = _run(orc, ("order", mode), lambda: tc.order_battery(mode))
    kinds = [r.expect for r in b.recipes]
    assert kinds.count(("hit", 1 if mode == "start" else 0)) == 8 and kinds.count(("cand_ok", 0 if mode == "start" else 1)) >= 5
    _trimmed(b, res)


@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_odd_bytes(orc, mode):
    """N, n, lower case and U in the copy and beside it; the reads that hold one stand among plain ones"""
    b, res = _run(orc, ("bytes", mode), lambda: tc.bytes_battery(mode))
    assert len(b.recipes) == 64 + 36
    _trimmed(b, res)


@pytest.mark.parametrize("opt", [None, dict(trim_front=7, trim_tail=3)], ids=["whole", "cut"])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_read_lengths(orc, mode, opt):
    """r1 of alen, alen + 1, 199, 200, 201 and 232 bases, whole reads and reads that trimAndCut has shortened at both ends"""
    b, res = _run(orc, ("lengths", mode, bool(opt)), lambda: tc.lengths_battery(mode, opt=opt))
    assert {r.L - b.front - b.tail for r in b.recipes} == {24, 25, 199, 200, 201, 232}
    _trimmed(b, res)


@pytest.mark.parametrize("alen", tc.ADAPTER_LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_adapter_lengths(orc, mode, alen):
    """16..32 bases (six count planes, two plane words per output word) and 33..64 (seven and three): perfect copies, the threshold"""
    b, res = _run(orc, ("adapters", mode, alen), lambda: tc.adapters_battery(mode, alen))
    _trimmed(b, res)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_trim_scan_ragged_groups(orc, mode, n):
    """batches of 1, 63, 64 and 65 reads: a last round of a wave with one lane, with all but one, full, and a second round of one"""
    b, res = _run(orc, ("positions", mode), lambda: tc.positions_battery(mode), n=n)
    assert len(b.recipes) == n
