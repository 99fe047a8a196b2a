"""k_scan's middle-adapter scan on the emulator against the oracle, on reads where the match count decides (tests/scan_cases.py: the
builders assert on the CPU that every read does what it is for before a kernel sees it).  tests/test_gpu_scan.py runs the same
batteries on an MI355X; tools/scan_mutants.py runs this file against one-line mutants of kernels.h (docs/kernels.md has the table)."""
import numpy as np
import pytest

from fastplong_amd import abi
from tests import parity, scan_cases as sc
from tests.emu import emu


PLAIN_CUS = 16  # CUs the emulator pretends to have in the runs with the chunk hook cleared: enough waves for one read per dequeue


def _run(orc, key, make, plain=False):
    """battery -> the oracle's records, after the emulated kernels gave the same records and counters.  plain: the run with
    FPL_SCAN_CHUNK cleared must be one without pair packing -- the built-in rule deals these reads one per dequeue"""
    b, want_res, want_cnt = sc.verified(orc, key, make)
    if plain:
        assert sc.builtin_chunk(len(b.recipes), PLAIN_CUS, 2) == 1
    got_res, got_cnt = emu.process_batch(b.config(orc), b.seq, b.qual, b.off, b.C, n_cu=PLAIN_CUS if plain else 2)
    parity.assert_results_equal(got_res, want_res, b.seq, b.off)
    parity.assert_counters_equal(got_cnt, want_cnt, b.C, 2)
    return b, want_res


_assert_duels_split = sc.assert_duels_split


def _chunk(monkeypatch, chunk):
    """FPL_SCAN_CHUNK as the battery was laid out for it (0: the hook cleared -- the built-in rule deals a small batch one read per
    dequeue)"""
    if chunk:
        monkeypatch.setenv("FPL_SCAN_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)


def _assert_heads(b, n):
    """n duels of the battery promise a head, and k_scan's rules give each of them exactly that head (Battery.check_geometry)"""
    hs = b.check_geometry()
    promised = [i for i in b.duels if b.recipes[i].head is not None]
    assert len(promised) == n and all(hs[i] == b.recipes[i].head for i in promised)


@pytest.mark.parametrize("plant", [False, True])
def test_emulated_scan_duels_every_byte_pair(orc, plant):
    """every (X, Y) at k = 1, 2, 3, both orders: with all-ACGTN tiles (code_planes; Y = N alone keeps a tile on that path) and with
    lower-case bases planted beside A (build_planes)"""
    b, res = _run(orc, ("bytes", plant), lambda: sc.bytes_battery(plant=plant))
    assert len(b.duels) == 64 * 6
    _assert_duels_split(b, res)


@pytest.mark.parametrize("chunk", [4, 3, 0])
def test_emulated_scan_duels_every_place(orc, monkeypatch, chunk):
    """B at every residue of the lane chunk, across the boundary of the read's first two own tiles, as the last tested window and one
    base further, in and around a head that rides in the predecessor's last tile; chunk 0: the plain scan, no read has a next one"""
    _chunk(monkeypatch, chunk)
    b, res = _run(orc, ("places", chunk), lambda: sc.places_battery(chunk), plain=not chunk)
    _assert_duels_split(b, res)
    _assert_heads(b, 28 if chunk else 0)
    assert sum(b.recipes[i].edge is not None for i in b.duels) == 25
    assert {b.recipes[i].where for i in b.duels} - {None} == ({"inside", "ends at", "across", "at", "behind"} if chunk else set())
    kinds = [b.recipes[i].expect for i in b.duels]
    assert kinds.count("a") >= 18 and kinds.count(None) >= 9
    none = [i for i in b.duels if b.recipes[i].expect is None]
    assert (res["n_frag"][none] == 1).all()


@pytest.mark.parametrize("chunk", [4, 3, 0])
def test_emulated_scan_ties_first_copy_wins(orc, monkeypatch, chunk):
    _chunk(monkeypatch, chunk)
    b, res = _run(orc, ("ties", chunk), lambda: sc.ties_battery(chunk=chunk), plain=not chunk)
    _assert_duels_split(b, res)
    _assert_heads(b, 8 if chunk else 0)
    assert all(b.recipes[i].tie for i in b.duels)


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("la,lb", sc.EXTREME_PAIRS)
def test_emulated_scan_count_extremes(orc, monkeypatch, la, lb, chunk):
    """perfect copies of 32- and 64-base adapters (the top count plane of the six- / seven-plane form), one substitution beside none,
    lengths on both sides of the adder's groups of eight and sixteen; chunk 0: every read starts its own tiles at 0, so the copies
    laid across byte 1984 lie across a tile boundary in the pair-packing instance too"""
    _chunk(monkeypatch, chunk)
    b, res = _run(orc, ("extremes", la, lb), lambda: sc.extremes_battery(la, lb), plain=not chunk)
    _assert_duels_split(b, res)


@pytest.mark.parametrize("which", ["n", "long"])
@pytest.mark.parametrize("battery", ["bytes", "ties"])
def test_emulated_byte_scan_duels_and_ties(orc, battery, which):
    """range_scan_bytes / hamming16: an adapter that holds an N, and one of 70 bases"""
    start, end = (sc.N_ADAPTER, sc.END) if which == "n" else (sc.LONG_ADAPTER, sc.random_adapter(71, 40))
    make = (lambda: sc.bytes_battery(start, end)) if battery == "bytes" else (lambda: sc.ties_battery(start, end))
    b, res = _run(orc, (battery, which), make)
    _assert_duels_split(b, res)
    assert not any(b.check_geometry())  # (no pair packing in this instance: the ties lie where the recipes put them)
    assert any(b.recipes[i].ad == 0 for i in b.duels)  # (the adapter that forces the byte-wise scan duels too)


def test_emulated_scan_split_reads_redo(orc):
    """three copies: k_redo scans the pieces, and the N's of the middle copy decide the filter code of the piece that holds it"""
    b, res = _run(orc, "split", sc.split_battery)
    _assert_duels_split(b, res)
    for i in b.duels:  # (the copy with the Y bytes is the middle one)
        d = b.recipes[i]
        assert min(d.b_pos, d.c_pos) < d.a_pos < max(d.b_pos, d.c_pos)
    assert abi.FPL_FAIL_N_BASE in set(res["code"].ravel().tolist()) and (res["code"] == abi.FPL_PASS_FILTER).any()


@pytest.mark.parametrize("which", [0, 1])
def test_emulated_scan_sums_at_the_16_bit_fold(orc, which):
    """reads of 65535 and 65536 bases whose filter code hangs on the exact N count / complexity sum"""
    seq, qual, off = sc.fold_battery()
    cfg = orc.Config(abi.FplOptions.default(**sc.FOLD_OPTS[which]), sc.START, sc.END)
    C = 65536
    want_res, want_cnt = orc.process_batch(cfg, seq, qual, off, max_cycles=C)
    code = want_res["code"][:, 0].tolist()
    N, CX, OK = abi.FPL_FAIL_N_BASE, abi.FPL_FAIL_COMPLEXITY, abi.FPL_PASS_FILTER
    # per length: all N, ACAC.., ACAC.. with one repeat, half N, half N and one more, GNGN..
    assert code == ([CX, OK, CX, CX, CX, OK, N, OK, CX, CX, CX, OK] if which == 0 else [N, OK, OK, OK, N, OK, N, OK, OK, OK, N, OK])
    got_res, got_cnt = emu.process_batch(cfg, seq, qual, off, C)
    parity.assert_results_equal(got_res, want_res)
    parity.assert_counters_equal(got_cnt, want_cnt, C, 2)
