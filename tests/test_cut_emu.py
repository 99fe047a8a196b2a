"""Filter::trimAndCut and PolyX::trimPolyX on the emulator against the oracle, in both hand-written forms -- lane = read
(trim_and_cut_lanes / trim_polyx_lanes of k_trim_ends_batched, also in front of a FASTA chain) and lanes = positions
(trim_and_cut_wave / trim_polyx_wave of k_trim_ends<1> / <2> and of the batched kernel's fallback) -- on the reads of
tests/cut_cases.py: every scan stopped at the steps where the code changes path, with a promise that the builder has checked on the
CPU before a kernel sees the read.  The emulator build used here carries the FPL_EMU_TRIM_STATS counters of kernels.h, so every case
also asserts WHICH form ran: how many groups of 64 the batched kernel took and how many reads it handed to its fallback, against what
the model's step counts predict (cut_cases.falls_back: step 161 is the first to fall back).  tests/test_gpu_cut.py runs the same
batteries on an MI355X; docs/kernels.md lists the one-line mutants this file stops (tools/cut_mutants.py)."""
import pytest

from tests import cut_cases as cc
from tests import parity
from tests.emu import emu

FORMS = ["batched", "wave"]
CHAIN = ["batched-chain", "wave-chain"]


@pytest.fixture(scope="module", autouse=True)
def _counting_build():
    emu.use_trim_stats(True)
    yield
    emu.use_trim_stats(False)


def _run(orc, monkeypatch, key, make, form="batched", idx=None):
    b, want_res, want_cnt, n_fallback = cc.verified(orc, key, make)
    if idx is not None:
        b, want_res, want_cnt, n_fallback = cc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))
    if form.endswith("chain"):
        b, want_res, want_cnt, n_fallback = cc.verified(orc, (key, idx and tuple(idx), "fasta"), lambda: b.with_fasta(cc.FASTA))
    if form.startswith("batched"):
        monkeypatch.setenv("FPL_TRIM_BATCH_MIN", "1")
    else:
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
    emu.trim_stats()
    got_res, got_cnt = emu.process_batch(b.config(orc), b.seq, b.qual, b.off, b.C, n_cu=2)
    parity.assert_results_equal(got_res, want_res, b.seq, b.off)
    parity.assert_counters_equal(got_cnt, want_cnt, b.C, 2 + len(b.fasta))
    groups, handed = emu.trim_stats()
    n = len(b.recipes)
    if form.startswith("batched"):
        assert (groups, handed) == ((n + 63) // 64, n_fallback), (b.name, groups, handed, n_fallback)
    else:
        assert (groups, handed) == (0, 0), (b.name, groups, handed)
    return b, n_fallback


# ---- A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tf,tt", cc.A_TRIMS)
@pytest.mark.parametrize("w", cc.A_WINDOWS)
@pytest.mark.parametrize("side", ["front", "tail"])
def test_emulated_cut_first_good_window(orc, monkeypatch, side, w, tf, tt, form):
    """the scan stops at steps 0..17, 31..33, 63..65, 158..163 and around byte 256, on a window at the threshold and one below it"""
    b, n_fallback = _run(orc, monkeypatch, ("A", side, w, tf, tt), lambda: cc.first_window_battery(side, w, tf, tt), form)
    key = "cf" if side == "front" else "ct"
    assert {158, 159, 160, 161, 162, 163} <= {r.steps[key] for r in b.recipes}
    assert n_fallback == (len(b.recipes) if w > cc.SCAN_WMAX else sum(r.steps[key] > cc.SCAN_CAP for r in b.recipes))


@pytest.mark.parametrize("form", CHAIN)
@pytest.mark.parametrize("tf,tt", cc.A_TRIMS)
@pytest.mark.parametrize("w", cc.A_WINDOWS)
@pytest.mark.parametrize("side", ["front", "tail"])
def test_emulated_cut_first_good_window_before_a_fasta_chain(orc, monkeypatch, side, w, tf, tt, form):
    """the same reads with a two-entry FASTA list: k_trim_ends_batched<CHAIN> + k_trim_ends<2> from its records, and k_trim_ends<2> alone"""
    _run(orc, monkeypatch, ("A", side, w, tf, tt), lambda: cc.first_window_battery(side, w, tf, tt), form)


# ---- B ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tf,tt", [(0, 0), (0, 1), (3, 2)])
@pytest.mark.parametrize("w", [1, 4, 16])
@pytest.mark.parametrize("side", ["front", "tail"])
def test_emulated_cut_scan_runs_out(orc, monkeypatch, side, w, tf, tt, form):
    """no good window, or only the last one, in reads with 0..17 and 159..162 windows and on both sides of the block loads"""
    b, _ = _run(orc, monkeypatch, ("B", side, w, tf, tt), lambda: cc.run_out_battery(side, w, tf, tt), form)
    assert not b.recipes[0].alive and any(r.alive for r in b.recipes)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w", [4, 16])
def test_emulated_cut_good_stretch_between_bad_ends(orc, monkeypatch, w, form):
    b, _ = _run(orc, monkeypatch, ("B-stretch", w), lambda: cc.stretch_battery(w), form)
    assert [r.alive for r in b.recipes][:2] == [False, True]


# ---- C ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + CHAIN)
def test_emulated_cut_n_skips(orc, monkeypatch, form):
    """N runs of 0..2, 63..65 and 159..162 bases from the front cut point on and up to the tail cut point; n is no N"""
    b, n_fallback = _run(orc, monkeypatch, "C-skips", cc.n_skip_battery, form)
    assert n_fallback == sum(max(r.steps.get("cf_n", 0), r.steps.get("ct_n", 0)) > cc.SCAN_CAP for r in b.recipes) > 0


@pytest.mark.parametrize("form", FORMS + CHAIN)
def test_emulated_cut_quirks(orc, monkeypatch, form):
    """the tail's N run down to `front` and one base short of it; s = 0 and t = l - 1 stay where they are; front >= l - 1"""
    for tf in (0, 3):
        _run(orc, monkeypatch, ("C-reach", tf), lambda: cc.tail_reaches_front_battery(tf), form)
    for tf in (0, 1):
        for tt in (0, 1):
            _run(orc, monkeypatch, ("C-quirks", tf, tt), lambda: cc.quirks_battery(tf, tt), form)
    _run(orc, monkeypatch, "C-front-at-end", cc.front_at_end_battery, form)


# ---- D ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("min_len", [5, 8, 10, 12, 20])
def test_emulated_polyx_tail_lengths(orc, monkeypatch, min_len, form):
    """tails around polyx_min_len, around 16, 32, ... 128 and the cap, the whole read, r1 of 31..33 bases"""
    b, n_fallback = _run(orc, monkeypatch, ("D-len", min_len), lambda: cc.polyx_lengths_battery(min_len, "ATCG" if min_len == 10 else "AG", min_len == 10), form)
    assert n_fallback == sum(r.steps.get("px", 0) > cc.SCAN_CAP for r in b.recipes) > 0
    assert any(r.poly is None for r in b.recipes) and any(r.poly and r.win[1] == r.poly[1] for r in b.recipes)


@pytest.mark.parametrize("form", FORMS + CHAIN)
def test_emulated_polyx_mismatches_ties_and_cuts(orc, monkeypatch, form):
    """the allowance reached exactly at 8, 16 ... 56 and passed by one; N for all four; ties go to the first of A, T, C, G; the scan
    starts at the tail cut"""
    _run(orc, monkeypatch, "D-mismatch", cc.polyx_mismatch_battery, form)
    b, _ = _run(orc, monkeypatch, "D-ties", cc.polyx_tie_battery, form)
    assert sum(r.poly == (0, 0) for r in b.recipes) == 4
    _run(orc, monkeypatch, "D-behind-cut", cc.polyx_behind_cut_battery, form)


# ---- E ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", [0, 1])
def test_emulated_cut_mixed_lanes_of_one_wave(orc, monkeypatch, order, form):
    """lanes that end at step 0, 1, 15, 16, 17 and beyond the cap, dropped ones and reads too short for the block, in two orders"""
    b, n_fallback = _run(orc, monkeypatch, ("E-mix", order), lambda: cc.wave_mix_battery(order), form)
    slow = [r.steps.get("cf", 0) > cc.SCAN_CAP for r in b.recipes]
    assert len(slow) == 64 and slow[63 if order else 0] and n_fallback == sum(slow) >= 10


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_emulated_cut_ragged_groups(orc, monkeypatch, n, form):
    b, _ = _run(orc, monkeypatch, "E-ragged", cc.ragged_battery, form, idx=list(range(n)))
    assert len(b.recipes) == n


# ---- F ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
def test_emulated_start_window_behind_a_front_cut(orc, monkeypatch, form):
    """cuts of 55..58 bases with a copy at the last tested position of r1[0, 200): up to 56 the window lies in the staged head"""
    b, _ = _run(orc, monkeypatch, "F-start-cut", lambda: cc.inherit_start_battery("cut"), form)
    assert {r.win[0] for r in b.recipes} == set(cc.F_CUTS)
    for c in cc.F_CUTS:
        _run(orc, monkeypatch, ("F-start-trim", c), lambda: cc.inherit_start_battery(("trim", c)), form)


@pytest.mark.parametrize("form", FORMS)
def test_emulated_end_window_behind_a_tail_cut(orc, monkeypatch, form):
    """cut_tail, polyX and trim_tail take 55..58 bases, with a copy at the first tested position of r1's last 200 bases"""
    for how in ("cut", "polyx"):
        b, _ = _run(orc, monkeypatch, ("F-end", how), lambda: cc.inherit_end_battery(how), form)
        assert {len(s) - (r.win[1] - (r.poly[1] if r.poly else 0)) for r, (s, _) in zip(b.recipes, b.reads)} == set(cc.F_CUTS)
    for c in cc.F_CUTS:
        _run(orc, monkeypatch, ("F-end-trim", c), lambda: cc.inherit_end_battery(("trim", c)), form)
