"""The partial-pattern searches of trimBySequenceStart / trimBySequenceEnd and the edit-distance confirmations behind them, on the
emulator against the oracle, on the reads of tests/partial_cases.py -- in every hand-written form: lane = read (partial16_candidates +
partial16_resolve_lanes + lev_lanes32 / lev_lanes64 of k_trim_ends_batched, NW = 4 and NW = 8, its wave fallback for the reads beyond
the cap, also in front of a FASTA chain) and lanes = positions (trim_start_wave / trim_end_wave of k_trim_ends<1>, <2> and <0>, with
the hinted one-round search of <2> behind a FASTA list).  Every read carries a promise that the builder has checked on the CPU before
a kernel sees it.  The emulator build used here carries the FPL_EMU_TRIM_STATS counters of kernels.h, so every case also asserts WHICH
path ran, against what the model's column counts predict: how many reads asked for a partial search at each end, how many a lane
handed to the wave search (those with more than 10 candidate columns: 10 stays, 11 goes), how many lane-parallel searches ran and
how many rounds they took -- and that the wave-per-read kernels count nothing.  tests/test_gpu_partial.py runs the same batteries on
an MI355X; docs/kernels.md lists the one-line mutants this file stops (tools/partial_mutants.py)."""
import pytest

from tests import parity
from tests import partial_cases as pc
from tests.emu import emu
from tests.scan_cases import random_adapter

FORMS = ["batched", "wave"]
CHAIN = ["batched-chain", "wave-chain"]
MODES = ["start", "end"]


@pytest.fixture(scope="module", autouse=True)
def _counting_build():
    emu.use_trim_stats(True)
    yield
    emu.use_trim_stats(False)


def _lane_form(b):
    """does k_trim_ends_batched take this adapter set?  Adapters of 16..64 bases of A, C, G, T (DevConfig::trim_mode 1 and 2)"""
    return all(a == "" or (16 <= len(a) <= 64 and set(a) <= set("ACGT")) for a in (b.start, b.end))


def _run(orc, monkeypatch, key, make, form="batched", idx=None):
    b, want_res, want_cnt = pc.verified(orc, key, make)
    if idx is not None:
        b, want_res, want_cnt = pc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))
    if form.endswith("chain") and not b.fasta:
        b, want_res, want_cnt = pc.verified(orc, (key, idx and tuple(idx), "fasta"), lambda: b.with_fasta(pc.FASTA))
    if form.startswith("batched"):
        monkeypatch.setenv("FPL_TRIM_BATCH_MIN", "1")
    else:
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
    emu.trim_stats()
    got_res, got_cnt = emu.process_batch(b.config(orc), b.seq, b.qual, b.off, b.C, n_cu=2)
    parity.assert_results_equal(got_res, want_res, b.seq, b.off)
    parity.assert_counters_equal(got_cnt, want_cnt, b.C, 2 + len(b.fasta))
    got = dict(zip(emu.TRIM_STATS, emu.trim_stats(full=True)))
    if form.startswith("batched") and _lane_form(b):
        p = b.paths()
        want = dict(groups=(len(b.recipes) + 63) // 64, p1b=0, p2=p["cands"][0], p3_wants=p["wants"][0], p3_may=p["handed"][0],
                    p6=p["cands"][1], p7_wants=p["wants"][1], p7_may=p["handed"][1], searches=p["searches"], rounds=p["rounds"])
    else:
        want = dict.fromkeys(emu.TRIM_STATS, 0)
    assert got == want, (b.name, form, got, want)
    return b


def _models(b, mode):
    return [m[0 if mode == "start" else 1] for m in b.model()]


# ---- A ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("trims", [(0, 0), (7, 3)])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_places(orc, monkeypatch, mode, trims, form):
    """a perfect pattern copy at 0, 1, 2, 15..17, 31..33, alen - 17 .. alen - 15, 167, 168, 182, 183 (the last tested) and 184, 185,
    187 (not tested: the neighbours trim, or nothing does), alone and as the end of a truncated adapter; also behind trim_front 7 /
    trim_tail 3"""
    opt = dict(trim_front=trims[0], trim_tail=trims[1]) if trims != (0, 0) else None
    b = _run(orc, monkeypatch, ("A", mode, trims), lambda: pc.places_battery(mode, opt=opt), form)
    ms = _models(b, mode)
    assert len(b.recipes) == 35
    assert sum(m["pos"] == 183 for m in ms) == 3 and sum(m["wants"] and m["pos"] < 0 for m in ms) == 1
    # the `pos > 0` of the end search: the two tail copies at 0 are chosen and not trimmed
    assert sum(m["pos"] == 0 for m in ms) == 2 and sum(m["pos"] == 0 and m["count"] == 0 for m in ms) == (2 if mode == "end" else 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_last_window_trims(orc, monkeypatch, mode, form):
    """the window at 183 trims: the full-match search's candidate is a decoy elsewhere, the partial search's confirmation passes"""
    b = _run(orc, monkeypatch, ("A-last", mode), lambda: pc.last_window_battery(mode), form)
    m = _models(b, mode)[0]
    assert (m["pos"], m["ok"], m["count"], m["cand"], m["full"]) == (183, True, 209, True, None)


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_r1_lengths(orc, monkeypatch, mode, form):
    """r1 of 16 (lim = 0), 17, 18, 31..33, 47..49, 199..201 and 216 bases, the copy at the first and the last tested place and at lim"""
    b = _run(orc, monkeypatch, ("A-len", mode), lambda: pc.lengths_battery(mode), form)
    assert len(b.recipes) == (36 if mode == "start" else 35)
    assert {r.L for r in b.recipes} == set(pc.A_LENGTHS)


# ---- B ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_order(orc, monkeypatch, mode, form):
    """two copies in one window, and the ties of a copy with one inserted base; at the tail such a tie is how a copy at 0 trims"""
    b = _run(orc, monkeypatch, ("B", mode), lambda: pc.order_battery(mode), form)
    ms = _models(b, mode)
    assert len(b.recipes) == (7 if mode == "start" else 10)
    assert sum(m["pos"] == 1 and m["count"] > 0 for m in ms) == (0 if mode == "start" else 2)


# ---- C ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ed_max", [0.25, 0.4])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_pattern_thresholds(orc, monkeypatch, mode, ed_max, form):
    """the best window at exactly thrP and thrP + 1 edits: substitutions, and mixes with one insertion or deletion"""
    b = _run(orc, monkeypatch, ("C-pattern", mode, ed_max), lambda: pc.pattern_threshold_battery(mode, ed_max), form)
    ms = _models(b, mode)
    assert len(ms) == 12 and sum(m["pos"] >= 0 for m in ms) == 6 and {m["nearest"] - pc.thr_at(ed_max, 16) for m in ms} == {0, 1}


CONFIRMS = [(24, 0.25, 10), (40, 0.25, 0), (24, 0.4, 500), (40, 0.4, 500), (24, 0.25, 0)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alen,ed_max,ext", CONFIRMS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_confirm_thresholds(orc, monkeypatch, mode, alen, ed_max, ext, form):
    """for every cmplen from 16 to alen a truncated adapter at exactly thr[cmplen] and thr[cmplen] + 1 edits -- with the half-way
    cases round(0.25 * 18) = 5 and round(0.25 * 22) = 6 -- under ed_max 0.25 and 0.4 and ext 0, 10 and 500 (the min decides)"""
    ad = (pc.START if mode == "start" else pc.END) if alen == 24 else random_adapter(340, alen)
    b = _run(orc, monkeypatch, ("C-confirm", mode, alen, ed_max, ext), lambda: pc.confirm_battery(mode, ad, ed_max, ext), form)
    ms = _models(b, mode)
    seen = {(m["cmplen"], m["ced"] - pc.thr_at(ed_max, m["cmplen"])) for m in ms}
    lo = 16 if mode == "start" else 17
    assert {c for c, _ in seen} == set(range(lo, alen + 1)) and {d for _, d in seen} == {0, 1}
    thrP = pc.thr_at(ed_max, 16)
    for c in range(lo, alen + 1):
        # both sides of every threshold, but: the adapter's own length at the start (the full-match search has taken such a copy),
        # and where the flank of c - 16 bases is too short for thr + 1 edits with at most thrP in the pattern (the search fails first)
        assert (c, 0) in seen or (mode == "start" and c == alen), (c, seen)
        assert (c, 1) in seen or pc.thr_at(ed_max, c) + 1 - (c - 16) > thrP, (c, seen)
    assert all(m["ok"] == (m["ced"] <= pc.thr_at(ed_max, m["cmplen"])) for m in ms)


# ---- D ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alen", [24, 40, 64])
def test_emulated_partial_reads_shorter_than_the_adapter(orc, monkeypatch, alen, form):
    """r1 of 17..23 bases: pos = min(pos + ext, rlen - alen) is negative; with 40 and 64 bases pos + 16 is negative too, the read is
    erased and only a positive total is booked"""
    b = _run(orc, monkeypatch, ("D-short", alen), lambda: pc.short_reads_battery(alen), form)
    ms = _models(b, "start")
    assert len(ms) == 7 and all(m["ok"] for m in ms)
    assert sum(m["count"] <= 0 for m in ms) == (0 if alen == 24 else 7) and sum(m["left"][0] == m["left"][1] for m in ms) == (0 if alen == 24 else 7)


@pytest.mark.parametrize("form", FORMS)
def test_emulated_partial_what_is_left(orc, monkeypatch, form):
    """r1 left with 0 bases and with 1 base; both ends trimmed in one read"""
    b = _run(orc, monkeypatch, "D-left", pc.leftover_battery, form)
    left = [m[1]["left"][1] - m[1]["left"][0] for m in b.model()]
    assert len(b.recipes) == 16 and left.count(0) >= 3 and left.count(1) >= 1
    assert sum(m[0]["count"] > 0 and m[1]["count"] > 0 for m in b.model()) >= 4


# ---- E ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_candidates_and_the_cap(orc, monkeypatch, mode, form):
    """lanes that consume exactly 0, 1, 9, 10 (stay) and 11 or more columns (handed on); columns below 15 and at lim, consumed and
    never tested; an end walk that stops after 2 columns while many more remain"""
    b = _run(orc, monkeypatch, ("E-cap", mode), lambda: pc.cap_battery(mode), form)
    cols = [m["cols"] for m in _models(b, mode)]
    assert {0, 1, 9, 10, 11} <= set(cols)
    if mode == "start":
        assert len(cols) == 13 and sum(c == 10 for c in cols) == 2 and sum(c > 10 for c in cols) == 4 and max(cols) >= 18
    else:
        assert len(cols) == 11 and sum(c == 10 for c in cols) == 1 and sum(c > 10 for c in cols) == 1 and cols.count(2) >= 2
    assert sum(m["cols"] == 1 and m["pos"] < 0 for m in _models(b, mode)) == 3  # (the columns that are never tested)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_one_lane_beyond_the_cap(orc, monkeypatch, mode, lane, form):
    """a wave of plain reads around one read that is handed on, at lane 0, 31 and 63, and one that stays at the cap"""
    b = _run(orc, monkeypatch, ("E-wave", mode, lane), lambda: pc.wave_battery(mode, lane), form)
    over = [m["over"] for m in _models(b, mode)]
    assert len(over) == 64 and over[lane] and sum(over) == 1 and b.paths()["rounds"] == pc.CAP + 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_ragged_groups(orc, monkeypatch, mode, n, form):
    b = _run(orc, monkeypatch, ("E-ragged", mode), lambda: pc.wave_battery(mode, 0, 129), form, idx=list(range(n)))
    assert len(b.recipes) == n and b.paths()["handed"][0 if mode == "start" else 1] == (n + 63) // 64


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_wave_search_decides(orc, monkeypatch, mode, form):
    """reads beyond the cap on which a wrong choice of the wave search would trim: the smallest distance (not position) at the
    start; the later equal one and the strict pos > 0 at the end; columns that no window stands behind"""
    b = _run(orc, monkeypatch, ("E-fallback", mode), lambda: pc.fallback_battery(mode), form)
    ms = _models(b, mode)
    assert len(ms) == (2 if mode == "start" else 3) and all(m["over"] for m in ms)
    assert sum(m["count"] > 0 for m in ms) == 1 and sum(m["pos"] == 0 for m in ms) == (0 if mode == "start" else 1)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_emulated_partial_no_column_beyond_the_text(orc, monkeypatch, mode, form):
    """a copy that ends one base beyond r1, in a wave whose column loop runs on for a longer read"""
    b = _run(orc, monkeypatch, ("E-beyond", mode), lambda: pc.beyond_battery(mode), form)
    assert b.paths()["searches"] == 0 and b.paths()["wants"][0 if mode == "start" else 1] == 2


@pytest.mark.parametrize("form", CHAIN)
def test_emulated_partial_hinted_round(orc, monkeypatch, form):
    """a FASTA entry's truncated copy at the last position the filter's verdict leaves open, and one place to either side"""
    # (no command-line adapter: k_trim_ends_batched<CHAIN> counts its one group and nothing else, k_trim_ends<2> alone nothing)
    b = _run(orc, monkeypatch, "H-hint", pc.hint_battery, form)
    trimmed = [sum(m["count"] > 0 for m in ms if m) for ms in b.model()]
    assert len(trimmed) == 14 and trimmed == [1] * 12 + [0, 0]


# ---- F ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alen", pc.F_LENGTHS32 + pc.F_LENGTHS64 + pc.F_LENGTHS0 + ["24N"])
@pytest.mark.parametrize("mode", MODES)
def test_emulated_confirmations_every_form(orc, monkeypatch, mode, alen, form):
    """adapters of 16..32 bases (lev_lanes32 / k_trim_ends<1>), 33..64 (lev_lanes64, NW = 8 / k_trim_ends<2>) and 8, 12, 15, 70 and
    24 with an N (k_trim_ends<0>): the window scan's candidate with all thr edits in its first columns, all in its last, one more of
    each, and an indel; truncated adapters; the batch ends with a copy"""
    with_n = alen == "24N"
    n = 24 if with_n else alen
    b = _run(orc, monkeypatch, ("F", mode, alen), lambda: pc.forms_battery(mode, n, with_n), form)
    ms = _models(b, mode)
    assert len(ms) >= 15 and sum(m["cand"] for m in ms) >= 4
    if n > 16:  # (a candidate that passes and one that fails)
        assert any(m["cand"] and m["full"] is not None for m in ms) and any(m["cand"] and m["full"] is None for m in ms)


# ---- G ------------------------------------------------------------------------------------------------------------------------------

PLAIN_CUS = 16  # CUs the emulator pretends to have with FPL_SCAN_CHUNK cleared: one read per dequeue (as tests/test_scan_emu.py)


def _run_middle(orc, monkeypatch, key, make, chunk, idx=None):
    """battery G through the normal pipeline, FPL_SCAN_CHUNK = 4 or cleared; the end trims take the batched kernel and count nothing
    but their groups and the hopeless candidates of their window scans (no read asks for more than the model says)"""
    b, want_res, want_cnt = pc.verified(orc, key, make)
    if idx is not None:
        b, want_res, want_cnt = pc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))
    if chunk:
        monkeypatch.setenv("FPL_SCAN_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)
    monkeypatch.setenv("FPL_TRIM_BATCH_MIN", "1")
    emu.trim_stats()
    got_res, got_cnt = emu.process_batch(b.config(orc), b.seq, b.qual, b.off, b.C, n_cu=2 if chunk else PLAIN_CUS)
    parity.assert_results_equal(got_res, want_res, b.seq, b.off)
    parity.assert_counters_equal(got_cnt, want_cnt, b.C, 2)
    got = dict(zip(emu.TRIM_STATS, emu.trim_stats(full=True)))
    if _lane_form(b):  # (no read is handed on: the filler holds no candidate column)
        assert got["groups"] == (len(b.recipes) + 63) // 64 and got["p1b"] == got["p3_may"] == got["p7_may"] == got["searches"] == 0, got
    else:
        assert got == dict.fromkeys(emu.TRIM_STATS, 0), got
    return b


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("which", list(pc.G_PAIRS))
def test_emulated_resolve_confirmations(orc, monkeypatch, which, chunk):
    """one middle copy per read at exactly thr and thr + 1 edits, all in the first columns and all in the last, in reads of 600 and
    2100 bases (the copy across byte 1984); substitutions only; an N and a lower-case base in the window; both adapters in one read:
    lev_lanes32_acgt_w (16..32 bases), lev_lanes64_acgt (33..64), lev_lanes_any (an N in the adapter, 70 bases)"""
    b = _run_middle(orc, monkeypatch, ("G", which), lambda: pc.resolve_battery(which), chunk)
    ms = b.mids
    assert len(ms) == 19 and sum(m["split"] for m in ms) == 9
    # split at thr, not at thr + 1 -- and the N / lower-case windows two beyond
    for key, ad in (("sp", b.start), ("ep", b.end)):
        thr = pc.thr_at(0.25, len(ad))
        d = [m[key + "_ed"] - thr for m in ms if m.get(key + "_need") and m[key + "_ham"] < len(ad) // 2 + thr]
        assert d.count(0) >= 3 and d.count(1) >= 2 and d.count(2) >= 1, (key, d)
        assert all((m[key] is not None) == (m[key + "_ed"] <= thr) for m in ms)
    assert sum(m["sp"] is not None and m["ep"] is not None for m in ms) == 1


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("lane", [0, 63])
def test_emulated_resolve_one_lane_alive(orc, monkeypatch, lane, chunk):
    """63 hopeless windows and one that passes with equality, at lane 0 and at lane 63"""
    b = _run_middle(orc, monkeypatch, ("G-wave", lane), lambda: pc.resolve_wave_battery(lane), chunk)
    split = [m["split"] for m in b.mids]
    assert len(split) == 64 and split[lane] and sum(split) == 1 and all(m["sp_need"] and m["ep_need"] for m in b.mids)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_emulated_resolve_ragged_groups(orc, monkeypatch, n):
    b = _run_middle(orc, monkeypatch, ("G-wave", 0, 65), lambda: pc.resolve_wave_battery(0, 65), 4, idx=list(range(n)))
    assert len(b.recipes) == n and sum(m["split"] for m in b.mids) == (n + 63) // 64

