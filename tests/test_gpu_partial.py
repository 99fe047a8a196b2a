"""The partial-pattern searches of trimBySequenceStart / trimBySequenceEnd and the edit-distance confirmations on an MI355X against
the oracle, on the reads of tests/partial_cases.py.  The same batteries as tests/test_partial_emu.py, under the same forms --
k_trim_ends_batched (the suite's FPL_TRIM_BATCH_MIN=1; NW = 8 for the adapters of 33..64 bases), k_trim_ends<1> / <2> / <0> (the hook
cleared) and, for batteries A, B and E, both with a two-entry FASTA list behind them; battery G (the confirmations of k_resolve) through
the normal pipeline under FPL_SCAN_CHUNK = 4 and with that hook cleared.  Here the reads meet what the emulator build
replaces: v_bitop3, v_lshl_or and v_alignbit in the recurrence of partial16_candidates, brev, the scalar-unit column loop of
lev_round32 on v_readlane broadcasts, the LDS cand[][] words and the 64-bit Peq shifts.  Every battery goes through the host entry
and the device entry.  The device library has no path counters: the tests assert the battery sizes and that the promised trims
happened.  Need a real MI355X: run with -m gpu."""
import pytest

from tests import partial_cases as pc
from tests.scan_cases import random_adapter
from tests.test_gpu_parity import _run_both

pytestmark = pytest.mark.gpu

FORMS = ["batched", "wave"]
CHAIN = ["batched-chain", "wave-chain"]
MODES = ["start", "end"]


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    from fastplong_amd import engine

    engine.load_library()
    return engine


def _run(orc, engine_mod, monkeypatch, key, make, form, idx=None):
    b = pc.verified(orc, key, make)[0]
    if idx is not None:
        b = pc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))[0]
    if form.endswith("chain") and not b.fasta:
        b = pc.verified(orc, (key, idx and tuple(idx), "fasta"), lambda: b.with_fasta(pc.FASTA))[0]
    if form.startswith("batched"):  # (the library reads the hook when a context is created)
        monkeypatch.setenv("FPL_TRIM_BATCH_MIN", "1")
    else:
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
    for via in ("host", "device"):
        res, _ = _run_both(orc, engine_mod, b.cfgd, b.seq, b.qual, b.off, fasta=b.fasta, via=via)
    # the promised trims happened: the record both sides agree on is the model's r1
    for i, ms in enumerate(b.model()):
        a, e = 0, b.recipes[i].L
        for m in ms:
            if m is not None:
                a, e = a + m["left"][0], a + m["left"][1]
        assert (int(res["r1_start"][i]) - b.front, int(res["r1_len"][i])) == (a, e - a), (b.name, i, b.recipes[i].note)
    return b


def _trimmed(b):
    return sum(any(m is not None and m["count"] > 0 for m in ms) for ms in b.model())


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_partial_places_and_lengths_bit_exact(orc, engine_mod, monkeypatch, mode, form):
    for trims in ((0, 0), (7, 3)):
        opt = dict(trim_front=trims[0], trim_tail=trims[1]) if trims != (0, 0) else None
        b = _run(orc, engine_mod, monkeypatch, ("A", mode, trims), lambda: pc.places_battery(mode, opt=opt), form)
        assert len(b.recipes) == 35 and _trimmed(b) == (20 if mode == "start" else 18)
    b = _run(orc, engine_mod, monkeypatch, ("A-len", mode), lambda: pc.lengths_battery(mode), form)
    if not form.endswith("chain"):
        assert _trimmed(_run(orc, engine_mod, monkeypatch, ("A-last", mode), lambda: pc.last_window_battery(mode), form)) == 1
    assert len(b.recipes) == (36 if mode == "start" else 35)


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_partial_order_bit_exact(orc, engine_mod, monkeypatch, mode, form):
    b = _run(orc, engine_mod, monkeypatch, ("B", mode), lambda: pc.order_battery(mode), form)
    assert len(b.recipes) == (7 if mode == "start" else 10)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_partial_thresholds_bit_exact(orc, engine_mod, monkeypatch, mode, form):
    for ed_max in (0.25, 0.4):
        b = _run(orc, engine_mod, monkeypatch, ("C-pattern", mode, ed_max), lambda: pc.pattern_threshold_battery(mode, ed_max), form)
        assert len(b.recipes) == 12
    for alen, ed_max, ext in ((24, 0.25, 10), (40, 0.25, 0), (24, 0.4, 500), (40, 0.4, 500), (24, 0.25, 0)):
        ad = (pc.START if mode == "start" else pc.END) if alen == 24 else random_adapter(340, alen)
        b = _run(orc, engine_mod, monkeypatch, ("C-confirm", mode, alen, ed_max, ext), lambda: pc.confirm_battery(mode, ad, ed_max, ext), form)
        ms = [m[0 if mode == "start" else 1] for m in b.model()]
        assert any(m["ok"] for m in ms) and any(m["cmplen"] and not m["ok"] for m in ms)


@pytest.mark.parametrize("form", FORMS)
def test_partial_what_is_left_bit_exact(orc, engine_mod, monkeypatch, form):
    for alen in (24, 40, 64):
        b = _run(orc, engine_mod, monkeypatch, ("D-short", alen), lambda: pc.short_reads_battery(alen), form)
        assert len(b.recipes) == 7
    b = _run(orc, engine_mod, monkeypatch, "D-left", pc.leftover_battery, form)
    assert len(b.recipes) == 16


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("mode", MODES)
def test_partial_candidates_and_the_cap_bit_exact(orc, engine_mod, monkeypatch, mode, form):
    b = _run(orc, engine_mod, monkeypatch, ("E-cap", mode), lambda: pc.cap_battery(mode), form)
    assert len(b.recipes) == (13 if mode == "start" else 11)
    b = _run(orc, engine_mod, monkeypatch, ("E-fallback", mode), lambda: pc.fallback_battery(mode), form)
    assert _trimmed(b) == 1
    _run(orc, engine_mod, monkeypatch, ("E-beyond", mode), lambda: pc.beyond_battery(mode), form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_partial_lanes_and_ragged_groups_bit_exact(orc, engine_mod, monkeypatch, mode, form):
    for lane in (0, 31, 63):
        _run(orc, engine_mod, monkeypatch, ("E-wave", mode, lane), lambda: pc.wave_battery(mode, lane), form)
    for n in (1, 63, 64, 65, 129):
        b = _run(orc, engine_mod, monkeypatch, ("E-ragged", mode), lambda: pc.wave_battery(mode, 0, 129), form, idx=list(range(n)))
        assert len(b.recipes) == n


@pytest.mark.parametrize("form", CHAIN)
def test_partial_hinted_round_bit_exact(orc, engine_mod, monkeypatch, form):
    b = _run(orc, engine_mod, monkeypatch, "H-hint", pc.hint_battery, form)
    assert len(b.recipes) == 14 and _trimmed(b) == 12


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("alens", [pc.F_LENGTHS32, pc.F_LENGTHS64, pc.F_LENGTHS0 + ["24N"]])
@pytest.mark.parametrize("mode", MODES)
def test_confirmations_every_form_bit_exact(orc, engine_mod, monkeypatch, mode, alens, form):
    for alen in alens:
        with_n = alen == "24N"
        b = _run(orc, engine_mod, monkeypatch, ("F", mode, alen), lambda: pc.forms_battery(mode, 24 if with_n else alen, with_n), form)
        assert len(b.recipes) >= 15


def _run_middle(orc, engine_mod, monkeypatch, key, make, chunk, idx=None):
    """battery G through the normal pipeline (k_scan, k_resolve, k_redo), FPL_SCAN_CHUNK = 4 or cleared"""
    b = pc.verified(orc, key, make)[0]
    if idx is not None:
        b = pc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))[0]
    if chunk:
        monkeypatch.setenv("FPL_SCAN_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)
    for via in ("host", "device"):
        res, _ = _run_both(orc, engine_mod, b.cfgd, b.seq, b.qual, b.off, via=via)
    for i, m in enumerate(b.mids):  # the promised splits happened
        got = [(int(res["frag_start"][i, f]), int(res["frag_len"][i, f])) for f in range(int(res["n_frag"][i]))]
        assert got == m["frags"], (b.name, i, b.recipes[i].note)
    return b


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("which", [[16, 24, 31, 32], [33, 40, 63, 64], ["N", 70]])
def test_resolve_confirmations_bit_exact(orc, engine_mod, monkeypatch, which, chunk):
    for w in which:
        b = _run_middle(orc, engine_mod, monkeypatch, ("G", w), lambda: pc.resolve_battery(w), chunk)
        assert len(b.recipes) == 19 and sum(m["split"] for m in b.mids) == 9


@pytest.mark.parametrize("chunk", [4, 0])
def test_resolve_one_lane_alive_and_ragged_groups_bit_exact(orc, engine_mod, monkeypatch, chunk):
    for lane in (0, 63):
        b = _run_middle(orc, engine_mod, monkeypatch, ("G-wave", lane), lambda: pc.resolve_wave_battery(lane), chunk)
        assert [m["split"] for m in b.mids].index(True) == lane and sum(m["split"] for m in b.mids) == 1
    for n in (1, 63, 64, 65):
        b = _run_middle(orc, engine_mod, monkeypatch, ("G-wave", 0, 65), lambda: pc.resolve_wave_battery(0, 65), chunk, idx=list(range(n)))
        assert len(b.recipes) == n
