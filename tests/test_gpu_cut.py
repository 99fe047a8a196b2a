"""Filter::trimAndCut and PolyX::trimPolyX on an MI355X against the oracle, on the reads of tests/cut_cases.py: every scan stopped at
the steps where the code changes path.  The same batteries as tests/test_cut_emu.py, under the same forms -- k_trim_ends_batched
(the suite's FPL_TRIM_BATCH_MIN=1), k_trim_ends<1> (the hook cleared: what every command-line batch takes) and, for batteries A, C and
D, both with a two-entry FASTA list behind them (k_trim_ends_batched<CHAIN> + k_trim_ends<2> from its records; k_trim_ends<2> alone).
Here the reads meet the device forms the emulator compiles as plain C: load16, the masked v_sad_u8 warm-up sums, byte16<K>
extraction, the wave scan and the ballots.  Every battery goes through the host entry and the device entry.  Need a real MI355X:
run with -m gpu."""
import pytest

from tests import cut_cases as cc
from tests.test_gpu_parity import _run_both

pytestmark = pytest.mark.gpu

FORMS = ["batched", "wave"]
CHAIN = ["batched-chain", "wave-chain"]


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    from fastplong_amd import engine

    engine.load_library()
    return engine


def _run(orc, engine_mod, monkeypatch, key, make, form, idx=None):
    b = cc.verified(orc, key, make)[0]
    if idx is not None:
        b = cc.verified(orc, (key, tuple(idx)), lambda: b.pick(idx, "%d" % len(idx)))[0]
    if form.endswith("chain"):
        b = cc.verified(orc, (key, idx and tuple(idx), "fasta"), lambda: b.with_fasta(cc.FASTA))[0]
    if form.startswith("batched"):  # (the library reads the hook when a context is created)
        monkeypatch.setenv("FPL_TRIM_BATCH_MIN", "1")
    else:
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
    for via in ("host", "device"):
        _run_both(orc, engine_mod, b.cfgd, b.seq, b.qual, b.off, fasta=b.fasta, via=via)
    return b


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("w", cc.A_WINDOWS)
@pytest.mark.parametrize("side", ["front", "tail"])
def test_cut_first_good_window_bit_exact(orc, engine_mod, monkeypatch, side, w, form):
    for tf, tt in cc.A_TRIMS:
        b = _run(orc, engine_mod, monkeypatch, ("A", side, w, tf, tt), lambda: cc.first_window_battery(side, w, tf, tt), form)
        assert len(b.recipes) >= 70


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w", [1, 4, 16])
@pytest.mark.parametrize("side", ["front", "tail"])
def test_cut_scan_runs_out_bit_exact(orc, engine_mod, monkeypatch, side, w, form):
    for tf, tt in ((0, 0), (0, 1), (3, 2)):
        _run(orc, engine_mod, monkeypatch, ("B", side, w, tf, tt), lambda: cc.run_out_battery(side, w, tf, tt), form)
    if side == "front" and w > 1:
        _run(orc, engine_mod, monkeypatch, ("B-stretch", w), lambda: cc.stretch_battery(w), form)


@pytest.mark.parametrize("form", FORMS + CHAIN)
def test_cut_n_skips_and_quirks_bit_exact(orc, engine_mod, monkeypatch, form):
    _run(orc, engine_mod, monkeypatch, "C-skips", cc.n_skip_battery, form)
    for tf in (0, 3):
        _run(orc, engine_mod, monkeypatch, ("C-reach", tf), lambda: cc.tail_reaches_front_battery(tf), form)
    for tf in (0, 1):
        for tt in (0, 1):
            _run(orc, engine_mod, monkeypatch, ("C-quirks", tf, tt), lambda: cc.quirks_battery(tf, tt), form)
    _run(orc, engine_mod, monkeypatch, "C-front-at-end", cc.front_at_end_battery, form)


@pytest.mark.parametrize("form", FORMS + CHAIN)
@pytest.mark.parametrize("min_len", [5, 8, 10, 12, 20])
def test_polyx_tail_lengths_bit_exact(orc, engine_mod, monkeypatch, min_len, form):
    _run(orc, engine_mod, monkeypatch, ("D-len", min_len), lambda: cc.polyx_lengths_battery(min_len, "ATCG" if min_len == 10 else "AG", min_len == 10), form)


@pytest.mark.parametrize("form", FORMS + CHAIN)
def test_polyx_mismatches_ties_and_cuts_bit_exact(orc, engine_mod, monkeypatch, form):
    _run(orc, engine_mod, monkeypatch, "D-mismatch", cc.polyx_mismatch_battery, form)
    _run(orc, engine_mod, monkeypatch, "D-ties", cc.polyx_tie_battery, form)
    _run(orc, engine_mod, monkeypatch, "D-behind-cut", cc.polyx_behind_cut_battery, form)


@pytest.mark.parametrize("form", FORMS)
def test_cut_mixed_lanes_and_ragged_groups_bit_exact(orc, engine_mod, monkeypatch, form):
    for order in (0, 1):
        _run(orc, engine_mod, monkeypatch, ("E-mix", order), lambda: cc.wave_mix_battery(order), form)
    for n in (1, 63, 64, 65, 129):
        b = _run(orc, engine_mod, monkeypatch, "E-ragged", cc.ragged_battery, form, idx=list(range(n)))
        assert len(b.recipes) == n


@pytest.mark.parametrize("form", FORMS)
def test_adapter_windows_behind_the_cuts_bit_exact(orc, engine_mod, monkeypatch, form):
    _run(orc, engine_mod, monkeypatch, "F-start-cut", lambda: cc.inherit_start_battery("cut"), form)
    for how in ("cut", "polyx"):
        _run(orc, engine_mod, monkeypatch, ("F-end", how), lambda: cc.inherit_end_battery(how), form)
    for c in cc.F_CUTS:
        _run(orc, engine_mod, monkeypatch, ("F-start-trim", c), lambda: cc.inherit_start_battery(("trim", c)), form)
        _run(orc, engine_mod, monkeypatch, ("F-end-trim", c), lambda: cc.inherit_end_battery(("trim", c)), form)
