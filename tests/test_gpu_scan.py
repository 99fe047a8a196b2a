"""k_scan's middle-adapter scan on an MI355X against the oracle, on the reads of tests/scan_cases.py: duels and ties, where the match
count decides which window wins.  The same batteries as tests/test_scan_emu.py (which tools/scan_mutants.py proves to bite); here
they meet the device forms the emulator build leaves out: v_dot4 plane building, ds_read_addtid_b32 plane fetches, the
add-with-carry of sliced_max.  Need a real MI355X: run with -m gpu."""
import numpy as np
import pytest

from fastplong_amd import abi
from tests import scan_cases as sc
from tests.test_gpu_parity import _run_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    from fastplong_amd import engine

    engine.load_library()
    return engine


def _run(orc, engine_mod, key, make, via="host", plain=False):
    """plain: the run with FPL_SCAN_CHUNK cleared must be one without pair packing"""
    b, want_res, _ = sc.verified(orc, key, make)
    if plain:
        import torch

        assert sc.builtin_chunk(len(b.recipes), torch.cuda.get_device_properties(0).multi_processor_count, 4) == 1
    _run_both(orc, engine_mod, b.cfgd, b.seq, b.qual, b.off, via=via)
    sc.assert_duels_split(b, want_res)
    return b, want_res


def _chunk(monkeypatch, chunk):
    """FPL_SCAN_CHUNK as the battery was laid out for it (0: the hook cleared)"""
    if chunk:
        monkeypatch.setenv("FPL_SCAN_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)


def _assert_heads(b, n):
    hs = b.check_geometry()
    promised = [i for i in b.duels if b.recipes[i].head is not None]
    assert len(promised) == n and all(hs[i] == b.recipes[i].head for i in promised)


@pytest.mark.parametrize("plant,via", [(False, "host"), (True, "host"), (False, "device")])
def test_scan_duels_every_byte_pair_bit_exact(orc, engine_mod, plant, via):
    b, _ = _run(orc, engine_mod, ("bytes", plant), lambda: sc.bytes_battery(plant=plant), via)
    assert len(b.duels) == 64 * 6


@pytest.mark.parametrize("chunk", [4, 3, 0])
def test_scan_duels_every_place_bit_exact(orc, engine_mod, monkeypatch, chunk):
    _chunk(monkeypatch, chunk)
    b, res = _run(orc, engine_mod, ("places", chunk), lambda: sc.places_battery(chunk), plain=not chunk)
    _assert_heads(b, 28 if chunk else 0)
    none = [i for i in b.duels if b.recipes[i].expect is None]
    assert len(none) >= 9 and (res["n_frag"][none] == 1).all()


@pytest.mark.parametrize("chunk", [4, 3, 0])
def test_scan_ties_first_copy_wins_bit_exact(orc, engine_mod, monkeypatch, chunk):
    _chunk(monkeypatch, chunk)
    b, _ = _run(orc, engine_mod, ("ties", chunk), lambda: sc.ties_battery(chunk=chunk), plain=not chunk)
    _assert_heads(b, 8 if chunk else 0)


@pytest.mark.parametrize("chunk", [4, 0])
@pytest.mark.parametrize("la,lb", sc.EXTREME_PAIRS)
def test_scan_count_extremes_bit_exact(orc, engine_mod, monkeypatch, la, lb, chunk):
    _chunk(monkeypatch, chunk)
    _run(orc, engine_mod, ("extremes", la, lb), lambda: sc.extremes_battery(la, lb), plain=not chunk)


@pytest.mark.parametrize("which", ["n", "long"])
@pytest.mark.parametrize("battery", ["bytes", "ties"])
def test_byte_scan_duels_and_ties_bit_exact(orc, engine_mod, battery, which):
    start, end = (sc.N_ADAPTER, sc.END) if which == "n" else (sc.LONG_ADAPTER, sc.random_adapter(71, 40))
    make = (lambda: sc.bytes_battery(start, end)) if battery == "bytes" else (lambda: sc.ties_battery(start, end))
    _run(orc, engine_mod, (battery, which), make)


def test_scan_split_reads_redo_bit_exact(orc, engine_mod):
    b, res = _run(orc, engine_mod, "split", sc.split_battery, via="device")
    assert abi.FPL_FAIL_N_BASE in set(res["code"].ravel().tolist()) and (res["code"] == abi.FPL_PASS_FILTER).any()


@pytest.mark.parametrize("which", [0, 1])
def test_scan_sums_at_the_16_bit_fold_bit_exact(orc, engine_mod, which):
    """(tests/test_scan_emu.py asserts the filter codes the oracle gives these reads)"""
    seq, qual, off = sc.fold_battery()
    res, _ = _run_both(orc, engine_mod, dict(opt=sc.FOLD_OPTS[which], start=sc.START, end=sc.END), seq, qual, off)
    assert len(set(res["code"][:, 0].tolist())) >= 2 and int(np.diff(off.astype(np.int64)).max()) == 65536
