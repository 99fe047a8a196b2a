"""The window scans of k_trim_ends_batched on an MI355X against the oracle, on the reads of tests/trim_scan_cases.py: copies of the
adapters where the scan's hit or candidate decides the trim.  The same batteries as tests/test_trim_scan_emu.py; here they meet the
device forms the emulator build leaves out: v_dot4 plane building with its wait states, ds_read_addtid_b32 fetches of a lane's own
plane words, the add-with-carry of sliced_max.  Need a real MI355X: run with -m gpu."""
import pytest

from tests import trim_scan_cases as tc
from tests.test_gpu_parity import _run_both

pytestmark = pytest.mark.gpu

MODES = ["start", "end"]


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    from fastplong_amd import engine

    engine.load_library()
    return engine


def _run(orc, engine_mod, key, make, via="host", n=None):
    b, want_res, _ = tc.verified(orc, key, make)
    if n is not None:
        b, want_res, _ = tc.verified(orc, (key, n), lambda: b.head(n))
    _run_both(orc, engine_mod, b.cfgd, b.seq, b.qual, b.off, via=via)
    full = [i for i, r in enumerate(b.recipes) if r.expect[0] in ("hit", "cand_ok")]
    assert all(int(want_res["r1_len"][i]) < b.recipes[i].L - b.front - b.tail for i in full)
    return b


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_every_position_bit_exact(orc, engine_mod, mode, via):
    b = _run(orc, engine_mod, ("positions", mode), lambda: tc.positions_battery(mode), via)
    assert len(b.recipes) >= 80


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_threshold_and_order_bit_exact(orc, engine_mod, mode, via):
    _run(orc, engine_mod, ("threshold", mode), lambda: tc.threshold_battery(mode), via)
    _run(orc, engine_mod, ("order", mode), lambda: tc.order_battery(mode), via)


@pytest.mark.parametrize("via", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_odd_bytes_bit_exact(orc, engine_mod, mode, via):
    _run(orc, engine_mod, ("bytes", mode), lambda: tc.bytes_battery(mode), via)


@pytest.mark.parametrize("opt", [None, dict(trim_front=7, trim_tail=3)], ids=["whole", "cut"])
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_read_lengths_bit_exact(orc, engine_mod, mode, opt):
    _run(orc, engine_mod, ("lengths", mode, bool(opt)), lambda: tc.lengths_battery(mode, opt=opt))
    _run(orc, engine_mod, ("lengths", mode, bool(opt)), lambda: tc.lengths_battery(mode, opt=opt), "device")


@pytest.mark.parametrize("alen", tc.ADAPTER_LENGTHS)
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_adapter_lengths_bit_exact(orc, engine_mod, mode, alen):
    _run(orc, engine_mod, ("adapters", mode, alen), lambda: tc.adapters_battery(mode, alen), "host" if alen % 2 else "device")
    _run(orc, engine_mod, ("adapters", mode, alen), lambda: tc.adapters_battery(mode, alen), "device" if alen % 2 else "host")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("mode", MODES)
def test_trim_scan_ragged_groups_bit_exact(orc, engine_mod, mode, n):
    b = _run(orc, engine_mod, ("positions", mode), lambda: tc.positions_battery(mode), "device", n=n)
    assert len(b.recipes) == n
