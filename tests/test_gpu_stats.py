"""The statistics passes on an MI355X against the oracle, at the limits of their packed 14-bit counter fields: the cases of
tests/stats_cases.py (stacks of n copies of one read; tests/test_stats_emu.py runs them on the emulator, and tools/stats_mutants.py
proves that they bite), here with reads of two cycle tiles, through the device entry and the shipped instructions -- ds_add_u64 on
the packed cells, the slab hand-over, the reduce kernels' unpacking.  Need a real MI355X: run with -m gpu."""
import numpy as np
import pytest

from fastplong_amd import abi
from tests import parity, stats_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    from fastplong_amd import engine

    engine.load_library()
    return engine


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_statistics_at_the_counter_limits_bit_exact(orc, engine_mod, monkeypatch, name):
    """every cell of a cycle at full height: results and all counters bit for bit, and the pass the case is about is the one the
    batch took"""
    import torch

    case = sc.CASES[name]
    sc.apply_hooks(monkeypatch, case)  # (the library reads the hooks when a context is created)
    seq, qual, off, C, want_res, want_cnt = sc.verified(orc, case, sc.GPU_LEN)
    n = len(off) - 1
    cfgd = case.cfgd()
    eng = engine_mod.Engine(abi.FplOptions.default(**cfgd["opt"]), cfgd["start"], cfgd["end"], device=0, max_cycles=C)
    st = torch.from_numpy(seq.copy()).cuda()
    qt = torch.from_numpy(qual.copy()).cuda()
    ot = torch.from_numpy(off.astype(np.int64)).cuda()
    rt = eng.process_device(st, qt, ot, C)
    torch.cuda.synchronize()
    got_res = eng.results_to_numpy(rt, n)
    got_cnt = eng.counters()
    forms = eng.batch_forms()
    eng.close()
    assert forms["batches"] == 1 and forms["reads"] == n and forms["stats_sorted"] == case.sorted_form
    parity.assert_results_equal(got_res, want_res, seq, off)
    parity.assert_counters_equal(got_cnt, want_cnt, C, 2)
