"""The statistics passes on the emulator against the oracle, at the limits of their packed 14-bit counter fields (tests/stats_cases.py:
stacks of n copies of one read, checked on the CPU before a kernel sees them), and the host rule that sizes the slices.
tests/test_gpu_stats.py runs the same cases on an MI355X; tools/stats_mutants.py runs this file against one-line mutants of the kernels
and of the host rules (docs/kernels.md has the table)."""
import ctypes as C

import pytest

from fastplong_amd import abi
from tests import parity, stats_cases as sc
from tests.emu import emu


def _run(orc, monkeypatch, case):
    sc.apply_hooks(monkeypatch, case)
    seq, qual, off, cyc, want_res, want_cnt = sc.verified(orc, case, sc.EMU_LEN)
    got_res, got_cnt = emu.process_batch(orc.Config(abi.FplOptions.default(**case.options()), "", ""), seq, qual, off, cyc)
    parity.assert_results_equal(got_res, want_res, seq, off)
    parity.assert_counters_equal(got_cnt, want_cnt, cyc, 2)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_emulated_statistics_at_the_counter_limits(orc, monkeypatch, name):
    """every cell of a cycle at full height: results and all counters bit for bit"""
    _run(orc, monkeypatch, sc.CASES[name])


@pytest.mark.parametrize("name", sorted(sc.PER_HOOK_CASES))
def test_emulated_statistics_slice_hook_beyond_the_limit(orc, monkeypatch, name):
    """FPL_STATS_PER=20000 on 20 000 equal reads: the hook is clamped like the built-in rule, no field wraps"""
    _run(orc, monkeypatch, sc.PER_HOOK_CASES[name])


# ---- the slice rule itself (pipeline.h), on the host ---------------------------------------------------------------------------

def _rule(n, mean_len, n_cu, per_hook=0, min_bucket=0):
    """-> (per, max_slices, slabs of a batch whose longest read is mean_len)"""
    f = emu.lib().emu_stats_slice_rule
    f.restype = None
    f.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 3)()
    f(n, mean_len, n_cu, per_hook, min_bucket, out)
    return int(out[0]), int(out[1]), int(out[2])


NS = (0, 1, 63, 64, 1000, 150000, 10 ** 6, 11 * 10 ** 6)
MEANS = (1, 100, 511, 512, 2048, 9000, 200000)
CUS = (2, 16, 104, 256, 304)
FS_NB = 98          # buckets of k_bucket_plan: front trims 0 .. 96 and "not post"
FS_MIN_BUCKET = 256


def _fillings(n, min_bucket):
    """bucket fillings of a batch of n reads, the kinds that cost most slices (those k_bucket_plan gives slices of their own: at
    least min_bucket reads; the smaller ones are merged into "not post" first)"""
    yield [n]                                                    # all reads in one bucket
    if n >= FS_NB * min_bucket:                                  # every bucket just large enough: the rest in the first one
        yield [n - (FS_NB - 1) * min_bucket] + [min_bucket] * (FS_NB - 1)
    if min_bucket > 1 and n >= FS_NB * (min_bucket - 1):         # every bucket just too small: all merged, but for the first one
        rest = n - (FS_NB - 1) * (min_bucket - 1)
        merged = (FS_NB - 1) * (min_bucket - 1)
        yield [rest, merged] if rest >= min_bucket else [n]


def test_statistics_slice_rule_keeps_the_counter_limits():
    # (the two further sizes: 98 buckets of exactly FS_MIN_BUCKET reads, and of one read fewer -- _fillings)
    for n in NS + (FS_NB * FS_MIN_BUCKET, FS_NB * (FS_MIN_BUCKET - 1)):
        for mean in MEANS:
            for n_cu in CUS:
                per, max_slices, slabs = _rule(n, mean, n_cu)
                where = (n, mean, n_cu, per, max_slices)
                assert per % 64 == 0 and 64 <= per <= sc.SLICE_MAX, where
                assert max_slices % 2 == 1, where
                for counts in _fillings(n, FS_MIN_BUCKET):
                    assert sum(counts) == n
                    assert max_slices >= sum(-(-c // per) for c in counts), (where, counts[:3])
                assert slabs >= max_slices * -(-max(mean, 1) // 512), where
    # the bench's own batch -- a million reads of 9 kb on 256 CUs -- runs exactly at the limit
    assert _rule(10 ** 6, 9000, 256)[0] == sc.SLICE_MAX


@pytest.mark.parametrize("hook,want", [(1, 64), (64, 64), (65, 128), (1088, 1088), (16320, 16320), (16321, 16320), (16383, 16320),
                                       (16384, 16320), (20000, 16320), (4000000000, 16320)])
def test_statistics_slice_hook_is_rounded_and_clamped(hook, want):
    """FPL_STATS_PER: a multiple of 64 (k_bucket_plan sizes a bucket's slices by it) that a 14-bit field holds"""
    for n in (1, 1000, 10 ** 6):
        per, max_slices, _ = _rule(n, 9000, 256, per_hook=hook, min_bucket=1)
        assert per == want
        assert max_slices % 2 == 1 and max_slices >= -(-n // per)
    assert _rule(0, 0, 256, per_hook=hook)[0] == 64
