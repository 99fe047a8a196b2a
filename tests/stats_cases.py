"""Batches for the limits of the statistics passes' packed counters (k_stats, k_stats<EXTRA>, k_stats_sorted + k_stats_reduce_sorted):
a 64-bit LDS cell holds a 22-bit quality sum and three 14-bit fields -- count, Q20, Q30 -- and three rules keep a field from carrying
into its neighbour: a slice holds <= 16 320 reads, a group of slices is handed over once its rows would pass 16 383, an EXTRA block
empties its tables once its items could pass 16 383.  A random batch puts a handful of rows into a cell; these put ALL of them there.

A STACK is n copies of one read, so that every cycle's cell of one base class gets n rows.  Nothing is random and nothing is
retried: verified() asserts on the CPU, before a kernel sees the batch, that the oracle passes every read unsplit with the promised
window and that its table reaches the promised height.

tests/test_stats_emu.py runs the cases on the emulator with reads of EMU_LEN bases (its time goes per read, not per base),
tests/test_gpu_stats.py on an MI355X with reads of GPU_LEN bases: two cycle tiles, the second one ragged."""
from dataclasses import dataclass, field

import numpy as np

from fastplong_amd import abi

EMU_LEN = 24
GPU_LEN = 520
KMER6_LEN = 1030  # two full cycle tiles and a ragged third: the second one takes the 6-mer rows
SLICE_MAX = 16320  # CS_MAX_ITEMS_PER_SLICE / 64 * 64: reads per slice
FIELD_MAX = 16383  # CS_MAX_ITEMS_PER_SLICE: rows a 14-bit field holds
FRONT = 100        # trim_front of the EXTRA cases: beyond FS_SMAX = 96, so every read is a post-only item

# by position: all three count fields set (~ ?), count and Q20 (> 5), count alone (4 !) -- a count that wraps shows in the Q20 field
# beside it, a Q20 that wraps in the Q30 field
QUALS = np.frombuffer(b"~?>54!", np.uint8)

HOOKS = ("FPL_STATS_PER", "FPL_STATS_EXTRA_PER", "FPL_STATS_EXTRA_BLOCKS", "FPL_STATS_EXTRA_ACC", "FPL_STATS_MIN_BUCKET",
         "FPL_STATS_SORT_MIN", "FPL_STATS_HI_TILE", "FPL_STATS_GROUP", "FPL_STATS_GROUP_ROWS")


def text_bytes(text, n):
    """acgt: one class per cycle; a / g: the 5-mer bins 0 and 1023 and, in reads of 1024 bases or more, the 6-mer bins 0 and 4095;
    n: an N per eight bases -- class row 6, the invalid-window path, the single 5-mer updates"""
    i = np.arange(n)
    if text == "a":
        return np.full(n, ord("A"), np.uint8)
    if text == "g":
        return np.full(n, ord("G"), np.uint8)
    s = np.frombuffer(b"ACGT", np.uint8)[i % 4].copy()
    if text == "n":
        s[i % 8 == 3] = ord("N")
    else:
        assert text == "acgt"
    return s


@dataclass
class Stack:
    n: int
    lead: int = 0  # bases of quality '!' in front of the body (cut off by --cut_front with a window of one)


@dataclass
class Case:
    name: str
    hooks: dict          # FPL_STATS_* -> value; every other hook of HOOKS is cleared
    stacks: list
    text: str = "acgt"
    opt: dict = field(default_factory=dict)
    front: int = 0       # bases in front of every read that --trim_front takes
    sorted_form: int = 0  # does the batch take k_stats_sorted?
    table: str = "pre"   # the table whose height the case is about: some cell of it holds a row of every read
    starts: tuple = ()   # r1_start per stack (default: front + lead)
    length: int = 0      # bases of the body, where the case needs a length of its own (0: EMU_LEN / GPU_LEN)

    def options(self):
        o = dict(adapter_enabled=0)
        if self.text == "n":
            o["n_base_percent_limit"] = 20  # (an eighth of the bases are N)
        if self.front:
            o["trim_front"] = self.front
        o.update(self.opt)
        return o

    def cfgd(self):
        return dict(opt=self.options(), start="", end="")

    def build(self, L):
        """-> (seq, qual, off): the stacks one after the other"""
        seqs, quals, lens = [], [], []
        for st in self.stacks:
            pre = self.front + st.lead
            seq = text_bytes(self.text, pre + L)
            qual = np.concatenate([QUALS[np.arange(self.front) % 6], np.full(st.lead, ord("!"), np.uint8), QUALS[np.arange(L) % 6]])
            seqs.append(np.tile(seq, st.n))
            quals.append(np.tile(qual, st.n))
            lens += [pre + L] * st.n
        off = np.zeros(len(lens) + 1, np.uint64)
        off[1:] = np.cumsum(np.array(lens, np.uint64))
        return np.concatenate(seqs), np.concatenate(quals), off


SORT_SLICE = dict(FPL_STATS_MIN_BUCKET=1, FPL_STATS_PER=SLICE_MAX)
SORT_GROUP = dict(FPL_STATS_MIN_BUCKET=1, FPL_STATS_PER=1088, FPL_STATS_HI_TILE=1, FPL_STATS_GROUP=16)
EXTRA = dict(FPL_STATS_EXTRA_BLOCKS=1)
EXTRA_SHORT = dict(FPL_STATS_EXTRA_BLOCKS=1, FPL_STATS_EXTRA_PER=64)
TEXTS = ("a", "g", "n")


def _cases():
    cs = []
    for n in (SLICE_MAX, SLICE_MAX + 1):  # one slice at the limit; two slices
        cs.append(Case("sorted_slice_%d" % n, SORT_SLICE, [Stack(n)], sorted_form=1))
    # 16 slices of one front trim in one group: 16 383 rows are one slab with every count field at 0x3FFF, one more row and the
    # slab goes out in two pieces; 17 408 = 16 full slices of 1088
    for n in (FIELD_MAX, FIELD_MAX + 1, 17408):
        cs.append(Case("sorted_group_%d" % n, SORT_GROUP, [Stack(n)], sorted_form=1))
    cs += [Case("sorted_group_17408_%s" % t, SORT_GROUP, [Stack(17408)], text=t, sorted_form=1) for t in TEXTS]
    # the row hook above the limit: the host's clamp of max_rows must hold
    cs.append(Case("sorted_group_rows_hook_17408", dict(SORT_GROUP, FPL_STATS_GROUP_ROWS=20000), [Stack(17408)], sorted_form=1))
    # two front trims, a full slice each
    cs.append(Case("sorted_two_trims_32640", SORT_SLICE, [Stack(SLICE_MAX), Stack(SLICE_MAX, lead=96)],
                   opt=dict(cut_front=1, cut_front_window=1), sorted_form=1, starts=(0, 96)))
    for n in (SLICE_MAX, SLICE_MAX + 1):
        cs.append(Case("unsorted_%d" % n, dict(FPL_STATS_PER=SLICE_MAX), [Stack(n)]))
    # EXTRA: one block walks all slices.  1024 items per slice: 15 slices fit, the 16th empties the tables first
    for n in (15360, 15361, 17408):
        cs.append(Case("extra_%d" % n, EXTRA, [Stack(n)], front=FRONT, table="post"))
    cs += [Case("extra_17408_%s" % t, EXTRA, [Stack(17408)], text=t, front=FRONT, table="post") for t in TEXTS]
    for n in (SLICE_MAX, FIELD_MAX + 1):  # 255 slices of 64 fit, the 256th does not
        cs.append(Case("extra_short_%d" % n, EXTRA_SHORT, [Stack(n)], front=FRONT, table="post"))
    # The 6-mer table of k_stats_sorted counts only in a cycle tile that lies inside r1 from its fourth base on, so a read reaches it
    # from 1024 bases on: all A / all G put every window pair into the 6-mer bins 0 / 4095, which kmer_flush reads twice each -- as
    # the 6-mer that starts with the 5-mer and as the one that ends with it.  (The table's counters are 32 bits wide: no height here.)
    cs += [Case("sorted_kmer6_%s" % t, SORT_GROUP, [Stack(1100)], text=t, sorted_form=1, length=KMER6_LEN) for t in TEXTS]
    return {c.name: c for c in cs}


CASES = _cases()
# FPL_STATS_PER beyond what a field holds: stats_items_per_slice clamps the hook like its own rule (emulator only)
PER_HOOK_CASES = {c.name: c for c in (
    Case("per_hook_20000_sorted", dict(FPL_STATS_MIN_BUCKET=1, FPL_STATS_PER=20000), [Stack(20000)], sorted_form=1),
    Case("per_hook_20000_unsorted", dict(FPL_STATS_PER=20000), [Stack(20000)]))}


def apply_hooks(monkeypatch, case):
    for h in HOOKS:
        if h in case.hooks:
            monkeypatch.setenv(h, str(case.hooks[h]))
        else:
            monkeypatch.delenv(h, raising=False)


_verified = {}


def verified(orc, case, L):
    """-> (seq, qual, off, C, want_res, want_cnt), built once per session, after the CPU-side assertions: every read passes unsplit
    with the window the recipe promises, and the oracle's table is as high as the case says"""
    L = case.length or L
    key = (case.name, L)
    if key not in _verified:
        seq, qual, off = case.build(L)
        C = int(np.diff(off.astype(np.int64)).max())
        cfg = orc.Config(abi.FplOptions.default(**case.options()), "", "")
        res, cnt = orc.process_batch(cfg, seq, qual, off, max_cycles=C)
        n = sum(st.n for st in case.stacks)
        assert len(res) == n
        assert (res["n_frag"] == 1).all() and not res["dropped"].any() and (res["code"][:, 0] == abi.FPL_PASS_FILTER).all(), case.name
        starts = case.starts or tuple(case.front + st.lead for st in case.stacks)
        want_start = np.repeat(np.array(starts, np.uint32), [st.n for st in case.stacks])
        assert np.array_equal(res["r1_start"], want_start) and (res["r1_len"] == L).all(), case.name
        assert np.array_equal(res["frag_start"][:, 0], want_start) and (res["frag_len"][:, 0] == L).all(), case.name
        view = abi.CountersView(cnt, C, 2)
        height = int(getattr(view, case.table).cyc[:, 0, :].max())
        assert height == n, (case.name, height)
        if case.table == "post":  # (the EXTRA cases: no read starts within FS_SMAX bases, so all of them are post-only items)
            assert min(starts) > 96
        for a in (seq, qual, off, res, cnt):
            a.setflags(write=False)
        _verified[key] = (seq, qual, off, C, res, cnt)
    return _verified[key]
