"""Test helpers shared by tests/test_trim_scan_emu.py and tests/test_gpu_trim_scan.py: reads built so that the WINDOW scans of the end
trims decide the outcome (k_trim_ends_batched: ham_scan_lanes in fastplong_amd/csrc/kernels.h -- the bit-sliced Hamming scan of a
read's first / last 200 bases, one read per lane).  No kernel code is imported here.

A recipe is one read: random ACGT bases with one or two copies of the start adapter near the read's start (mode "start") or of the end
adapter near its end (mode "end").  Every read is checked on the CPU before a kernel sees it (Battery.verify): a plain numpy Hamming
profile of the window -- one mismatch count per tested position, raw bytes -- and the scan's own order rule (searchAdapter of the
reference, src/adaptertrimmer.cpp:84-131: at the start the LARGEST position within the threshold, else the smallest among the minima;
at the end the SMALLEST within the threshold, else the largest among the minima) must give the hit or the candidate the recipe names,
the candidate's edit distance must pass or fail as the recipe says, and where that decides the trim the oracle's record must show it.
A read whose random flanks get in the way is built again from its next seed; at most 5 % of a battery may need that (asserted)."""
import math

import numpy as np

from fastplong_amd import abi, synth
from tests.scan_cases import random_adapter

START, END = synth.START_ADAPTER, synth.END_ADAPTER
WINDOW = 200
PLEN = 16
EXT = 10
REGEN_CAP = 0.05
ODD_BYTES = ["N", "n", "lower", "U"]


def thr_of(alen):
    return int(math.floor(0.25 * alen + 0.5))


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[-1]


def tested_positions(rlen, alen, mode):
    """the r1 positions whose windows the reference's loop compares"""
    if mode == "start":
        se = min(rlen, WINDOW)
        return np.arange(0, se - alen + 1) if (alen <= rlen and se > alen) else np.zeros(0, np.int64)
    ss = max(0, rlen - WINDOW)
    return np.arange(ss, rlen - alen) if ss + alen <= rlen else np.zeros(0, np.int64)


def window_rule(r1, ad, mode):
    """-> (hit, cand, mm, positions): the scan's decision on r1 (numpy bytes), positions in r1 coordinates"""
    rlen, alen = len(r1), len(ad)
    thr = thr_of(alen)
    pos = tested_positions(rlen, alen, mode)
    if len(pos) == 0:
        return None, None, np.zeros(0, np.int64), pos
    mm = np.zeros(len(pos), np.int64)
    for i in range(alen):
        mm += r1[pos + i] != ad[i]
    hits = pos[mm <= thr]
    mins = pos[mm == mm.min()]
    if len(hits):
        # (a hit beside a better non-hit cannot exist: whatever beats a hit is within the threshold too)
        assert mm.min() <= thr and not ((mm < mm[mm <= thr].min()) & (mm > thr)).any()
        return int(hits.max() if mode == "start" else hits.min()), None, mm, pos
    return None, int(mins.min() if mode == "start" else mins.max()), mm, pos


def _subs(rng, c, k, keep=()):
    """k substitutions by another of A, C, G, T at places of c outside `keep`"""
    where = np.array([i for i in range(len(c)) if i not in keep])
    for p in rng.choice(where, k, replace=False):
        c[p] = rng.choice(synth._ACGT[synth._ACGT != c[p]])
    return c


class Copy:
    """what stands at r1 position `pos`: the adapter with `subs` substitutions (None: exactly the threshold; "over": one more);
    odd = (byte, where): one more place takes a byte outside ACGT -- "in" the copy (one more mismatch), or right "beside" it;
    indel: the copy lost a base near its end, so that its Hamming count is threshold + 1 and its edit distance within it"""

    def __init__(self, pos, subs=None, odd=None, indel=False):
        self.pos, self.subs, self.odd, self.indel = pos, subs, odd, indel

    def build(self, rng, ad):
        thr = thr_of(len(ad))
        k = thr if self.subs is None else (thr + 1 if self.subs == "over" else self.subs)
        c = ad.copy()
        if self.indel:  # drop base d, the bases behind it move up, one random base enters: h0 mismatches in the tail, the rest as subs
            for d in range(len(ad) - 3, len(ad) - 12, -1):
                t = np.concatenate([ad[:d], ad[d + 1:], synth._ACGT[rng.integers(0, 4, 1)]])
                h0 = int((t != ad).sum())
                if 3 <= h0 <= thr + 1:
                    return _subs(rng, t, thr + 1 - h0, keep=range(d, len(ad)))
            raise AssertionError("no place for the indel")
        keep = ()
        if self.odd and self.odd[1] == "in":
            p = int(rng.integers(0, len(c)))
            y = self.odd[0]
            c[p] = ord(chr(c[p]).lower() if y == "lower" else y)
            keep = (p,)
        if k + len(keep) <= thr:
            return _subs(rng, c, k, keep)
        for _ in range(200):  # beyond the threshold the copy is to FAIL the confirmation: substitutions that no indel explains cheaper
            t = _subs(rng, c.copy(), k, keep)
            if edit_distance(bytes(t), bytes(ad)) > thr:
                return t
        raise AssertionError("no set of substitutions keeps the edit distance beyond the threshold")


class Recipe:
    def __init__(self, mode, L, copies, expect, note=""):
        """expect: ("hit", i) / ("cand_ok", i) / ("cand_fail", i): copy i is the scan's hit / its candidate, whose edit distance passes /
        fails; ("none",): the scan finds no copy (nothing within the threshold, and no candidate whose edit distance passes)"""
        self.mode, self.L, self.copies, self.expect, self.note = mode, L, copies, expect, note

    def build(self, seed, adapters, front=0, tail=0):
        """copies are placed in r1 coordinates: r1 = the read without its first `front` and last `tail` bases"""
        rng = np.random.default_rng(seed)
        s = synth._ACGT[rng.integers(0, 4, self.L)].astype(np.uint8)
        ad = np.frombuffer(adapters[0 if self.mode == "start" else 1].encode(), np.uint8)
        for c in self.copies:
            b = c.build(rng, ad)
            a = front + c.pos
            assert a >= 0 and a + len(b) <= self.L - tail, (self.note, c.pos, self.L)
            s[a:a + len(b)] = b
            if c.odd and c.odd[1] == "beside":
                y = ord("a" if c.odd[0] == "lower" else c.odd[0])
                if a > 0:
                    s[a - 1] = y
                if a + len(b) < self.L:
                    s[a + len(b)] = y
        return s, rng.integers(33 + 8, 33 + 42, self.L).astype(np.uint8)


class Battery:
    def __init__(self, name, recipes, start=START, end=END, opt=None, seed=1):
        self.name, self.recipes, self.start, self.end, self.opt = name, recipes, start, end, dict(opt or {})
        self.cfgd = dict(opt=self.opt, start=start, end=end)
        self.adapters = (start, end)
        self.front, self.tail = self.opt.get("trim_front", 0), self.opt.get("trim_tail", 0)
        self.seeds = [seed * 100003 + i for i in range(len(recipes))]
        self.regenerated = 0
        self._pack()

    def _pack(self):
        self.seq, self.qual, self.off = synth.pack([r.build(s, self.adapters, self.front, self.tail)
                                                    for r, s in zip(self.recipes, self.seeds)])
        self.C = int(np.diff(self.off.astype(np.int64)).max()) + 1

    def config(self, orc):
        return orc.Config(abi.FplOptions.default(**self.opt), self.start, self.end)

    def head(self, n):
        """the first n reads as a batch of their own (ragged groups of the 64-read rounds)"""
        b = Battery.__new__(Battery)
        b.__dict__.update(self.__dict__)
        b.recipes, b.seeds = self.recipes[:n], self.seeds[:n]
        b.regenerated = 0
        b._pack()
        return b

    def _problem(self, i, res):
        r = self.recipes[i]
        o, L = int(self.off[i]), r.L
        r1 = self.seq[o + self.front:o + L - self.tail]
        rlen = len(r1)
        s, n = int(res["r1_start"][i]) - self.front, int(res["r1_len"][i])
        if res["dropped"][i]:
            return "the read is dropped"
        if r.mode == "end" and s != 0:
            return "the start trim touched a read that is about the end"
        ad = np.frombuffer(self.adapters[0 if r.mode == "start" else 1].encode(), np.uint8)
        alen, thr = len(ad), thr_of(len(ad))
        hit, cand, mm, pos = window_rule(r1, ad, r.mode)
        kind = r.expect[0]
        want = r.copies[r.expect[1]].pos if kind != "none" else None
        m = None  # position of the full match the trim goes by
        if kind == "hit":
            if hit != want:
                return "the rule's hit is %s, not %s" % (hit, want)
            m = hit
        elif kind == "none":
            if hit is not None:
                return "the rule has a hit at %d" % hit
            if cand is not None and edit_distance(bytes(r1[cand:cand + alen]), bytes(ad)) <= thr:
                return "the candidate at %d passes" % cand
        else:
            if hit is not None or cand != want:
                return "the rule's hit / candidate are %s / %s, not a candidate at %s" % (hit, cand, want)
            ed = edit_distance(bytes(r1[cand:cand + alen]), bytes(ad))
            if (ed <= thr) != (kind == "cand_ok"):
                return "the candidate's edit distance is %d (threshold %d)" % (ed, thr)
            m = cand if kind == "cand_ok" else None
        if m is None:
            return None  # (the partial-pattern search decides: the oracle's record stands as it is)
        if r.mode == "start":
            ns = min(rlen - 1, min(m + EXT, rlen - alen) + alen)
            return None if (s, n) == (ns, rlen - ns) else "the oracle leaves (%d, %d), the match at %d asks for (%d, %d)" % (s, n, m, ns, rlen - ns)
        ne = max(0, m - EXT)
        return None if (s, n) == (0, ne) else "the oracle leaves (%d, %d), the match at %d asks for (0, %d)" % (s, n, m, ne)

    def verify(self, orc):
        cfg = self.config(orc)
        for attempt in range(6):
            res, cnt = orc.process_batch(cfg, self.seq, self.qual, self.off, max_cycles=self.C)
            bad = [(i, p) for i in range(len(self.recipes)) for p in [self._problem(i, res)] if p]
            if not bad:
                assert self.regenerated <= max(1, REGEN_CAP * len(self.recipes)), (self.name, self.regenerated, len(self.recipes))
                return res, cnt
            assert attempt < 5, (self.name, [(i, self.recipes[i].note, p) for i, p in bad[:5]])
            for i, _ in bad:
                if self.seeds[i] < 1 << 40:
                    self.regenerated += 1
                self.seeds[i] += 1 << 40
            self._pack()


_verified = {}


def verified(orc, key, make):
    """a battery and the oracle's results for it, built and checked once per session"""
    if key not in _verified:
        b = make()
        _verified[key] = (b,) + b.verify(orc)
    return _verified[key]


# ---- the batteries ---------------------------------------------------------------------------------------------------------------

def _at(mode, L, alen, i):
    """r1 position of window position i (0 = the first tested one) of a read of L bases"""
    return i if mode == "start" else max(0, L - WINDOW) + i


def _last(mode, L, alen):
    """window position of the last tested window"""
    return min(L, WINDOW) - alen if mode == "start" else min(L, WINDOW) - alen - 1


def positions_battery(mode, start=START, end=END, L=460):
    """a copy with exactly the threshold's substitutions at every residue mod 32 in words 0, 3 and the last; at position 0, at the
    last tested position and one past it (not tested: at the start the copy reaches out of the window, at the end it is the window
    flush with the read's end, which the reference's loop leaves out)"""
    alen = len(start if mode == "start" else end)
    last = _last(mode, L, alen)
    words = sorted({0, 3 if 96 <= last else 0, last // 32})
    at = sorted({32 * w + r for w in words for r in range(32) if 32 * w + r <= last} | {0, last})
    rs = [Recipe(mode, L, [Copy(_at(mode, L, alen, i))], ("hit", 0), "position %d" % i) for i in at]
    rs.append(Recipe(mode, L, [Copy(_at(mode, L, alen, last + 1))], ("none",), "one past the last"))
    return Battery("positions-%s" % mode, rs, start, end)


def threshold_battery(mode, start=START, end=END, L=300):
    alen = len(start if mode == "start" else end)
    last = _last(mode, L, alen)
    rs = []
    for i in (0, 7, 31, 32, 45, 64, 100, last - 1, last):
        p = _at(mode, L, alen, i)
        rs.append(Recipe(mode, L, [Copy(p)], ("hit", 0), "threshold at %d" % i))
        rs.append(Recipe(mode, L, [Copy(p, "over")], ("cand_fail", 0), "threshold + 1 at %d" % i))
        if i + alen + 1 <= min(L, WINDOW):
            rs.append(Recipe(mode, L, [Copy(p, indel=True)], ("cand_ok", 0), "threshold + 1 with an indel at %d" % i))
    return Battery("threshold-%s" % mode, rs, start, end, seed=2)


def order_battery(mode, start=START, end=END, L=300):
    """two copies with exactly the threshold's substitutions: the start takes the right one, the end the left one; two candidates with
    equally many mismatches and no hit: the start takes the left one, the end the right one"""
    alen = len(start if mode == "start" else end)
    last = _last(mode, L, alen)
    rs = []
    for a, b in ((0, alen), (3, 40), (20, 97), (31, 64), (50, last - 1), (0, last - 1), (96, 96 + alen + 1), (60, 130)):
        pa, pb = _at(mode, L, alen, a), _at(mode, L, alen, b)
        rs.append(Recipe(mode, L, [Copy(pa), Copy(pb)], ("hit", 1 if mode == "start" else 0), "two hits %d %d" % (a, b)))
        if b + alen + 1 <= min(L, WINDOW):
            rs.append(Recipe(mode, L, [Copy(pa, indel=True), Copy(pb, indel=True)], ("cand_ok", 0 if mode == "start" else 1),
                             "two minima %d %d" % (a, b)))
    return Battery("order-%s" % mode, rs, start, end, seed=3)


def bytes_battery(mode, start=START, end=END, L=300):
    """N, n, a lower-case letter and U inside the copy (one more mismatch: threshold - 1 substitutions still hit, the threshold's do
    not) and right beside it (nothing changes); every read with such a byte stands among 64 plain ones, so that the byte-exact plane
    building and the all-ACGTN shortcut both run"""
    alen = len(start if mode == "start" else end)
    thr = thr_of(alen)
    rs = []
    for y in ODD_BYTES:
        for i in (0, 29, 70):
            p = _at(mode, L, alen, i)
            rs.append(Recipe(mode, L, [Copy(p, thr - 1, (y, "in"))], ("hit", 0), "%s in a hit at %d" % (y, i)))
            rs.append(Recipe(mode, L, [Copy(p, thr, (y, "in"))], ("cand_fail", 0), "%s in a near miss at %d" % (y, i)))
            rs.append(Recipe(mode, L, [Copy(p, None, (y, "beside"))], ("hit", 0), "%s beside a hit at %d" % (y, i)))
    plain = [Recipe(mode, L, [Copy(_at(mode, L, alen, 5 + i))], ("hit", 0), "plain") for i in range(64)]
    return Battery("bytes-%s" % mode, plain[:20] + rs[:12] + plain[20:] + rs[12:], start, end, seed=4)


def lengths_battery(mode, start=START, end=END, opt=None):
    """reads of alen, alen + 1, 199, 200, 201 and 232 bases (of r1: with trim_front / trim_tail set, trimAndCut has shortened the read
    and the window starts inside it)"""
    alen = len(start if mode == "start" else end)
    o = dict(opt or {})
    cut = o.get("trim_front", 0) + o.get("trim_tail", 0)
    rs = []
    for rl in (alen, alen + 1, 199, 200, 201, 232):
        last = _last(mode, rl, alen)
        for i in sorted({0, last // 2, last - 1, last, last + 1}):
            if i < 0 or _at(mode, rl, alen, i) + alen > rl:
                continue
            tested = _at(mode, rl, alen, i) in tested_positions(rl, alen, mode)
            rs.append(Recipe(mode, rl + cut, [Copy(_at(mode, rl, alen, i))], ("hit", 0) if tested else ("none",), "r1 of %d, position %d" % (rl, i)))
    return Battery("lengths-%s" % mode, rs, start, end, opt=o, seed=5)


ADAPTER_LENGTHS = [16, 23, 24, 25, 31, 32, 33, 40, 48, 63, 64]  # around the adder's groups of eight and sixteen and the top count plane


def adapters_battery(mode, alen, L=330):
    """both adapters of alen bases: perfect copies (the top count plane), copies at the threshold and one beyond, at the window's ends,
    across its word boundaries and (beyond 32 bases) across two of them"""
    start, end = random_adapter(100 + alen, alen), random_adapter(200 + alen, alen)
    last = _last(mode, L, alen)
    rs = []
    for i in sorted({0, 1, 17, 31, 32, 60, 95, last // 2, last - 1, last}):
        p = _at(mode, L, alen, i)
        rs.append(Recipe(mode, L, [Copy(p, 0)], ("hit", 0), "perfect at %d" % i))
        rs.append(Recipe(mode, L, [Copy(p)], ("hit", 0), "threshold at %d" % i))
        rs.append(Recipe(mode, L, [Copy(p, "over")], ("cand_fail", 0), "threshold + 1 at %d" % i))
    rs.append(Recipe(mode, L, [Copy(_at(mode, L, alen, last + 1))], ("none",), "threshold, one past the last"))
    rs.append(Recipe(mode, L, [Copy(_at(mode, L, alen, 3)), Copy(_at(mode, L, alen, 3 + alen + 2))], ("hit", 1 if mode == "start" else 0), "two hits"))
    return Battery("adapters-%s-%d" % (mode, alen), rs, start, end, seed=6)
