"""Test helpers shared by tests/test_cut_emu.py and tests/test_gpu_cut.py: reads built so that the boundary rules of the first two
phases of a batch decide the outcome -- Filter::trimAndCut (the quality cuts with their N skips) and PolyX::trimPolyX, in both
hand-written forms (lane = read: trim_and_cut_lanes / trim_polyx_lanes; lanes = positions: trim_and_cut_wave / trim_polyx_wave, in
fastplong_amd/csrc/kernels.h).  No kernel code is imported here.

A recipe is one read written as segments (base pattern, quality byte, length) and a promise worked out from the rule BY HAND where
the recipe is made: alive or dropped, the r1 window [s, e) after trimAndCut, the polyX verdict, the scan steps it is about and, in
battery F, the window after the adapter trims.  Nothing is random (battery F places its substitutions with a seeded generator, as
tests/trim_scan_cases.Copy does), nothing is rebuilt and nothing is left out: Battery.verify asserts for every read, before a
kernel sees it, that the plain model below, the oracle's direct entries and the oracle's batch record all give the promise.  A
promise that does not hold is a bug in the recipe.

The model is one loop per scan -- no blocks, no rounds, no caps -- and returns the STEP each scan ended at; from the steps it
predicts which reads k_trim_ends_batched hands to its wave-per-read fallback (falls_back)."""
from dataclasses import dataclass, field

import numpy as np

from fastplong_amd import abi, synth
from tests import trim_scan_cases as tsc

Q = 60             # cut_front_quality / cut_tail_quality of every battery: room below the threshold for the tuned byte of w = 50
T = 33 + Q         # a window passes when its bytes sum to T * w
HI, LO = T + 1, T - 1  # the two levels around the threshold
BAD = 35           # far below: one such byte fails any window of up to 50
FILL = "ACGT"
SCAN_CAP = 160     # LANE_SCAN_CAP: a lane's scan may take this many steps
SCAN_WMAX = 16     # LANE_SCAN_WMAX
POLY = "ATCG"


# ---- the model: the rule as kernels.h and SURVEY A.1 / A.2 state it ---------------------------------------------------------------

def model_trim_and_cut(seq, qual, o):
    """-> (alive, s, e, steps).  steps: cf / ct = the windows that failed before the scan ended (the step of the good window, or all
    of them), cf_n / ct_n = the N's skipped behind it"""
    seq, qual = bytes(seq), bytes(qual)  # (plain ints: no byte arithmetic)
    l, front, tail = len(seq), o.trim_front, o.trim_tail
    steps = {}
    if front == 0 and tail == 0 and not o.cut_front and not o.cut_tail:
        return True, 0, l, steps
    rlen = l - front - tail
    if rlen < 0:
        return False, 0, 0, steps
    if not o.cut_front and not o.cut_tail:
        return True, front, front + rlen, steps
    if o.cut_front:
        w, thr = o.cut_front_window, (33 + o.cut_front_quality) * o.cut_front_window
        if l - front - tail - w <= 0:
            return False, 0, 0, steps
        s = front
        while s + w < l - tail and sum(qual[s:s + w]) < thr:
            s += 1
        steps["cf"] = s - front
        if s > 0:
            s += w - 1
        n = 0
        while s < l and seq[s] == ord("N"):
            s, n = s + 1, n + 1
        steps["cf_n"] = n
        front, rlen = s, l - s - tail
    if o.cut_tail:
        w, thr = o.cut_tail_window, (33 + o.cut_tail_quality) * o.cut_tail_window
        if l - front - tail - w <= 0:
            return False, 0, 0, steps
        t = l - tail - 1
        while t - w >= front and sum(qual[t - w + 1:t + 1]) < thr:
            t -= 1
        steps["ct"] = l - tail - 1 - t
        if t < l - 1:
            t = t - w + 1
        n = 0
        while t >= 0 and seq[t] == ord("N"):
            t, n = t - 1, n + 1
        steps["ct_n"] = n
        rlen = t - front + 1
    if rlen <= 0 or front >= l - 1:
        return False, 0, 0, steps
    return True, front, front + rlen, steps


def model_polyx(r1, min_len):
    """-> (verdict, steps): verdict None or (base 0..3 in A, T, C, G order, bases cut); steps: px = the position the scan ended at
    (the length of r1 when nothing stopped it), walk = the bases the way back passed before it met the poly base"""
    r1 = bytes(r1)
    rlen = len(r1)
    n = [0, 0, 0, 0]
    P = rlen
    for pos in range(rlen):
        c = chr(r1[rlen - pos - 1])
        for b in range(4):
            n[b] += c == POLY[b] or c == "N"
        cmp_ = pos + 1
        allowed = min(5, cmp_ // 8)
        if all(cmp_ - n[b] > allowed for b in range(4)) and (pos >= 8 or pos + 1 >= min_len - 1):
            P = pos
            break
    steps = {"px": P}
    if P + 1 < min_len:
        return None, steps
    poly = n.index(max(n))  # the first maximum
    i0 = max(0, rlen - P - 1)
    i = i0
    while i < rlen and r1[i] != ord(POLY[poly]):
        i += 1
    steps["walk"] = i - i0
    return (poly, rlen - i if i < rlen else 0), steps


def falls_back(steps, o):
    """does k_trim_ends_batched hand this read to the wave-per-read forms?  Every read when a cut window is wider than
    LANE_SCAN_WMAX; else the reads one of whose scans made more than LANE_SCAN_CAP steps: `if (++it > LANE_SCAN_CAP) slow = true`
    stands behind the step, so a scan that ends AT step 160 (160 failed windows, skipped N's or passed bases before it) stays in
    its lane and step 161 is the first to fall back"""
    if (o.cut_front and o.cut_front_window > SCAN_WMAX) or (o.cut_tail and o.cut_tail_window > SCAN_WMAX):
        return True
    return any(v > SCAN_CAP for v in steps.values())


# ---- recipes ------------------------------------------------------------------------------------------------------------------------

def seg(n, q=HI, pat=FILL):
    return (pat, q, n)


@dataclass
class Recipe:
    segs: list
    alive: bool
    win: tuple = None          # [s, e) after trimAndCut
    poly: tuple = None         # (base, bases cut) when polyX is called
    steps: dict = field(default_factory=dict)  # the steps the recipe is about
    tune: tuple = ()           # (position, quality byte)
    copy: tuple = None         # battery F: (mode, trim_scan_cases.Copy): an adapter copy in r1 coordinates (after polyX)
    after: tuple = None        # battery F: r1 after the adapter trims
    note: str = ""

    def build(self, adapters=None, seed=0):
        s = "".join((pat * (n // len(pat) + 1))[:n] for pat, _, n in self.segs)
        q = b"".join(bytes([qb]) * n for _, qb, n in self.segs)
        s, q = np.frombuffer(s.encode(), np.uint8).copy(), np.frombuffer(q, np.uint8).copy()
        for p, v in self.tune:
            assert 33 <= v <= 126
            q[p] = v
        if self.copy:
            mode, c = self.copy
            ad = np.frombuffer(adapters[0 if mode == "start" else 1].encode(), np.uint8)
            b = c.build(np.random.default_rng(seed), ad)
            a = self.win[0] + c.pos
            assert a + len(b) <= self.win[1] - (self.poly[1] if self.poly else 0)
            s[a:a + len(b)] = b
        return s, q


class Battery:
    def __init__(self, name, opt, recipes, start="", end="", fasta=()):
        o = dict(cut_front_quality=Q, cut_tail_quality=Q)
        o.update(opt)
        if not start and not end and not fasta:
            o.setdefault("adapter_enabled", 0)
        self.name, self.opt, self.recipes, self.start, self.end, self.fasta = name, o, list(recipes), start, end, tuple(fasta)
        self.cfgd = dict(opt=o, start=start, end=end)
        assert 0 < len(self.recipes) <= 400
        self._pack()

    def _pack(self):
        self.reads = [r.build((self.start, self.end), 7919 + i) for i, r in enumerate(self.recipes)]
        assert max(len(s) for s, _ in self.reads) <= 720
        self.seq, self.qual, self.off = synth.pack(self.reads)
        self.C = int(np.diff(self.off.astype(np.int64)).max()) + 1

    def options(self):
        return abi.FplOptions.default(**self.opt)

    def config(self, orc):
        return orc.Config(self.options(), self.start, self.end, self.fasta)

    def pick(self, idx, name):
        """the reads idx, in that order, as a battery of their own"""
        return Battery("%s-%s" % (self.name, name), self.opt, [self.recipes[i] for i in idx], self.start, self.end, self.fasta)

    def with_fasta(self, fasta):
        """the same reads in front of a FASTA chain (adapters on: the chain's entries occur in no read)"""
        o = dict(self.opt, adapter_enabled=1)
        return Battery(self.name + "-fasta", o, self.recipes, self.start, self.end, fasta)

    def verify(self, orc):
        """the four assertions per read -> (the oracle's records, its counters, the reads the batched kernel's fallback takes)"""
        o = self.options()
        res, cnt = orc.process_batch(self.config(orc), self.seq, self.qual, self.off, max_cycles=self.C)
        n_fallback = 0
        for i, (r, (s, q)) in enumerate(zip(self.recipes, self.reads)):
            tag = (self.name, i, r.note)
            alive, ms, me, steps = model_trim_and_cut(s, q, o)
            verdict = None
            if alive and o.polyx:
                verdict, psteps = model_polyx(s[ms:me], o.polyx_min_len)
                steps.update(psteps)
            # 1. the model gives the promise
            assert alive == r.alive, tag
            if alive:
                assert (ms, me) == tuple(r.win), (tag, ms, me)
                assert verdict == r.poly, (tag, verdict)
            # 2. the oracle's direct entries give what the model gives
            d = orc.trim_and_cut(s.tobytes(), q.tobytes(), o)
            assert (d is not None) == alive, tag
            if alive:
                assert (d[0], len(d[1])) == (ms, me - ms) or (ms == 0 and d[0] == 0 and len(d[1]) == me), (tag, d[0], len(d[1]))
                if o.polyx:
                    left, called, poly, tl = orc.trim_polyx(s[ms:me].tobytes(), None, o.polyx_min_len)
                    assert ((poly, tl) if called else None) == verdict and len(left) == me - ms - (tl if called else 0), (tag, called, poly, tl)
            # 3. the oracle's batch record is the promised one
            assert bool(res["dropped"][i]) == (not alive), tag
            if alive:
                e = me - (verdict[1] if verdict else 0)
                want = tuple(r.after) if r.after else (ms, e)
                if r.copy:
                    mode, c = r.copy
                    ad = np.frombuffer((self.start if mode == "start" else self.end).encode(), np.uint8)
                    hit = tsc.window_rule(s[ms:e], ad, mode)[0]
                    assert hit == c.pos, (tag, hit, c.pos)
                got = (int(res["r1_start"][i]), int(res["r1_start"][i]) + int(res["r1_len"][i]))
                assert got == want, (tag, got, want)
            # 4. the scans ended at the steps the recipe names
            for k, v in r.steps.items():
                assert steps.get(k) == v, (tag, k, steps.get(k), v)
            n_fallback += falls_back(steps, o)
        return res, cnt, n_fallback


_verified = {}


def verified(orc, key, make):
    """a battery, the oracle's results for it and its predicted fallback count, built and checked once per session"""
    if key not in _verified:
        b = make()
        _verified[key] = (b,) + b.verify(orc)
    return _verified[key]


# ---- A. the first good window, front and tail --------------------------------------------------------------------------------------

A_STEPS = list(range(18)) + [31, 32, 33, 63, 64, 65] + list(range(158, 164))
A_WINDOWS = [1, 2, 4, 5, 15, 16, 17, 50]
A_TRIMS = [(0, 0), (3, 0), (0, 2), (3, 2)]


def front_read(k, w, tf, tt, exact, body=40, note=""):
    """trim_front bases, k bases below the threshold, then the deciding window: a tuned byte and w - 1 bytes of HI, summing to the
    threshold exactly (the scan stops at step k) or to one less (it stops at k + 1, on a window of HI alone)"""
    l = tf + k + w + body + tt
    st = k if exact else k + 1
    s = tf + st
    if s > 0:
        s += w - 1
    return Recipe([seg(tf + k, LO), seg(w + body, HI), seg(tt, LO)], True, (s, l - tt), steps={"cf": st},
                  tune=((tf + k, T - (w - 1) if exact else T - w),), note=note or "front k=%d w=%d %s" % (k, w, "thr" if exact else "thr-1"))


def tail_read(k, w, tf, tt, exact, body=40, note=""):
    l = tf + body + w + k + tt
    st = k if exact else k + 1
    t = l - tt - 1 - st
    if t < l - 1:
        t = t - w + 1
    return Recipe([seg(tf, LO), seg(body + w, HI), seg(k + tt, LO)], True, (tf, t + 1), steps={"ct": st},
                  tune=((l - tt - 1 - k, T - (w - 1) if exact else T - w),), note=note or "tail k=%d w=%d %s" % (k, w, "thr" if exact else "thr-1"))


def first_window_battery(side, w, tf=0, tt=0):
    """the scan stops at each step of A_STEPS, and where its window (and, with lanes = positions, the round of 64 candidates it
    belongs to) crosses the 256 staged bytes of the read's head / tail; two of the reads are longer than 512 bases, so that head and
    tail are two windows"""
    make = front_read if side == "front" else tail_read
    edge = (tt if side == "tail" else tf)
    cross = sorted({190, 192, 255 - w - edge, 256 - w - edge, 257 - w - edge, 256 - edge})
    rs = [make(k, w, tf, tt, exact) for k in A_STEPS + cross for exact in (True, False)]
    rs += [make(k, w, tf, tt, True, body=300) for k in (5, 256 - w - edge)]
    opt = dict(trim_front=tf, trim_tail=tt)
    opt.update(dict(cut_front=1, cut_front_window=w) if side == "front" else dict(cut_tail=1, cut_tail_window=w))
    return Battery("A-%s-w%d-%d-%d" % (side, w, tf, tt), opt, rs)


# ---- B. where a scan runs out -----------------------------------------------------------------------------------------------------

def _ran_out_front(l, w, tf, tt):
    """cut_front alone on a read with no good window: s runs to lim = l - tt - w and the cut point is the base before trim_tail"""
    if l - tf - tt - w <= 0:
        return Recipe([seg(l, BAD)], False, note="front: no room, l=%d" % l)
    n = l - tt - w - tf
    return Recipe([seg(l, BAD)], tt > 0, (l - tt - 1, l - tt), steps={"cf": n}, note="front ran out after %d, l=%d tt=%d" % (n, l, tt))


def _last_front(l, w, tf, tt):
    """... and with the LAST window good: it ends one base short of trim_tail (the loop runs while s + w < l - tt)"""
    k = l - tt - w - tf - 1
    s = tf + k + (w - 1 if tf + k > 0 else 0)
    return Recipe([seg(tf + k, BAD), seg(w, HI), seg(1 + tt, BAD)], True, (s, l - tt), steps={"cf": k}, note="front: last window, l=%d tt=%d" % (l, tt))


def _ran_out_tail(l, w, tf, tt):
    """cut_tail alone with no good window: t runs down to front + w - 1 and one base is left, the one at front"""
    if l - tf - tt - w <= 0:
        return Recipe([seg(l, BAD)], False, note="tail: no room, l=%d" % l)
    n = l - tt - tf - w
    return Recipe([seg(l, BAD)], tf < l - 1, (tf, tf + 1), steps={"ct": n}, note="tail ran out after %d, l=%d" % (n, l))


def _last_tail(l, w, tf, tt):
    k = l - tt - tf - w - 1  # the window [tf + 1, tf + w] (the one that starts AT front is never tested)
    return Recipe([seg(tf + 1, BAD), seg(w, HI), seg(l - tf - 1 - w, BAD)], True, (tf, tf + 2) if (k > 0 or tt > 0) else (tf, l),
                  steps={"ct": k}, note="tail: last window, l=%d tt=%d" % (l, tt))


def run_out_battery(side, w, tf, tt):
    room = [0, 1, 2, 15, 16, 17, 40, 159, 160, 161, 162]
    ran, last = (_ran_out_front, _last_front) if side == "front" else (_ran_out_tail, _last_tail)
    rs = [ran(tf + tt + w + x, w, tf, tt) for x in room]
    rs += [last(tf + tt + w + x, w, tf, tt) for x in room if x > 0]
    # both sides of the block load: front + w + 15 <= l, and t = l - tt - 1 >= w + 14
    for l in sorted({tf + w + 14, tf + w + 15, tf + w + 16, tf + w + 17, w + 13 + tt + 1, w + 14 + tt + 1, w + 15 + tt + 1}):
        if l - tf - tt - w > 1:
            rs += [ran(l, w, tf, tt), last(l, w, tf, tt)]
    opt = dict(trim_front=tf, trim_tail=tt)
    opt.update(dict(cut_front=1, cut_front_window=w) if side == "front" else dict(cut_tail=1, cut_tail_window=w))
    return Battery("B-%s-w%d-%d-%d" % (side, w, tf, tt), opt, rs)


def stretch_battery(w):
    """both cuts on, a good stretch of g bases between two bad ends.  g < w: no window, dropped.  w <= g < 2 w: cut_front stops at
    the stretch and moves to its w-th base; every window cut_tail may test lies behind that base and has a bad byte, so it runs out
    and one base is left.  g = 2 w: cut_tail finds the stretch's last window and leaves two bases"""
    a, b = 9, 3 * w + 30
    rs = []
    for g in sorted({w - 1, w, w + 1, w + 2, 2 * w - 1, 2 * w}):
        l = a + g + b
        segs = [seg(a, BAD), seg(g, HI), seg(b, BAD)]
        if g < w:
            rs.append(Recipe(segs, False, steps={"cf": l - w}, note="stretch %d" % g))
            continue
        f = a + w - 1
        if g < 2 * w:
            rs.append(Recipe(segs, True, (f, f + 1), steps={"cf": a, "ct": (l - 1) - (f + w - 1)}, note="stretch %d" % g))
        else:
            rs.append(Recipe(segs, True, (f, f + 2), steps={"cf": a, "ct": b}, note="stretch %d" % g))
    return Battery("B-stretch-w%d" % w, dict(cut_front=1, cut_tail=1, cut_front_window=w, cut_tail_window=w), rs)


# ---- C. the N skips and the quirks --------------------------------------------------------------------------------------------------

C_RUNS = [0, 1, 2, 63, 64, 65, 159, 160, 161, 162]


def _n_read(n, m, w=4, a=5, b=6, body=30):
    """a bad bases, the first good window, n N's from its last base's place on (the cut point s + w - 1 itself holds a base of the
    window: the run starts there), filler, m N's that END at the tail's cut point t - w + 1, the last good window, b bad bases"""
    segs = [seg(a, BAD), seg(w - 1), seg(n, HI, "N"), seg(body), seg(m, HI, "N"), seg(w - 1), seg(b, BAD)]
    l = a + w - 1 + n + body + m + w - 1 + b
    # the front window is [a, a + w): its last byte is the first N (or filler); the tail window is [t - w + 1, t], t = l - b - 1
    s = a + w - 1 + n
    e = l - b - (w - 1) - m
    return Recipe(segs, True, (s, e), steps={"cf": a, "cf_n": n, "ct": b, "ct_n": m}, note="N runs %d / %d" % (n, m))


def n_skip_battery(w=4):
    rs = [_n_read(n, n, w) for n in C_RUNS] + [_n_read(n, 0, w) for n in C_RUNS[1:]] + [_n_read(0, n, w) for n in C_RUNS[1:]]
    a, b = 5, 6
    # the N run reaches the read's end: s runs to l, and cut_tail finds no room
    rs.append(Recipe([seg(a, BAD), seg(w - 1), seg(20, HI, "N")], False, steps={"cf": a, "cf_n": 20}, note="N run to the read's end"))
    # the tail's N run reaches down to one base behind `front`: that base is left
    f = a + w - 1
    rs.append(Recipe([seg(a, BAD), seg(w), seg(25, HI, "N"), seg(w - 1), seg(b, BAD)], True, (f, f + 1), steps={"cf_n": 0, "ct_n": 25},
                     note="tail N run ends one base behind front"))
    # lower-case n is not skipped, at either end
    rs.append(Recipe([seg(a, BAD), seg(w - 1), seg(3, HI, "n"), seg(30), seg(3, HI, "n"), seg(w - 1), seg(b, BAD)], True,
                     (a + w - 1, a + w - 1 + 3 + 30 + 3), steps={"cf_n": 0, "ct_n": 0}, note="lower-case n"))
    # good-quality N's only: the front scan stops at once, s = 0 stays (the `if (s > 0)` quirk), the skip runs to l
    rs.append(Recipe([seg(40, HI, "N")], False, steps={"cf": 0, "cf_n": 40}, note="N only"))
    rs.append(Recipe([seg(200, HI, "N")], False, steps={"cf": 0, "cf_n": 200}, note="N only, 200"))
    return Battery("C-skips-w%d" % w, dict(cut_front=1, cut_tail=1, cut_front_window=w, cut_tail_window=w), rs)


def tail_reaches_front_battery(tf, w=4):
    """cut_tail alone: the tail's N run reaches `front` itself (nothing is left: dropped), or stops one base short of it"""
    b = 6
    rs = []
    for n in (10, 70):
        rs.append(Recipe([seg(tf, HI), seg(n, HI, "N"), seg(w - 1), seg(b, BAD)], False, steps={"ct": b, "ct_n": n},
                         note="N AT front, run of %d" % n))
        rs.append(Recipe([seg(tf + 1, HI), seg(n, HI, "N"), seg(w - 1), seg(b, BAD)], True, (tf, tf + 1), steps={"ct_n": n},
                         note="N from front + 1, run of %d" % n))
    return Battery("C-tail-to-front-%d" % tf, dict(trim_front=tf, cut_tail=1, cut_tail_window=w), rs)


def quirks_battery(tf, tt, w=4):
    """first and last window good: `if (s > 0)` keeps s = 0 where it is and moves any other s on by w - 1; `if (t < l - 1)` keeps the
    read's last base and moves any other t back"""
    l = 60
    s = 0 if tf == 0 else tf + w - 1
    e = l if tt == 0 else l - tt - 1 - w + 1 + 1
    rs = [Recipe([seg(l)], True, (s, e), steps={"cf": 0, "ct": 0}, note="all good")]
    # ... and an N where that lands
    segs = [seg(s), seg(2, HI, "N"), seg(e - s - 4), seg(2, HI, "N"), seg(l - e)]
    rs.append(Recipe(segs, True, (s + 2, e - 2), steps={"cf": 0, "ct": 0, "cf_n": 2, "ct_n": 2}, note="all good, N at both cut points"))
    return Battery("C-quirks-%d-%d" % (tf, tt), dict(trim_front=tf, trim_tail=tt, cut_front=1, cut_tail=1, cut_front_window=w, cut_tail_window=w), rs)


def front_at_end_battery():
    """front >= l - 1 with a window of one: trim_front = l - 2 leaves two bases; the first is bad, so the cut lands on the last base"""
    rs = [Recipe([seg(5, BAD), seg(1, HI)], False, steps={"cf": 1}, note="front = l - 1"),
          Recipe([seg(5, BAD), seg(2, HI)], True, (5, 7), steps={"cf": 1}, note="front = l - 2")]
    return Battery("C-front-at-end", dict(trim_front=4, cut_front=1, cut_front_window=1), rs)


# ---- D. polyX ----------------------------------------------------------------------------------------------------------------------

def _guard(x):
    """twelve bases without x, which stop the scan: at most five mismatches are allowed"""
    return "".join(c for c in "CGTA" if c != x)


def _px_end(n, min_len, more=0):
    """where the scan ends behind n matching bases (of which `more` are mismatches already) followed by mismatches only"""
    j = 0
    while True:
        pos = n + j
        if j + 1 + more > min(5, (pos + 1) // 8) and (pos >= 8 or pos + 1 >= min_len - 1):
            return pos
        j += 1


def tail_read_px(x, n, min_len, lead=60, note=""):
    """filler, a guard, n bases of x"""
    P = _px_end(n, min_len)
    called = P + 1 >= min_len and n > 0
    return Recipe([seg(lead), seg(12, HI, _guard(x)), seg(n, HI, x)], True, (0, lead + 12 + n),
                  (POLY.index(x), n) if called else None, steps={"px": P}, note=note or "poly%s of %d" % (x, n))


def polyx_lengths_battery(min_len, bases="ATCG", full=True):
    ns = [0, 3, min_len - 3, min_len - 2, min_len - 1, min_len, min_len + 1, 31, 32, 33] + list(range(159, 164))
    if full:
        ns += [15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129]
    rs = [tail_read_px(x, n, min_len) for x in bases for n in sorted(set(ns))]
    for x in bases:
        # the whole read: nothing stops the scan, the way back meets x at the read's first base, r1 is left with no base
        for n in (12, 40, 160, 161):
            if n + 1 >= min_len:
                rs.append(Recipe([seg(n, HI, x)], True, (0, n), (POLY.index(x), n), steps={"px": n, "walk": 0}, note="poly%s, the whole read of %d" % (x, n)))
        # r1 of 31, 32 and 33 bases: the block of 32 is loaded from 32 on
        for l in (31, 32, 33):
            rs.append(Recipe([seg(l - 12 - 12), seg(12, HI, _guard(x)), seg(12, HI, x)], True, (0, l), (POLY.index(x), 12) if _px_end(12, min_len) + 1 >= min_len else None,
                             note="poly%s of 12 in r1 of %d" % (x, l)))
    return Battery("D-lengths-%d" % min_len, dict(polyx=1, polyx_min_len=min_len), rs)


def _tail_with(x, n, places, ch):
    """n bases of x with `ch` at the given positions counted from the read's end -> segments"""
    t = [x] * n
    for p in places:
        t[n - 1 - p] = ch
    return "".join(t)


def polyx_mismatch_battery(min_len=10):
    rs = []
    lead = [seg(60), seg(12, HI, "CGT")]
    for c in (8, 16, 24, 32, 40, 48, 56):
        reg = [8 * i - 1 for i in range(1, min(5, c // 8) + 1)]  # a mismatch as the 8th, 16th ... base: the count is the allowance
        n = c + 6
        rs.append(Recipe(lead + [seg(n, HI, _tail_with("A", n, reg, "C"))], True, (0, 72 + n), (0, n), steps={"px": _px_end(n, min_len, len(reg))},
                         note="allowed mismatches up to %d" % c))
        over = reg + [c if c <= 40 else c - 1]  # one more: behind the last allowed one, or (the cap of five) as the 48th / 56th base
        P = max(over)
        rs.append(Recipe(lead + [seg(n, HI, _tail_with("A", n, over, "C"))], True, (0, 72 + n), (0, c - 1) if P + 1 >= min_len else None, steps={"px": P},
                         note="one mismatch too many at %d" % (P + 1)))
    # a mismatch as the read's very last base: nothing stops the scan before position 8, where one is allowed
    rs.append(Recipe(lead + [seg(20, HI, _tail_with("A", 20, [0], "C"))], True, (0, 92), (0, 20), note="mismatch as the last base"))
    # N counts for all four bases, below step 32, beyond it and beyond 64
    rs.append(Recipe([seg(60), seg(12, HI, _guard("G")), seg(80, HI, _tail_with("G", 80, [5, 40, 70], "N"))], True, (0, 152), (3, 80), steps={"px": _px_end(80, min_len)}, note="N in the tail"))
    for p in (5, 40, 70):  # ... where a lost N is one mismatch too many
        reg = [7, 15, 23, 31, 39]
        t = list(_tail_with("T", 80, reg, "C"))
        t[80 - 1 - p] = "N"
        rs.append(Recipe([seg(60), seg(12, HI, _guard("T")), seg(80, HI, "".join(t))], True, (0, 152), (1, 80), steps={"px": _px_end(80, min_len, 5)}, note="N at %d among the allowed mismatches" % p))
    # lower-case a is not counted: two of them as the 8th and 9th base stop the scan at position 8, short of min_len
    rs.append(Recipe(lead + [seg(20, HI, _tail_with("A", 20, [7, 8], "a"))], True, (0, 92), None, steps={"px": 8}, note="lower-case a"))
    return Battery("D-mismatch", dict(polyx=1, polyx_min_len=min_len), rs)


def _tie(x, y):
    """from the end: 15 N, y, x, 6 N, y, x, 5 N behind a lower-case guard that counts for nobody: x and y have the same count when
    the scan ends at position 32; x lies deeper, at position 24"""
    t = ["N"] * 30
    for p, ch in ((15, y), (16, x), (23, y), (24, x)):
        t[29 - p] = ch
    return "".join(t)


def polyx_tie_battery(min_len=10):
    lead = [seg(60), seg(12, HI, "acgt")]
    rs = []
    for x, y in (("A", "T"), ("T", "A"), ("C", "G"), ("G", "C"), ("A", "G"), ("G", "A"), ("T", "C"), ("T", "G")):
        win = min(x, y, key=POLY.index)
        rs.append(Recipe(lead + [seg(30, HI, _tie(x, y))], True, (0, 102), (POLY.index(win), 25 if win == x else 24), steps={"px": 32},
                         note="tie of %s and %s" % (x, y)))
    # N only: every count is the same, A is taken, the way back meets no A and nothing is cut -- yet the read is booked, with 0 bases
    for n in (40, 160, 161, 200):
        rs.append(Recipe([seg(n, HI, "N")], True, (0, n), (0, 0), steps={"px": n, "walk": n}, note="N only, %d" % n))
    return Battery("D-ties", dict(polyx=1, polyx_min_len=min_len), rs)


def polyx_behind_cut_battery(w=4, min_len=10):
    """the polyX scan starts at the cut e, not at l: behind a cut_tail that took six bad bases and w - 1 of the tail, and behind an N
    skip that ended at the tail's last base"""
    rs = []
    for x in "AG":
        for n in (20, 40, 170, 260):  # (260: the scan's fourth round of 64 starts inside the staged tail and ends in front of it)
            l = 72 + n + 6
            e = l - 6 - (w - 1)
            rs.append(Recipe([seg(60), seg(12, HI, _guard(x)), seg(n, HI, x), seg(6, BAD)], True, (0, e), (POLY.index(x), n - (w - 1)),
                             steps={"ct": 6, "px": _px_end(n - (w - 1), min_len)}, note="poly%s of %d behind a cut" % (x, n)))
            e = 72 + n
            rs.append(Recipe([seg(60), seg(12, HI, _guard(x)), seg(n, HI, x), seg(5, HI, "N"), seg(w - 1), seg(6, BAD)], True, (0, e), (POLY.index(x), n),
                             steps={"ct": 6, "ct_n": 5, "px": _px_end(n, min_len)}, note="poly%s of %d behind an N skip" % (x, n)))
    return Battery("D-behind-cut", dict(cut_tail=1, cut_tail_window=w, polyx=1, polyx_min_len=min_len), rs)


# ---- E. waves ------------------------------------------------------------------------------------------------------------------------

def wave_mix_battery(order, w=4):
    """one group of 64 reads whose lanes end at step 0, 1, 15, 16, 17 and beyond the cap, are not alive or are too short for the
    block; order 0 puts the slow lanes at lane 0 and in between, order 1 (reversed) at lane 63"""
    kinds = [lambda: front_read(170, w, 0, 0, True), lambda: front_read(0, w, 0, 0, True), lambda: front_read(1, w, 0, 0, False),
             lambda: front_read(15, w, 0, 0, True), lambda: _ran_out_front(w, w, 0, 0), lambda: front_read(16, w, 0, 0, True),
             lambda: front_read(2, w, 0, 0, True, body=3), lambda: front_read(17, w, 0, 0, False), lambda: front_read(161, w, 0, 0, True),
             lambda: _ran_out_front(w + 9, w, 0, 0), lambda: front_read(15, w, 0, 0, False)]
    rs = [kinds[i % len(kinds)]() for i in range(64)]
    if order:
        rs.reverse()
    return Battery("E-mix-%d" % order, dict(cut_front=1, cut_front_window=w, polyx=1), rs)


def ragged_battery(w=4):
    """129 reads of which batches of 1, 63, 64, 65 and 129 are run: front and tail cuts and polyX tails by turns"""
    rs = []
    for i in range(129):
        k = (i * 7) % 40
        n = 20 + (i * 5) % 50
        a = front_read(k, w, 0, 0, i % 2 == 0, body=30)
        l = k + w + 30 + 12 + n + 6
        e = l - 6 - (w - 1)
        rs.append(Recipe(a.segs[:2] + [seg(12, HI, "CGT"), seg(n, HI, "A"), seg(6, BAD)], True, (a.win[0], e), (0, n - (w - 1)),
                         steps=dict(a.steps, ct=6), tune=a.tune, note="ragged %d" % i))
    return Battery("E-ragged", dict(cut_front=1, cut_tail=1, cut_front_window=w, cut_tail_window=w, polyx=1), rs)


# ---- F. the windows the adapter trims inherit ------------------------------------------------------------------------------------

F_CUTS = [55, 56, 57, 58]
ALEN = len(tsc.START)


def _start_after(rlen, m):
    return min(rlen - 1, min(m + tsc.EXT, rlen - ALEN) + ALEN)


def inherit_start_battery(how, L=560):
    """a front cut of exactly 55..58 bases (the start window r1[0, 200) lies in the 256 staged bytes of the read's head up to a cut
    of 56), with a start-adapter copy at the last tested position of that window, and one at position 0.  how: "cut" (cut_front, a
    window of four) or ("trim", c) (trim_front = c alone)"""
    rs = []
    for c in (F_CUTS if how == "cut" else [how[1]]):
        for pos in (tsc.WINDOW - ALEN, 0):
            for l in (L, 300):
                rlen = l - c
                ns = _start_after(rlen, pos)
                cp = ("start", tsc.Copy(pos))
                if how == "cut":
                    k = c - 3
                    rs.append(Recipe([seg(k, BAD), seg(l - k)], True, (c, l), steps={"cf": k}, copy=cp, after=(c + ns, l), note="cut of %d, copy at %d, l=%d" % (c, pos, l)))
                else:
                    rs.append(Recipe([seg(l)], True, (c, l), copy=cp, after=(c + ns, l), note="trim_front %d, copy at %d, l=%d" % (c, pos, l)))
    opt = dict(cut_front=1, cut_front_window=4) if how == "cut" else dict(trim_front=how[1])
    return Battery("F-start-%s" % (how if how == "cut" else "trim%d" % how[1]), opt, rs, tsc.START, tsc.END)


def inherit_end_battery(how, L=560):
    """the mirror: cut_tail, polyX or trim_tail take exactly 55..58 bases (the end window lies in the staged tail up to 56), with an
    end-adapter copy at the first tested position of r1's last 200 bases"""
    rs = []
    for c in (F_CUTS if how in ("cut", "polyx") else [how[1]]):
        for l in (L, 300):
            if how == "cut":
                k = c - 3
                e = l - c
                r = Recipe([seg(l - k), seg(k, BAD)], True, (0, e), steps={"ct": k})
            elif how == "polyx":
                e = l - c
                r = Recipe([seg(l - c - 12), seg(12, HI, "CGT"), seg(c, HI, "A")], True, (0, l), (0, c))
            else:
                e = l - c
                r = Recipe([seg(l)], True, (0, e))
            pos = e - tsc.WINDOW
            r.copy, r.after, r.note = ("end", tsc.Copy(pos)), (0, max(0, pos - tsc.EXT)), "%s of %d, copy at %d, l=%d" % (how, c, pos, l)
            rs.append(r)
    opt = dict(cut_tail=1, cut_tail_window=4) if how == "cut" else (dict(polyx=1) if how == "polyx" else dict(trim_tail=how[1]))
    return Battery("F-end-%s" % (how if isinstance(how, str) else "trim%d" % how[1]), opt, rs, tsc.START, tsc.END)


FASTA = ["TTGACCAGTAGGCATCAGGATCCA", "GGTCATTCAGGCTAAGCTTCGGAATCCGTTAGCA"]  # the two-entry list behind batteries A, C and D
