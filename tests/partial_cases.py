"""Test helpers shared by tests/test_partial_emu.py and tests/test_gpu_partial.py: reads built so that what runs BEHIND a window scan
of the end trims decides the outcome -- the partial-pattern searches of trimBySequenceStart / trimBySequenceEnd (the adapter's last /
first 16 bases against every 16-base window of r1's first / last 200 bases) and the edit-distance confirmations (lev_lanes32 /
lev_lanes64 with lane = read, lev_wave_core with lanes = columns; fastplong_amd/csrc/kernels.h).  No kernel code is imported here.

A recipe is one read: deterministic filler with pieces laid over it (pattern copies, flanks) and a promise -- the position and distance
the search of each end chooses, cmplen, whether the confirmation passes, r1 afterwards, the returned count, the key length booked in
the adapter histogram and the candidate columns a lane of k_trim_ends_batched consumes.  A promise names the fields the recipe is
about; Battery.verify asserts for every read, before a kernel sees it, that the plain model below gives every promised field, that
the oracle's direct entries (trim_start / trim_end: sequence, count, key length) give what the model gives, that the oracle's batch
record is the model's r1, and that the full-match search finds nothing unless the promise says it does.  Nothing is random, nothing is
rebuilt and nothing is left out: a promise that does not hold is a bug in the recipe.

The model: the two reference loops written literally over the Wagner-Fischer distance of every window; a semi-global DP row (first
row all zero) that yields the candidate columns `score <= thr` of partial16_candidates; and a replay of a lane's walk over those
columns (partial16_resolve_lanes), which must choose what the literal loop chooses and counts every column it consumes -- tested or
not -- so that the reads k_trim_ends_batched hands to its wave search (more than PART_CAND_CAP = 10 columns) are known beforehand."""
import math
from dataclasses import dataclass, field

import numpy as np

from fastplong_amd import abi, synth
from tests import scan_cases as sc
from tests import trim_scan_cases as tsc
from tests.scan_cases import random_adapter

START, END = tsc.START, tsc.END
PLEN = tsc.PLEN
WINDOW = tsc.WINDOW
CAP = 10           # PART_CAND_CAP: a lane may consume this many candidate columns
FILL = "ACGT"
Q = ord("I")       # flat and high


def thr_at(ed_max, n):
    """round(edMax * n) of the reference: half-way cases go up (round(0.25 * 18) = 5, round(0.25 * 22) = 6)"""
    return int(math.floor(ed_max * n + 0.5))


assert tsc.thr_of(18) == thr_at(0.25, 18) == 5 and thr_at(0.25, 22) == 6 and thr_at(0.25, 16) == 4


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def window_distances(r1, pat, mode):
    """Wagner-Fischer, all windows at once: ed[p] of r1[p, p + plen) (start) / r1[rlen - plen - p, rlen - p) (end) against pat, for
    the p the reference's loop tests: p < rlen - plen && p < 200 - plen"""
    rlen, plen = len(r1), len(pat)
    lim = max(0, min(rlen - plen, WINDOW - plen))
    if lim == 0:
        return []
    p = np.arange(lim)
    base = p if mode == "start" else rlen - plen - p
    a = np.frombuffer(bytes(r1), np.uint8)
    prev = np.tile(np.arange(plen + 1), (lim, 1))  # row i = 0 of every window: D[0][j] = j
    for i in range(1, plen + 1):                   # i: text byte i of the window, j: pattern base j
        t = a[base + i - 1]
        cur = np.empty_like(prev)
        cur[:, 0] = i
        for j in range(1, plen + 1):
            cur[:, j] = np.minimum(np.minimum(prev[:, j], cur[:, j - 1]) + 1, prev[:, j - 1] + (t != pat[j - 1]))
        prev = cur
    return [int(x) for x in prev[:, plen]]


def search_start(eds, thr):
    """src/adaptertrimmer.cpp:202-216 -> (pos, mined): the smallest distance, the first among equals"""
    pos, mined = -1, -1
    for p, ed in enumerate(eds):
        if ed <= thr:
            if pos < 0:
                pos, mined = p, ed
            elif ed >= mined:
                pass
            else:
                pos, mined = p, ed
    return pos, mined


def search_end(eds, thr):
    """:273-286 -> (pos, mined): walking in from the tail, stop at the first increase; a later equal wins"""
    pos, mined = -1, -1
    for p, ed in enumerate(eds):
        if ed <= thr:
            if pos < 0:
                pos, mined = p, ed
            elif ed > mined:
                break
            else:
                pos, mined = p, ed
    return pos, mined


def candidate_columns(text, pat, thr):
    """the semi-global row: D[0][j] = 0 (a match may start anywhere), D[i][0] = i -> the text columns j (0-based: the match ENDS at
    byte j) with D[plen][j + 1] <= thr"""
    plen = len(pat)
    col = list(range(plen + 1))
    out = []
    for j, c in enumerate(bytes(text)):
        new = [0] * (plen + 1)
        for i in range(1, plen + 1):
            new[i] = min(col[i] + 1, new[i - 1] + 1, col[i - 1] + (pat[i - 1] != c))
        col = new
        if col[plen] <= thr:
            out.append(j)
    return out


def lane_walk(r1, pat, mode, thr, eds):
    """a lane of partial16_resolve_lanes -> (pos, mined, columns consumed were there no cap).  Start: all columns ascending.  End:
    descending until the stop rule fires; the column that fires it is consumed"""
    rlen = len(r1)
    n = min(rlen, WINDOW)
    lim = min(rlen - PLEN, WINDOW - PLEN)
    text = r1[:n] if mode == "start" else r1[rlen - n:]
    cols = candidate_columns(text, pat, thr)
    pos, mined, used = -1, -1, 0
    for j in (cols if mode == "start" else reversed(cols)):
        used += 1
        p = j - 15 if mode == "start" else n - 1 - j
        if not (0 <= p < lim):
            continue  # (consumed, never tested)
        ed = eds[p]
        if ed > thr:
            continue
        if mode == "start":
            if pos < 0 or ed < mined:
                pos, mined = p, ed
        elif pos < 0 or ed <= mined:
            pos, mined = p, ed
        else:
            break
    return pos, mined, used


def full_match(r1, ad, mode, thrA):
    """searchAdapter as the end trims call it -> (the position of the full match or None, whether a candidate's edit distance was
    taken).  The Hamming profile and the tested positions are trim_scan_cases.window_rule's; the threshold is this battery's"""
    r1 = np.frombuffer(bytes(r1), np.uint8)
    _, _, mm, pos = tsc.window_rule(r1, ad, mode)
    if len(pos) == 0:
        return None, False
    hits = pos[mm <= thrA]
    if len(hits):
        return int(hits.max() if mode == "start" else hits.min()), False
    mins = pos[mm == mm.min()]
    cand = int(mins.min() if mode == "start" else mins.max())
    return (cand if tsc.edit_distance(bytes(r1[cand:cand + len(ad)]), bytes(ad)) <= thrA else None), True


def model_trim(r1, adapter, mode, ed_max, ext, skip_full=False):
    """one end trim of r1 (bytes) -> dict: full (position or None), wants (the partial search runs), pos / mined (its choice; the END
    search's pos before the strict `pos > 0`), cmplen, ok (the confirmation passes), cols / over (lane walk; adapters of >= 16
    bases), left = (s, e) of r1 afterwards, count (the value returned) and key (the length booked)"""
    r1 = bytes(r1)
    rlen, alen = len(r1), len(adapter)
    ad = np.frombuffer(adapter.encode(), np.uint8)
    out = dict(full=None, wants=False, pos=-1, mined=-1, cmplen=0, ok=False, cols=0, over=False, left=(0, rlen), count=0, key=0)
    out["cand"] = False
    if rlen < PLEN:
        return out
    plen = min(PLEN, alen)
    m, out["cand"] = (None, False) if skip_full else full_match(r1, ad, mode, thr_at(ed_max, alen))  # (skip_full: only while a recipe is being built)
    if m is not None:
        out["full"] = m
        out["key"] = alen
        if mode == "start":
            x = min(m + ext, rlen - alen) + alen
            n = min(rlen - 1, x)
            out["left"], out["count"] = ((rlen, rlen) if n < 0 else (n, rlen)), x
        else:
            mp = max(0, m - ext)
            out["left"], out["count"] = (0, mp), rlen - mp
        return out
    out["wants"] = True
    pat = bytes(ad[alen - plen:]) if mode == "start" else bytes(ad[:plen])
    thrP = thr_at(ed_max, plen)
    eds = window_distances(r1, pat, mode)
    pos, mined = (search_start if mode == "start" else search_end)(eds, thrP)
    if plen == PLEN:
        lp, lm, used = lane_walk(r1, pat, mode, thrP, eds)
        assert (lp, lm) == (pos, mined), ("the lane walk and the reference loop disagree", mode, lp, lm, pos, mined)
        out["cols"], out["over"] = used, used > CAP
    out["pos"], out["mined"], out["found"] = pos, mined, pos >= 0
    out["nearest"] = min(eds, default=None)  # (the smallest distance of any tested window, qualifying or not)
    if pos < 0 or (mode == "end" and pos == 0):
        return out
    cmplen = min(pos + plen, alen)
    out["cmplen"] = cmplen
    if mode == "start":
        ed = tsc.edit_distance(r1[pos + plen - cmplen:pos + plen], bytes(ad[alen - cmplen:]))
    else:
        ed = tsc.edit_distance(r1[rlen - plen - pos:rlen - plen - pos + cmplen], bytes(ad[:cmplen]))
    out["ced"] = ed
    if ed > thr_at(ed_max, cmplen):
        return out
    out["ok"], out["key"] = True, cmplen
    if mode == "start":
        p2 = min(pos + ext, rlen - alen)  # (may be negative)
        n = min(rlen - 1, p2 + plen)      # Read::trimFront: a negative count erases the read
        out["left"], out["count"] = ((rlen, rlen) if n < 0 else (n, rlen)), p2 + plen
    else:
        p2 = min(pos + ext, rlen - plen)
        out["left"], out["count"] = (0, rlen - plen - p2), p2 + plen
    return out


# ---- recipes ------------------------------------------------------------------------------------------------------------------------

_fillers = {}


def filler_for(start, end, ed_max=0.25, L=720):
    """ACGT repeated when neither adapter's pattern has a qualifying window in it (true of the synth adapters); else the first seeded
    filler of which that holds.  Every substring of it is free of qualifying windows too"""
    key = (start, end, ed_max, L)
    if key not in _fillers:
        cands = [(FILL * (L // 4 + 1))[:L]] + ["".join("ACGT"[i] for i in np.random.default_rng(9000 + s).integers(0, 4, L)) for s in range(40)]
        for f in cands:
            bad = False
            for ad, mode in ((start, "start"), (end, "end")):
                if not ad:
                    continue
                plen = min(PLEN, len(ad))
                if plen < PLEN:
                    continue  # (a pattern of 8 bases within 2 edits occurs in any text of this length: such batteries promise no place)
                pat = (ad[-plen:] if mode == "start" else ad[:plen]).encode()
                bad = bad or bool(candidate_columns(f.encode(), pat, thr_at(ed_max, plen)))
            if not bad:
                _fillers[key] = f
                break
        assert key in _fillers, "no filler without a qualifying window for %s / %s" % (start, end)
    return _fillers[key]


def sub(s, places, k=1):
    """s with the bases at `places` replaced by the k-th next of A, C, G, T"""
    t = list(s)
    for p in places:
        t[p] = "ACGT"[("ACGT".index(t[p]) + k) % 4] if t[p] in "ACGT" else "A"
    return "".join(t)


@dataclass
class Recipe:
    L: int                       # bases of r1 (the read is trim_front + L + trim_tail)
    over: list                   # [(r1 position, text)]: laid over the filler in this order
    start: dict = field(default_factory=dict)  # the promise about the start trim: any of model_trim's fields
    end: dict = field(default_factory=dict)    # ... and the end trim (positions in the r1 the start trim leaves)
    r1: tuple = None             # (s, e) of r1 in the end, in r1 coordinates
    note: str = ""
    chain: dict = field(default_factory=dict)  # {(i, mode): promise} about the trims by entry i of a FASTA list
    mid: dict = field(default_factory=dict)    # battery G: the promise about findMiddleAdapters (model_middle's fields)

    def build(self, fill, front=0, tail=0):
        s = list(fill[:front + self.L + tail])
        assert len(s) == front + self.L + tail, (self.note, self.L)
        for p, t in self.over:
            assert -front <= p and p + len(t) <= self.L + tail, (self.note, p, len(t), self.L)  # (r1, or the bases trim_front / trim_tail take)
            s[front + p:front + p + len(t)] = t
        s = np.frombuffer("".join(s).encode(), np.uint8).copy()
        return s, np.full(len(s), Q, np.uint8)


class Battery:
    def __init__(self, name, recipes, start=START, end=END, opt=None, fasta=()):
        self.name, self.recipes, self.start, self.end, self.fasta = name, list(recipes), start, end, tuple(fasta)
        self.opt = dict(opt or {})
        self.cfgd = dict(opt=self.opt, start=start, end=end)
        self.front, self.tail = self.opt.get("trim_front", 0), self.opt.get("trim_tail", 0)
        o = self.options()
        self.ed_max, self.ext = float(o.ed_max), int(o.trimming_extension)
        self.fill = filler_for(start, end, self.ed_max, 2200 if any(r.L > 700 for r in self.recipes) else 720)
        assert 0 < len(self.recipes) <= 400
        self.reads = [r.build(self.fill, self.front, self.tail) for r in self.recipes]
        self.seq, self.qual, self.off = synth.pack(self.reads)
        self.C = int(np.diff(self.off.astype(np.int64)).max()) + 1
        self.models = None

    def options(self):
        return abi.FplOptions.default(**self.opt)

    def config(self, orc):
        return orc.Config(self.options(), self.start, self.end, self.fasta)

    def pick(self, idx, name):
        return Battery("%s-%s" % (self.name, name), [self.recipes[i] for i in idx], self.start, self.end, self.opt, self.fasta)

    def with_fasta(self, fasta):
        return Battery(self.name + "-fasta", self.recipes, self.start, self.end, self.opt, fasta)

    def steps(self):
        """the trims in the order they run: the two command-line adapters, then every entry of the FASTA list at both ends"""
        out = [("start", self.start, "start"), ("end", self.end, "end")]
        for i, a in enumerate(self.fasta):
            out += [((i, "start"), a, "start"), ((i, "end"), a, "end")]
        return out

    def model(self):
        """[[start trim, end trim, entry 0 at the start, entry 0 at the end, ...]] per read, every trim on what the one before leaves
        (None: no such adapter)"""
        if self.models is None:
            self.models = []
            for s, _ in self.reads:
                r1 = bytes(s[self.front:len(s) - self.tail])
                a, b = 0, len(r1)
                ms = []
                for _, ad, mode in self.steps():
                    m = model_trim(r1[a:b], ad, mode, self.ed_max, self.ext) if ad else None
                    if m:
                        a, b = a + m["left"][0], a + m["left"][1]
                    ms.append(m)
                self.models.append(ms)
        return self.models

    def verify(self, orc):
        """the four assertions per read -> (the oracle's records, its counters)"""
        res, cnt = orc.process_batch(self.config(orc), self.seq, self.qual, self.off, max_cycles=self.C)
        for i, (r, (s, _), ms) in enumerate(zip(self.recipes, self.reads, self.model())):
            tag = (self.name, i, r.note)
            r1 = bytes(s[self.front:len(s) - self.tail])
            a, b = 0, len(r1)
            for (which, ad, mode), m in zip(self.steps(), ms):
                if m is None:
                    continue
                want = r.start if which == "start" else (r.end if which == "end" else dict(r.chain.get(which, {}), full_any=True))
                # 1. the model gives the promise
                for k, v in want.items():
                    assert k == "full_any" or m.get(k) == v, (tag, mode, k, m.get(k), v)
                # 4. the full-match search finds nothing, unless the promise says where it does (full_any: the recipe is about the
                # confirmation of the window scan's candidate, and the model says whether it passes)
                assert (m["full"] is None) or "full" in want or "full_any" in want, (tag, mode, "full match at", m["full"])
                # 2. the oracle's direct entry gives what the model gives: sequence, count, key length
                left, count, key = (orc.trim_start if mode == "start" else orc.trim_end)(r1[a:b], ad, self.ed_max, self.ext)
                assert (left.encode(), count, key) == (r1[a:b][m["left"][0]:m["left"][1]], m["count"], m["key"]), (tag, mode, len(left), count, key, m)
                a, b = a + m["left"][0], a + m["left"][1]
            if r.r1 is not None:
                assert (a, b) == tuple(r.r1), (tag, (a, b), r.r1)
            # 3. the oracle's batch record is the model's r1
            assert not res["dropped"][i], tag
            got = (int(res["r1_start"][i]) - self.front, int(res["r1_start"][i]) - self.front + int(res["r1_len"][i]))
            assert got == (a, b), (tag, got, (a, b))
        return res, cnt

    # ---- which path k_trim_ends_batched takes, from the model's counts
    def paths(self):
        """-> dict: wants / handed per end (reads that ask for a partial search / that a lane hands to the wave search), searches (the
        lane-parallel searches: one per group of 64 and end in which some lane has a candidate column) and rounds (of each search:
        the largest count of its lanes, and 11 = CAP + 1 when a lane has more than CAP)"""
        out = dict(cands=[0, 0], wants=[0, 0], handed=[0, 0], searches=0, rounds=0)
        ms = self.model()
        for g0 in range(0, len(ms), 64):
            for e in (0, 1):
                out["cands"][e] += sum(m[e]["cand"] for m in ms[g0:g0 + 64] if m[e] is not None)
                grp = [m[e] for m in ms[g0:g0 + 64] if m[e] is not None and m[e]["wants"]]
                out["wants"][e] += len(grp)
                out["handed"][e] += sum(m["over"] for m in grp)
                most = max([m["cols"] for m in grp], default=0)
                if most:
                    out["searches"] += 1
                    out["rounds"] += min(most, CAP + 1)
        return out


_verified = {}


def verified(orc, key, make):
    """a battery and the oracle's results for it, built and checked once per session"""
    if key not in _verified:
        b = make()
        _verified[key] = (b,) + b.verify(orc)
    return _verified[key]


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------

def pat_of(adapter, mode):
    plen = min(PLEN, len(adapter))
    return adapter[-plen:] if mode == "start" else adapter[:plen]


def anti(s):
    """as many bases as s has, of the letter s holds least often.  (A flank that merely differs from s at every place will not do:
    sixteen matching pattern bases leave the full adapter's confirmation to the flank alone, and a shifted alignment of two mixed
    texts of eight bases is cheap)"""
    return min("ACGT", key=s.count) * len(s)


def piece(mode, ad, p0, L, copy=None, flank="anti"):
    """-> what to lay over the filler: the pattern of `ad` (or `copy`) in the window the search calls p0 -- r1[p0, p0 + 16) at the
    start, r1[L - 16 - p0, L - p0) at the end (a longer copy reaches further INTO the read) -- and beside it, where the rest of the
    adapter would stand (in front of the pattern at the start, behind it at the end; as many bases as fit), flank: "own" = the
    adapter's bases (a truncated adapter), "anti" = a base that differs at every place (the pattern alone: 16 filler bases could match
    by chance and hand the read to the full-match search), any other text = that text, None = the filler stays"""
    pat = pat_of(ad, mode)
    c = pat if copy is None else copy
    k = min(p0, len(ad) - len(pat))
    if mode == "start":
        whole = ad[:len(ad) - len(pat)]
        fl, a = whole[len(whole) - k:], p0
        fa = p0 - k
    else:
        whole = ad[len(pat):]
        fl, a = whole[:k], L - p0 - len(c)
        fa = a + len(c)
    over = []
    if k and flank:
        t = fl if flank == "own" else (anti(whole)[:k] if flank == "anti" else flank)
        assert len(t) == k
        over.append((fa, t))
    return over + [(a, c)]


def one_read(mode, p0, L, adapter=None, copy=None, flank="anti", note="", **want):
    ad = adapter or (START if mode == "start" else END)
    r = Recipe(L, piece(mode, ad, p0, L, copy, flank), note=note or "%s p0=%d L=%d %s" % (mode, p0, L, flank))
    getattr(r, mode).update({k: v for k, v in want.items() if v is not None})
    return r


def _one_sided(name, mode, rs, ad, opt=None):
    return Battery(name, rs, ad if mode == "start" else "", ad if mode == "end" else "", opt)


# ---- A. places -------------------------------------------------------------------------------------------------------------------------

A_PLACES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 167, 168, 182, 183]


def places_battery(mode, adapter=None, opt=None, L=300):
    """a perfect pattern copy at every place where a code path changes: alone (the confirmation sees no flank) and as the end of a
    truncated adapter (the confirmation passes; from alen - 16 on the whole adapter stands there and the full-match search takes it
    -- except at the end, where the window flush with the tail is not among those it tests)"""
    ad = adapter or (START if mode == "start" else END)
    alen = len(ad)
    rs = []
    for p0 in sorted(set(A_PLACES) | {alen - 17, alen - 16, alen - 15}):
        for flank in ("anti", "own"):
            if mode == "end" and p0 == 0:  # the search chooses 0, which `pos > 0` turns down
                w = dict(pos=0, mined=0, ok=False, count=0, key=0, left=(0, L))
            elif flank == "own" and p0 >= alen - 16 and mode == "start":
                w = dict(full=p0 - (alen - 16), key=alen)
            elif flank == "own" and p0 > alen - 16:
                w = dict(full=L - 16 - p0, key=alen)
            elif flank == "own":
                w = dict(pos=p0, mined=0, cmplen=p0 + 16, ok=True, key=p0 + 16)
            else:
                w = dict(pos=p0, mined=0, cmplen=min(p0 + 16, alen))
            rs.append(one_read(mode, p0, L, ad, flank=flank, **w))
    # 184 is not tested: its neighbours 182 and 183 qualify, and 183 is chosen; at 185 only 183 is left, at 187 nothing
    rs.append(one_read(mode, 184, L, ad, pos=183, mined=2, cmplen=alen))
    rs.append(one_read(mode, 185, L, ad, pos=183, mined=4, cmplen=alen))
    rs.append(one_read(mode, 187, L, ad, pos=-1))
    return _one_sided("A-places-%s-%d" % (mode, alen), mode, rs, ad, opt)


def last_window_battery(mode, L=300):
    """the window at 183 decides a trim: the whole adapter ends there at four edits (two substitutions in the pattern, a base of the
    flank lost and one entered), eight mismatches place by place -- and a decoy with seven substitutions elsewhere in the window is
    the full-match search's Hamming candidate, whose confirmation fails.  The partial search finds 183 and its confirmation of all
    24 bases passes; one window less and 182 is taken, one base short"""
    ad = START if mode == "start" else END
    own = ad[:8] if mode == "start" else ad[16:]
    fl = (own[1:] + "A") if mode == "start" else ("A" + own[:6] + own[7:])  # (start: base 0 lost, an A behind; end: an A in front, base 6 lost)
    decoy = sub(ad, (0, 2, 6, 8, 10, 12, 14) if mode == "start" else (0, 2, 4, 6, 8, 10, 12), 2)
    over = piece(mode, ad, 183, L, sub(pat_of(ad, mode), [2, 6]), fl) + [(40 if mode == "start" else L - 200 + 40, decoy)]
    r = Recipe(L, over, note="%s: the window at 183 trims" % mode)
    getattr(r, mode).update(full=None, cand=True, pos=183, mined=2, cmplen=24, ced=4, ok=True, count=209, key=24)
    return _one_sided("A-last-%s" % mode, mode, [r, one_read(mode, 183, L, ad, pos=183, mined=0)], ad)


A_LENGTHS = [16, 17, 18, 31, 32, 33, 47, 48, 49, 199, 200, 201, 216]


def lengths_battery(mode, opt=None):
    """r1 of 16 (no window is tested), 17, 18, 31..33, 47..49, 199..201 and 216 bases, so that n and lim fall on both sides of every
    16-column block and of the tail word; the copy at the first place the search tests, at the last, and at lim itself: flush with
    the far end of r1 (or of its 200 bases), which is not tested while its neighbours are"""
    ad = START if mode == "start" else END
    rs = []
    for L in A_LENGTHS:
        lim = min(L - 16, 184)
        if lim <= 0:
            rs.append(one_read(mode, 0, L, ad, pos=-1, wants=True))
            continue
        for p0 in sorted({0 if mode == "start" else 1, lim - 1}):
            if p0 < lim:
                rs.append(one_read(mode, p0, L, ad, pos=p0, mined=0))
        rs.append(one_read(mode, lim, L, ad, note="%s p0 = lim = %d L=%d" % (mode, lim, L), **(dict(pos=lim - 1, mined=2) if lim > 1 or mode == "start" else {})))
    return _one_sided("A-lengths-%s" % mode, mode, rs, ad, opt)


# ---- B. order --------------------------------------------------------------------------------------------------------------------------

S2, S3, S4 = (3, 11), (3, 8, 12), (2, 6, 10, 13)  # where a copy's substitutions go


def order_battery(mode, L=300):
    """two copies in one window.  Start: the smallest distance, the first of equals.  End: the one nearer the tail even when the
    farther one is better; it moves on to an equal one, and to a better one when no worse window lies between them"""
    ad = START if mode == "start" else END
    pat = pat_of(ad, mode)
    a, b = 30, 90
    rs = []

    def two(ca, cb, **w):
        r = Recipe(L, piece(mode, ad, a, L, ca) + piece(mode, ad, b, L, cb))
        getattr(r, mode).update(w)
        return r
    if mode == "start":
        rs.append(two(sub(pat, S2), pat, pos=b, mined=0))            # a worse one before a better one
        rs.append(two(pat, sub(pat, S2), pos=a, mined=0))            # the reverse
        rs.append(two(pat, pat, pos=a, mined=0, over=True))          # two equal ones: the first (and 18 columns)
        rs.append(two(sub(pat, S3), sub(pat, S3, 2), pos=a, mined=3))
        rs.append(two(sub(pat, S4), sub(pat, S3), pos=b, mined=3))
    else:  # (a is the nearer one)
        rs.append(two(sub(pat, S2), pat, pos=a, mined=2))
        rs.append(two(pat, sub(pat, S2), pos=a, mined=0))
        rs.append(two(pat, pat, pos=a, mined=0))
        rs.append(two(sub(pat, S3), sub(pat, S3, 2), pos=b, mined=3))
        rs.append(two(sub(pat, S4), sub(pat, S3), pos=b, mined=3))
        rs.append(two(sub(pat, S3), sub(pat, S4), pos=a, mined=3))     # ... but not to a worse one
    for k in (4, 9):  # one inserted base: the windows p0 and p0 + 1 tie; the start takes the first, the end the later one
        c = pat[:k] + sub(pat[k], [0], 2) + pat[k:]
        rs.append(one_read(mode, a, L, ad, copy=c, pos=a if mode == "start" else a + 1, mined=2, note="insertion at %d" % k))
        if mode == "end":  # ... and with the copy at the tail this is how a tail copy does trim: pos = 1
            rs.append(one_read(mode, 0, L, ad, copy=c, pos=1, mined=2, cmplen=17, note="insertion at %d, at the tail" % k))
    for i, r in enumerate(rs):
        r.note = r.note or "order %s %d" % (mode, i)
    return _one_sided("B-order-%s" % mode, mode, rs, ad)


# ---- C. thresholds ---------------------------------------------------------------------------------------------------------------------

def _first_exact(mode, ad, L, ed_max, ext, n, order, make, value, base=0):
    """k substitutions do not always cost k edits (a shifted alignment may be cheaper): add one substitution at a time, each at the
    first place of `order` at which value(model of the read) goes up by exactly one.  Deterministic; the search is part of the
    recipe, and what it settles on is promised and verified like any other recipe"""
    fill = filler_for(ad if mode == "start" else "", ad if mode == "end" else "", ed_max)
    places = []
    for i in range(n):
        for x in order:
            if x not in places and value(model_trim(bytes(make(places + [x]).build(fill)[0]), ad, mode, ed_max, ext, i + 1 < n)) == base + i + 1:
                places.append(x)
                break
        else:
            raise AssertionError("no place for substitution %d of %d (%s)" % (i + 1, n, make(places).note))
    return make(places)


def pattern_threshold_battery(mode, ed_max=0.25, L=300):
    """pattern copies whose best window is at exactly thrP and at exactly thrP + 1 edits: substitutions only, and mixes with one
    inserted or one deleted base (either costs two edits in a window of 16: the other is the base that leaves or enters at its end)"""
    ad = START if mode == "start" else END
    pat = pat_of(ad, mode)
    thrP = thr_at(ed_max, 16)
    ins = pat[:7] + sub(pat[7], [0], 2) + pat[7:]   # 17 bases
    dele = pat[:7] + pat[8:]                         # 15 bases
    rs = []
    for p0 in ((40, 150) if ed_max < 0.3 else ((3, 5) if mode == "start" else (2, 5))):  # (at 0.4 sixteen matching bases of 24 ARE a full match wherever the whole adapter fits)
        for name, c, n0 in (("substitutions", pat, 0), ("insertion", ins, 2), ("deletion", dele, 2)):
            for target in (thrP, thrP + 1):
                def make(places, c=c, target=target, name=name):
                    w = dict(found=True, mined=thrP, nearest=thrP) if target == thrP else dict(found=False, nearest=thrP + 1)
                    if name == "substitutions" and target == thrP:
                        w["pos"] = p0
                    return one_read(mode, p0, L, ad, copy=sub(c, places), note="%s: %d edits at %d" % (name, target, p0), **w)
                rs.append(_first_exact(mode, ad, L, ed_max, 10, target - n0, range(1, 15), make, lambda m: m.get("nearest"), n0))
    return _one_sided("C-pattern-%s-%g" % (mode, ed_max), mode, rs, ad, dict(ed_max=ed_max))


def confirm_battery(mode, adapter, ed_max=0.25, ext=10, L=260):
    """a truncated adapter of cmplen bases at the read's start / end, for every cmplen from 16 (17 at the end) to alen, at exactly
    thr[cmplen] and thr[cmplen] + 1 edits: substitutions in the flank as far as it reaches, the rest in the pattern (at most thrP
    there, so that the search still finds it).  cmplen = alen is reached with the threshold's edits only at the end, flush with the
    tail (elsewhere the full-match search has taken such a copy); at the start it is reached with one edit more"""
    alen = len(adapter)
    pat = pat_of(adapter, mode)
    thrP = thr_at(ed_max, 16)
    rs = []
    for cmplen in range(16 if mode == "start" else 17, alen + 1):
        f = cmplen - 16
        p0 = f if (cmplen < alen or mode == "end") else f + 5
        t = thr_at(ed_max, cmplen)
        own = adapter[alen - cmplen:alen - 16] if mode == "start" else adapter[16:cmplen]
        for k in (t, t + 1):
            if k - min(f, k) > thrP or (cmplen == alen and mode == "start" and k == t):
                continue
            # places 0 .. f - 1: the flank, nearest the pattern first; f ..: the pattern
            near = list(range(f - 1, -1, -1)) if mode == "start" else list(range(f))
            order = near + [f + x for x in (2, 6, 10, 13, 4, 8)]

            def make(places, k=k, t=t, cmplen=cmplen, p0=p0, f=f, own=own):
                fl = sub(own, [x for x in places if x < f], 2)
                return one_read(mode, p0, L, adapter, copy=sub(pat, [x - f for x in places if x >= f]), flank=fl or None, pos=p0,
                                cmplen=cmplen, ok=k <= t, ced=k, note="cmplen %d, %d edits (thr %d)" % (cmplen, k, t))
            rs.append(_first_exact(mode, adapter, L, ed_max, ext, k, order, make,
                                   lambda m, p0=p0: m.get("ced") if m["full"] is None and m["pos"] == p0 else None))  # (on the way the full-match search may find it)
    return _one_sided("C-confirm-%s-%d-%g-%d" % (mode, alen, ed_max, ext), mode, rs, adapter, dict(ed_max=ed_max, trimming_extension=ext))


# ---- D. what is left -------------------------------------------------------------------------------------------------------------------

def short_reads_battery(alen):
    """start: reads shorter than the adapter.  pos = min(pos + ext, rlen - alen) is negative; with alen = 24 something is left or
    the count is still positive, with 40 and 64 pos + 16 is negative too: the read is erased, and booked with 0 bases"""
    ad = START if alen == 24 else random_adapter(300 + alen, alen)
    rs = []
    for L in range(17, 24):
        p2 = min(0 + 10, L - alen)
        n = min(L - 1, p2 + 16)
        left = (L, L) if n < 0 else (n, L)
        rs.append(one_read("start", 0, L, ad, pos=0, mined=0, cmplen=16, ok=True, count=p2 + 16, key=16, left=left, note="alen %d, r1 of %d" % (alen, L)))
    return Battery("D-short-%d" % alen, rs, ad, "")


def leftover_battery():
    """end: pos + ext >= rlen - 16 leaves r1 with 0 bases; trims that leave exactly 1 base; both ends trimmed in one read"""
    rs = []
    for L, p0 in ((40, 20), (40, 14), (40, 13), (60, 33), (60, 34), (57, 30)):
        p2 = min(p0 + 10, L - 16)
        rs.append(one_read("end", p0, L, END, flank="own", count=p2 + 16, left=(0, L - 16 - p2), note="end, r1 of %d, p0 = %d" % (L, p0),
                           **(dict(full_any=True) if p0 > 8 else dict(pos=p0, ok=True))))
    for L, p0 in ((40, 14), (40, 13), (41, 14), (30, 5), (30, 6), (31, 4)):  # (trimFront takes at most rlen - 1)
        p2 = min(p0 + 10, L - 24)
        n = min(L - 1, p2 + (24 if p0 >= 8 else 16))
        rs.append(one_read("start", p0, L, START, flank="own", left=(n, L), note="start, r1 of %d, p0 = %d" % (L, p0),
                           **(dict(full=p0 - 8) if p0 >= 8 else dict(pos=p0, ok=True, count=p2 + 16))))
    # both ends: the start trim moves what the end search sees (the end pattern pe bases from the tail)
    for L, ps, pe in ((120, 3, 5), (120, 5, 1), (80, 2, 7), (64, 4, 3)):
        ns = min(ps + 10, L - 24) + 16
        left = L - ns
        p2 = min(pe + 10, left - 16)
        rs.append(Recipe(L, piece("start", START, ps, L, flank="own") + piece("end", END, pe, L, flank="own"),
                         start=dict(pos=ps, ok=True, count=ns, left=(ns, L)), end=dict(pos=pe, ok=True, count=p2 + 16),
                         r1=(ns, ns + left - 16 - p2), note="both ends, r1 of %d, %d / %d" % (L, ps, pe)))
    return Battery("D-left", rs, START, END)


# ---- E. candidates and the cap -----------------------------------------------------------------------------------------------------------

def cap_reads(mode, L=300):
    """-> [(recipe, columns a lane consumes; None where the recipe is not about them)]"""
    ad = START if mode == "start" else END
    pat = pat_of(ad, mode)
    one = sub(pat, S4)       # a copy with ONE candidate column
    out = []

    def put(pieces, cols, note, **w):
        both = [piece(mode, ad, p, L, c) for p, c in pieces]
        over = [o for pc_ in both for o in pc_[:-1]] + [pc_[-1] for pc_ in both]  # (the flanks first: no flank lies over a copy)
        r = Recipe(L, over, note=note)
        if cols is not None:
            w.update(cols=cols, over=cols > CAP)
        getattr(r, mode).update(w)
        out.append((r, cols))
    put([], 0, "no column", pos=-1)
    put([(40, one)], 1, "one column", pos=40, mined=4)
    if mode == "start":
        put([(40, pat)], 9, "nine", pos=40)
        put([(40, pat), (100, one)], 10, "ten: stays in the lane", pos=40)
        put([(100, pat), (40, one)], 10, "ten, the single one first", pos=100)
        put([(40, pat), (100, one), (140, one)], 11, "eleven: handed on", pos=40)
        put([(40, pat), (100, pat)], 18, "eighteen", pos=40)
        put([(40, sub(pat, S2)), (100, pat)], None, "the better one lies behind the cap", pos=100, mined=0, over=True)
        put([(40 + 16 * i, one) for i in range(9)], 9, "nine single ones", pos=40, mined=4)
        put([(8 + 16 * i, one) for i in range(11)], 11, "eleven single ones", pos=8, mined=4)
        # candidates only below column 15 (the pattern's last 12 bases open the read) and only at lim (a one-column copy flush with
        # the 200 bases, or with the end of a shorter r1): consumed, never tested, nothing found
        for r, c in ((Recipe(L, [(0, pat[4:])], start=dict(cols=1, pos=-1), note="a column below 15"), 1),
                     (Recipe(L, piece(mode, ad, 184, L, one), start=dict(cols=1, pos=-1), note="a column at lim"), 1),
                     (Recipe(100, piece(mode, ad, 84, 100, one), start=dict(cols=1, pos=-1), note="a column at lim, r1 of 100"), 1)):
            out.append((r, c))
    else:
        # the walk stops at the first increase: of a perfect copy's columns it consumes those up to the first window past the best
        put([(40, pat)], None, "one copy", pos=40, mined=0)
        put([(0, pat), (60, pat), (120, pat)], 2, "stops after 2 while many more remain", pos=0, mined=0)
        put([(40, one), (100, one)], 2, "two single ones: moves on to the equal one", pos=100, mined=4)
        for n in (9, 10, 11):  # n single-column copies, all equal: the walk never stops and consumes them all
            put([(4 + 16 * i, one) for i in range(n)], n, "%d equal single ones" % n, pos=4 + 16 * (n - 1), mined=4)
        out.append((Recipe(100, [(0, one)], end=dict(cols=1, pos=-1), note="a column at lim, r1 of 100"), 1))
        out.append((Recipe(L, [(L - 200, one)], end=dict(cols=1, pos=-1), note="a column at lim"), 1))
        out.append((Recipe(100, [(0, pat[4:])], end=dict(cols=1, pos=-1), note="a column below 15"), 1))
    return out


def cap_battery(mode):
    return _one_sided("E-cap-%s" % mode, mode, [r for r, _ in cap_reads(mode)], START if mode == "start" else END)


def wave_battery(mode, lane, n=64):
    """plain reads (no column) around one that goes beyond the cap at `lane` of every group of 64 the batch reaches into, and one
    that stays at the cap seven lanes on; n = 1 .. 129 reads"""
    reads = cap_reads(mode)
    over = [r for r, c in reads if c is not None and c > CAP][0]
    stay = [r for r, c in reads if c == CAP][0]
    plain = reads[0][0]
    rs = [over if i % 64 == lane else (stay if i % 64 == (lane + 7) % 64 else plain) for i in range(n)]
    return _one_sided("E-wave-%s-%d-%d" % (mode, lane, n), mode, rs, START if mode == "start" else END)


def fallback_battery(mode, L=300):
    """reads beyond the cap on which the WAVE search of k_trim_ends_batched decides the outcome: a wrong choice there trims (a worse
    window with the adapter's own bases beside it, where the confirmation passes) and the right one does not"""
    ad = START if mode == "start" else END
    pat = pat_of(ad, mode)
    one = sub(pat, S4)
    junk = pat[:4] + pat[5:9] + pat[10:13] + pat[14:]  # three bases lost: three candidate columns, and no window within thrP
    rs = []

    def put(pieces, note, **w):
        both = [piece(mode, ad, *x) for x in pieces]
        r = Recipe(L, [o for b in both for o in b[:-1]] + [b[-1] for b in both], note=note)
        getattr(r, mode).update(w, over=True)
        rs.append(r)
    if mode == "start":
        # the smallest distance wins, not the smallest position: the worse copy at 3 would trim
        put([(3, L, sub(pat, S2), "own"), (60, L, pat), (120, L, pat)], "a worse copy that would trim, in front of two perfect ones", pos=60, mined=0, ok=False, count=0)
        put([(3, L, sub(pat, S2), "own"), (60, L, junk), (92, L, junk), (120, L, junk)], "a copy that trims, and columns without a window", pos=3, mined=2, ok=True)
    else:
        # a later equal one wins: the first of eleven equal ones would trim
        put([(4, L, one, "own")] + [(4 + 16 * i, L, one) for i in range(1, 11)], "eleven equal ones, the first would trim", pos=164, mined=4, ok=False, count=0, cols=11)
        # pos > 0 is strict: a tail copy at 0 behind twelve columns without a window is chosen and not trimmed
        put([(0, L, one)] + [(32 * i, L, junk) for i in range(1, 5)], "a tail copy at 0 beyond the cap", pos=0, mined=4, count=0, cols=13)
        put([(1, L, one, "own")] + [(32 * i, L, junk) for i in range(1, 5)], "a tail copy at 1 beyond the cap", pos=1, mined=4, ok=True, cols=13)
    return _one_sided("E-fallback-%s" % mode, mode, rs, ad)


def beyond_battery(mode):
    """a short r1 whose one-column copy ends one base BEYOND it, in the bases trim_tail takes, beside a longer read that keeps the
    column loop running: a column past the text's end is no candidate (no search runs: the batch has no column at all)"""
    ad = START if mode == "start" else END
    one = sub(pat_of(ad, mode), S4)
    L = 100
    rs = [Recipe(L, [(L - 15, one)], note="a copy that ends one base beyond r1"), Recipe(300, [], note="plain")]
    getattr(rs[0], mode).update(cols=0, pos=-1)
    return _one_sided("E-beyond-%s" % mode, mode, rs, ad, dict(trim_tail=3))


def hint_battery(L=40):
    """no command-line adapter and a FASTA list: k_trim_ends<2> searches the positions its filter's verdict leaves open, and in ONE
    round when they span fewer than 64.  The verdict is kept per block of 32 columns, so with r1 of 40 bases the last position of
    the range is 7: a one-column copy of an entry's pattern exactly there, as the end of a truncated entry (it trims), one place
    to either side, and plain reads"""
    rs = []
    for i, ad in enumerate(FASTA):
        for mode in ("start", "end"):
            one = sub(pat_of(ad, mode), S4)
            for p0 in (6, 7, 8):
                r = Recipe(L, piece(mode, ad, p0, L, one, "own"), note="entry %d, %s, p0 = %d" % (i, mode, p0))
                if p0 < len(ad) - 16:  # (from there on the whole entry stands in the read: the full-match search may take it)
                    r.chain[(i, mode)] = dict(pos=p0, mined=4, ok=True, cmplen=p0 + 16)
                rs.append(r)
    rs += [Recipe(L, [], note="plain"), Recipe(300, [], note="plain, 300")]
    return Battery("H-hint", rs, "", "", None, FASTA)


# ---- F. confirmations, every form -----------------------------------------------------------------------------------------------------------

F_LENGTHS32 = [16, 17, 23, 24, 31, 32]
F_LENGTHS64 = [33, 40, 48, 63, 64]
F_LENGTHS0 = [8, 12, 15, 70]


def adapter_of(alen, with_n=False):
    a = random_adapter(500 + alen, max(alen, 16))[:alen]
    return a[:9] + "N" + a[10:] if with_n else a


def _layouts(ad, thr):
    """the adapter with thr edits in its first columns, thr in its last, thr + 1 of each, and thr - 2 substitutions plus one deleted
    and plus one inserted base -> [(name, text)]"""
    n = len(ad)
    out = [("first", sub(ad, range(thr), 2)), ("last", sub(ad, range(n - thr, n), 2)),
           ("first+1", sub(ad, range(thr + 1), 2)), ("last+1", sub(ad, range(n - thr - 1, n), 2))]
    if thr >= 2:  # (in a window of alen bases either costs two edits: the other is the base that enters or leaves at its end)
        d = n // 2
        out.append(("deletion", sub(ad[:d] + ad[d + 1:], range(thr - 2), 2)))
        out.append(("insertion", sub(ad[:d] + anti(ad[d]) + ad[d:n - 1], range(thr - 2), 2)))
    return out


def forms_battery(mode, alen, with_n=False, L=300):
    """the full-adapter candidate of the window scan with all thr edits in its first columns (every early-exit bound holds with
    equality), all in its last, one more of each, and an indel; truncated adapters for the partial confirmation; the batch's last
    read ENDS with a copy, so that the 16-byte loads of the confirmation cross the end of the buffer.  What the window scan makes of
    the full copies is the model's to say (full_any)"""
    ad = adapter_of(alen, with_n)
    thr = thr_at(0.25, alen)
    plen = min(16, alen)
    rs = []
    for name, c in _layouts(ad, thr):
        for p in (20, 190 - alen):
            r = Recipe(L, [(p if mode == "start" else L - 200 + p, c)], note="%s at %d" % (name, p))
            getattr(r, mode)["full_any"] = True
            rs.append(r)
    for p0 in sorted({1, 2, max(1, alen - plen - 1), alen - plen, 100, 183}):
        rs.append(one_read(mode, p0, L, ad, flank="own", full_any=True, note="truncated, p0 = %d" % p0))
    if alen < 16:  # up to 200 - plen positions: the round beyond 192
        for p0 in (191, 192, 199 - plen):
            rs.append(one_read(mode, p0, L, ad, full_any=True, note="p0 = %d" % p0))
    tail = sub(ad, range(thr), 2)
    r = Recipe(L, [(L - len(tail), tail)], note="the buffer ends with the copy")
    getattr(r, mode)["full_any"] = True
    rs.append(r)
    return _one_sided("F-forms-%s-%d%s" % (mode, alen, "N" if with_n else ""), mode, rs, ad)


# ---- G. the confirmations of k_resolve ------------------------------------------------------------------------------------------------------

def model_middle(r1, start, end, ed_max, ext):
    """findMiddleAdapters on r1 (bytes) -> dict: per adapter (keys sp / ep) the strict-`<` first minimum of the Hamming profile
    (scan_cases.profile: every window start p < len - alen), whether it needs its edit distance (it is beyond the threshold), that
    distance, and the position when it stands; frags = the pieces breakByGap leaves, [(start, length)]"""
    a = np.frombuffer(bytes(r1), np.uint8)
    n = len(a)
    out = {}
    for key, ad in (("sp", start), ("ep", end)):
        adb = np.frombuffer(ad.encode(), np.uint8)
        mm = sc.profile(a, adb)
        out[key] = None
        if len(mm) == 0:
            continue
        p, thr = int(np.argmin(mm)), thr_at(ed_max, len(ad))
        need = int(mm[p]) > thr
        ed = tsc.edit_distance(bytes(a[p:p + len(ad)]), bytes(adb)) if need else int(mm[p])
        out.update({key + "_at": p, key + "_need": need, key + "_ed": ed, key + "_ham": int(mm[p]), key: p if ed <= thr else None})
    hits = [(out[k], len(ad)) for k, ad in (("sp", start), ("ep", end)) if out[k] is not None]
    out["split"] = bool(hits)
    if hits:
        gs, ge = max(0, min(p for p, _ in hits) - ext), min(n, max(p + l for p, l in hits) + ext)
        out["frags"] = [(x, y) for x, y in ((0, gs), (ge, n - ge)) if y > 0]
    else:
        out["frags"] = [(0, n)]
    return out


class MiddleBattery(Battery):
    """reads the end trims leave whole, with copies in the middle: verify asserts that the model gives every promise, that the
    oracle's find_middle gives what the model gives, and that the oracle's batch record holds the model's pieces"""

    def verify(self, orc):
        res, cnt = orc.process_batch(self.config(orc), self.seq, self.qual, self.off, max_cycles=self.C)
        self.mids = []
        for i, (r, (s, _)) in enumerate(zip(self.recipes, self.reads)):
            tag = (self.name, i, r.note)
            assert not res["dropped"][i] and (int(res["r1_start"][i]), int(res["r1_len"][i])) == (0, r.L), (tag, "an end trim touched the read")
            m = model_middle(bytes(s), self.start, self.end, self.ed_max, self.ext)
            self.mids.append(m)
            for k, v in r.mid.items():
                assert m.get(k) == v, (tag, k, m.get(k), v)
            found, st, ln = orc.find_middle(bytes(s), self.start, self.end, self.ed_max, self.ext)
            gap = [(0, st), (st + ln, r.L - st - ln)] if found else [(0, r.L)]
            assert found == m["split"] and [f for f in gap if f[1] > 0] == m["frags"], (tag, found, st, ln, m)
            got = [(int(res["frag_start"][i, f]), int(res["frag_len"][i, f])) for f in range(int(res["n_frag"][i]))]
            assert got == m["frags"], (tag, got, m["frags"])
        return res, cnt

    def pick(self, idx, name):
        return MiddleBattery("%s-%s" % (self.name, name), [self.recipes[i] for i in idx], self.start, self.end, self.opt)


def _edits_early(ad, thr, extra=0):
    """a window of alen bases at exactly thr + extra edits from the adapter, ALL of them in its first columns and the rest a plain
    match, so that every early-exit bound `score - (columns left) <= thr` holds with equality from there on -- and with more than thr
    mismatches place by place, so that the confirmation runs: base 1 is lost, a base enters at k (the bases between stand one place
    early), and the first bases are substituted.  Yields one such window per k for which the numbers hold"""
    n = len(ad)
    want = thr + extra
    for k in range(4, n - 2):
        w = ad[0] + ad[2:k] + anti(ad[k]) + ad[k:]
        assert len(w) == n
        places = []
        for x in range(0, k - 1):  # (substitutions among the first k - 1 bases of the window)
            if len(places) == want - 2:
                break
            t = sub(w, places + [x], 2)
            if tsc.edit_distance(t.encode(), ad.encode()) == 2 + len(places) + 1:
                places.append(x)
        w = sub(w, places, 2)
        if len(places) == want - 2 and tsc.edit_distance(w.encode(), ad.encode()) == want and sum(a != b for a, b in zip(w, ad)) > thr:
            yield w


def _edits_late(ad, thr, extra=0):
    """... and with all of them in its LAST columns: a base lost near the end, the last base entering, substitutions in between"""
    n = len(ad)
    want = thr + extra
    for d in range(n - want - 2, 2, -1):
        w = ad[:d] + ad[d + 1:] + anti(ad[-1])
        places = []
        for x in range(n - 2, d, -1):
            if len(places) == want - 2:
                break
            t = sub(w, places + [x], 2)
            if tsc.edit_distance(t.encode(), ad.encode()) == 2 + len(places) + 1:
                places.append(x)
        w = sub(w, places, 2)
        if len(places) == want - 2 and tsc.edit_distance(w.encode(), ad.encode()) == want and sum(a != b for a, b in zip(w, ad)) > thr:
            yield w


G_PAIRS = {16: None, 24: (START, END), 31: None, 32: None, 33: None, 40: None, 63: None, 64: None,
           "N": (sc.N_ADAPTER, END), 70: (sc.LONG_ADAPTER, random_adapter(71, 40))}


def g_adapters(which):
    if G_PAIRS[which] is not None:
        return G_PAIRS[which]
    k = 1000 if which == 16 else 0  # (with the pair of seeds 616 / 716 no window of 16 bases holds five edits in its first columns)
    return random_adapter(600 + which + k, which), random_adapter(700 + which + k, which)


def _mid_read(L, pieces, note, **mid):
    return Recipe(L, pieces, mid=mid, note=note)


def _placed(start, end, key, L, p, windows, want, note, odd=None, **mid):
    """the first of `windows` that, laid at p of a read of L bases, IS the adapter's first Hamming minimum there, beyond the threshold
    place by place and at exactly `want` edits (a shifted neighbour may undercut a layout: the next one is tried.  Deterministic; the
    choice is promised and verified like any other recipe).  odd: a change made to the window before it is laid"""
    fill = filler_for(start, end, 0.25, 2200 if L > 700 else 720)
    for w in windows:
        r = _mid_read(L, [(p, odd(w) if odd else w)], note, **dict({key + "_at": p, key + "_need": True, key + "_ed": want}, **mid))
        m = model_middle(bytes(r.build(fill)[0]), start, end, 0.25, 10)
        if m.get(key + "_at") == p and m[key + "_need"] and m[key + "_ed"] == want:
            return r
    raise AssertionError("no layout holds at %d: %s" % (p, note))


def resolve_battery(which):
    """one middle copy per read, 600 bases (and 2100, the copy across byte 1984): the adapter at exactly thr edits (split) and thr + 1
    (not split), all in the first columns, all in the last, as substitutions only (at thr the Hamming count stands and nothing is
    confirmed); an N and a lower-case base of the RIGHT letter inside a window at thr + 1 (taken for matches they would make it
    thr); both adapters confirmed in one read; plain reads, whose best windows are hopeless"""
    start, end = g_adapters(which)
    rs = []
    for key, ad, at in (("sp", start, 300), ("ep", end, 260)):
        thr = thr_at(0.25, len(ad))
        for name, make in (("early", _edits_early), ("late", _edits_late)):
            for extra in (0, 1):
                # (the copy across byte 1984 is the start adapter's: the end adapter's would lie in the 200 bases of the end trim)
                for L, p in ((600, at), (2100, sc.TILE - len(ad) // 2))[:2 if key == "sp" else 1]:
                    rs.append(_placed(start, end, key, L, p, make(ad, thr, extra), thr + extra, "%s %s thr+%d at %d" % (key, name, extra, p),
                                      **{key: None if extra else p, "split": not extra}))
        rs.append(_mid_read(600, [(at, sub(ad, [i for i in range(len(ad)) if ad[i] != "N"][:thr], 2))], "%s %d substitutions" % (key, thr),
                            **{key: at, key + "_need": False, "split": True}))
        # an N and a lower-case base of the right letter in a window at thr: two edits more (taken for matches: within the threshold)
        j = len(ad) - 2

        def odd(w, j=j):
            return w[:j - 3] + "N" + w[j - 2:j] + w[j].lower() + w[j + 1:]
        rs.append(_placed(start, end, key, 600, at, _edits_early(ad, thr, 0), thr + 2, "%s N and lower case" % key, odd, **{key: None, "split": False}))
    # both adapters in one read, each at exactly its threshold
    both = _placed(start, end, "sp", 900, 300, _edits_early(start, thr_at(0.25, len(start))), thr_at(0.25, len(start)), "both adapters")
    ep = _placed(start, end, "ep", 900, 520, _edits_late(end, thr_at(0.25, len(end))), thr_at(0.25, len(end)), "both adapters")
    rs.append(_mid_read(900, both.over + ep.over, "both adapters", sp=300, ep=520, sp_need=True, ep_need=True, split=True))
    rs += [_mid_read(600, [], "plain", split=False, sp_need=True, ep_need=True), _mid_read(601, [], "plain", split=False)]
    return MiddleBattery("G-%s" % which, rs, start, end)


def resolve_wave_battery(lane, n=64):
    """63 plain reads, whose windows are hopeless, around one whose confirmation passes with equality, at `lane`: the ballot keeps the
    loop alive for that lane alone"""
    start, end = START, END
    one = _placed(start, end, "sp", 600, 300, _edits_early(start, 6), 6, "passes with equality", sp=300, split=True)
    plain = _mid_read(600, [], "plain", split=False, sp_need=True, ep_need=True)
    return MiddleBattery("G-wave-%d-%d" % (lane, n), [one if i % 64 == lane else plain for i in range(n)], start, end)


FASTA = ["TTGACCAGTAGGCATCAGGATCCA","GGTCATTCAGGCTAAGCTTCGGAATCCGTTAGCA"]  # the two-entry list behind batteries A, B and E
