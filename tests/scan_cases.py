"""Test helpers shared by tests/test_scan_emu.py and tests/test_gpu_scan.py: reads built so that the middle-adapter scan's
match COUNT decides the outcome (k_scan: range_scan_fast / range_scan_bytes in fastplong_amd/csrc/kernels.h).  No kernel code is
imported here.

A DUEL is one read: random ACGT flanks, a copy A of an adapter with k substitutions of adapter letter X by byte Y, and a copy B
with k - 1 ordinary substitutions (another of A, C, G, T).  Compared as raw bytes B has fewer mismatches, so a correct scan finds
B; a scan that takes Y for X finds A.  A TIE holds two copies with equally many ordinary substitutions: the first must win.

Every duel is checked on the CPU before any kernel sees it (Battery.verify): the Hamming profile of the read's r1 range -- one
mismatch count per window start p in [0, len - alen), raw bytes, a plain numpy loop over the adapter's letters -- has its
strict-`<` first minimum (findMiddleAdapters / searchAdapter of the reference, src/adaptertrimmer.cpp:133-151) where the duel
expects it, that minimum is unique (ties: held by exactly the two copies), and the oracle's record splits the read there.  A duel
whose random flanks break one of these is built again from its next seed; at most 5 % of a battery's duels may need that
(asserted), so a battery can never thin out silently."""
import numpy as np

from fastplong_amd import abi, synth

START, END = synth.START_ADAPTER, synth.END_ADAPTER
N_ADAPTER = "AAGGATTCATTCCNACGGTAACAC"  # a byte outside ACGT: k_scan takes range_scan_bytes / hamming16
TILE = 1984   # bytes of r1 a tile of the bit-sliced scan advances by (62 lanes of SC_CHUNK = 32 bytes)
CHUNK = 32
FLANK = 260   # beyond the 200-base windows of the end trims
REGEN_CAP = 0.05
GAPS = (100, 700, 2500)


def random_adapter(seed, n):
    """n random bases, every letter at least three times (n >= 16)"""
    rng = np.random.default_rng(seed)
    while True:
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, n))
        if min(s.count(c) for c in "ACGT") >= 3:
            return s


LONG_ADAPTER = random_adapter(70, 70)  # beyond 64 bases: the byte-wise scan as well


def y_bytes(x):
    """the bytes a duel puts in place of adapter letter x"""
    return ["N", "n", x.lower(), "U"] + list("RYKMSWBDHV") + ["*", "-"]


def xy_pairs():
    return [(x, y) for x in "ACGT" for y in y_bytes(x)]


def profile(r1, ad):
    """mismatches of the adapter at every tested window start of r1 (p < len - alen, as the reference's loop)"""
    n = len(r1) - len(ad)
    if n <= 0:
        return np.zeros(0, np.int64)
    mm = np.zeros(n, np.int64)
    for i in range(len(ad)):
        mm += r1[i:i + n] != ad[i]
    return mm


def _copy_xy(rng, ad, k, x, y):
    c = ad.copy()
    where = np.nonzero(ad == ord(x))[0]
    assert len(where) >= k, (x, k)
    c[rng.choice(where, k, replace=False)] = ord(y)
    return c


def _copy_sub(rng, ad, k):
    c = ad.copy()
    where = np.nonzero(np.isin(ad, synth._ACGT))[0]
    for p in rng.choice(where, k, replace=False):
        c[p] = rng.choice(synth._ACGT[synth._ACGT != ad[p]])
    return c


PAIR_MIN_LANES = 12  # (FPL_PAIR_MIN_LANES: a head takes the free lanes of a last tile when at least that many are)
PAD = 100            # a read too short to be hosted, or to host anything shorter than a tile


def heads(lens, chunk):
    """bytes of each read's r1 that ride as a head in its predecessor's last tile (0: none) when a k_scan wave takes `chunk` reads
    per dequeue -- the kernel's rules replayed for reads the end trims leave whole: chunks start at multiples of `chunk`, only a
    read with a next one in ITS chunk hosts, its own tiles start where its own head ended, its last tile needs la lanes and hosts
    when 62 - la >= 12 are free and the next read has 32 * (64 - la) + 64 bytes"""
    h = [0] * len(lens)
    if chunk < 2:
        return h
    for i in range(len(lens) - 1):
        if (i + 1) % chunk == 0 or lens[i] <= h[i]:
            continue
        t0 = h[i]
        while t0 + TILE < lens[i]:
            t0 += TILE
        la = (lens[i] - t0 + CHUNK - 1) // CHUNK
        if 62 - la >= PAIR_MIN_LANES and lens[i + 1] >= CHUNK * (64 - la) + 64:
            h[i + 1] = CHUNK * (62 - la)
    return h


def builtin_chunk(n, n_cu, waves_per_block):
    """reads per dequeue that the library's own rule gives a batch of n reads when FPL_SCAN_CHUNK is not set (the k_scan launch in
    fastplong_amd/csrc/pipeline.h; waves_per_block: KWAVES, 4 on the device and 2 in the emulator build): 1 -- no read has a next
    one -- only while the batch has fewer than two reads per wave of the grid"""
    waves = min((n + waves_per_block - 1) // waves_per_block, 5 * n_cu) * waves_per_block
    chunk = n // (waves * 32)
    if chunk < 4:
        chunk = 4 if n >= 8 * waves else (2 if n >= 2 * waves else 1)
    return min(chunk, 64)


# where a copy of alen bases at position p lies to the end of a head of h bytes
HEAD_PLACES = {
    "inside": lambda p, alen, h: p + alen < h,
    "ends at": lambda p, alen, h: p + alen == h,
    "across": lambda p, alen, h: p < h < p + alen,
    "at": lambda p, alen, h: p == h,
    "behind": lambda p, alen, h: p == h + 1,
    "own tiles": lambda p, alen, h: p > h + 1,
}


class Duel:
    """a recipe: L bases, copy A at a_pos (None: no A) with k substitutions X -> Y (x None: ordinary ones), copy B at b_pos with
    kb ordinary ones (cut off where it reaches past the read), a third copy C at c_pos with k ordinary ones, odd bytes planted at
    `plants`.  expect: 'a' / 'b' -- the copy the scan must find -- or None: no window within the edit-distance limit, the read stays
    in one piece.  tie: the minimum is held by both copies.  Geometry the battery promises under its FPL_SCAN_CHUNK (checked by
    Battery.check_geometry against heads()): head -- the bytes of this read that ride in its predecessor's last tile; where -- how
    the copy named by `which` lies to the end of that head (HEAD_PLACES); edge -- the first boundary between two of the read's
    own tiles, which copy `which` must lie across"""

    def __init__(self, ad, L, a_pos, b_pos, k, x=None, y=None, kb=None, plants=(), expect="b", tie=False, c_pos=None, note="",
                 head=None, where=None, which="b", edge=None):
        self.ad, self.L, self.a_pos, self.b_pos, self.k, self.x, self.y = ad, L, a_pos, b_pos, k, x, y
        self.kb = k - 1 if kb is None else kb
        self.plants, self.expect, self.tie, self.c_pos, self.note = plants, expect, tie, c_pos, note
        self.head, self.where, self.which, self.edge = head, where, which, edge

    def build(self, seed, adapters):
        rng = np.random.default_rng(seed)
        ad = np.frombuffer(adapters[self.ad].encode(), np.uint8)
        s = synth._ACGT[rng.integers(0, 4, self.L)].astype(np.uint8)
        if self.a_pos is not None:
            a = _copy_xy(rng, ad, self.k, self.x, self.y) if self.x else _copy_sub(rng, ad, self.k)
            s[self.a_pos:self.a_pos + len(ad)] = a
        if self.b_pos is not None:
            b = _copy_sub(rng, ad, self.kb)[:self.L - self.b_pos]
            s[self.b_pos:self.b_pos + len(b)] = b
        for p, byte in self.plants:
            s[p] = ord(byte)
        q = rng.integers(33 + 8, 33 + 42, self.L).astype(np.uint8)  # ('5' and '?', the Q20 / Q30 limits, among them)
        if self.c_pos is not None:
            s[self.c_pos:self.c_pos + len(ad)] = _copy_sub(rng, ad, self.k)
        return s, q

    def want_pos(self):
        return {"a": self.a_pos, "b": self.b_pos, None: None}[self.expect]


class Filler:
    """a read that is no duel (the predecessor whose last tile hosts a duel's head): random bases"""

    def __init__(self, L):
        self.L = L

    def build(self, seed, adapters):
        rng = np.random.default_rng(seed)
        return synth._ACGT[rng.integers(0, 4, self.L)].astype(np.uint8), rng.integers(33 + 8, 33 + 42, self.L).astype(np.uint8)


class Battery:
    def __init__(self, name, recipes, start=START, end=END, opt=None, seed=1, chunk=0):
        self.chunk = chunk  # the FPL_SCAN_CHUNK the battery's geometry is laid out for (0: the hook cleared, no read has a next one)
        self.name, self.recipes, self.start, self.end, self.opt = name, recipes, start, end, dict(opt or {})
        self.cfgd = dict(opt=self.opt, start=start, end=end)
        self.adapters = (start, end)
        self.seeds = [seed * 100003 + i for i in range(len(recipes))]
        self.duels = [i for i, r in enumerate(recipes) if isinstance(r, Duel)]
        self.regenerated = 0
        self._pack()

    def _pack(self):
        self.seq, self.qual, self.off = synth.pack([r.build(s, self.adapters) for r, s in zip(self.recipes, self.seeds)])
        self.C = int(np.diff(self.off.astype(np.int64)).max()) + 1

    def check_geometry(self, res=None):
        """the heads and tile boundaries the recipes promise are the ones k_scan's rules give these reads under self.chunk"""
        hs = heads([r.L for r in self.recipes], self.chunk)
        if res is not None and any(hs):  # (the rules replayed in heads() are those for reads the end trims leave whole)
            assert not res["dropped"].any() and (res["r1_start"] == 0).all() and \
                (res["r1_len"] == np.diff(self.off.astype(np.int64))).all()
        for i in self.duels:
            d = self.recipes[i]
            alen = len(self.adapters[d.ad])
            p = d.a_pos if d.which == "a" else d.b_pos
            if d.head is not None:
                assert hs[i] == d.head and d.head > 0, (self.name, self.chunk, i, d.note, hs[i], d.head)
                assert HEAD_PLACES[d.where](p, alen, d.head), (self.name, i, d.where, p, d.head)
            if d.edge is not None:
                assert hs[i] + TILE == d.edge and p <= d.edge <= p + alen, (self.name, self.chunk, i, hs[i], d.edge, p)
        return hs

    def config(self, orc):
        return orc.Config(abi.FplOptions.default(**self.opt), self.start, self.end)

    def _problem(self, i, res):
        """None when duel i holds what it promises, else what is wrong with it"""
        d = self.recipes[i]
        ext = self.opt.get("trimming_extension", 10)
        o = int(self.off[i])
        s, n = int(res["r1_start"][i]), int(res["r1_len"][i])
        if res["dropped"][i] or (s, n) != (0, d.L):
            return "an end trim touched the read"
        ad = np.frombuffer(self.adapters[d.ad].encode(), np.uint8)
        mm = profile(self.seq[o:o + n], ad)
        want = d.want_pos()
        if want is None:
            return None if res["n_frag"][i] == 1 and res["frag_len"][i, 0] == n else "the oracle splits the read"
        if int(np.argmin(mm)) != want:
            return "the profile's first minimum is at %d, not %d" % (int(np.argmin(mm)), want)
        holders = np.nonzero(mm == mm.min())[0].tolist()
        if holders != ([d.a_pos, d.b_pos] if d.tie else [want]):
            return "the minimum is held at %s" % holders
        gs, ge = max(0, want - ext), min(n, want + len(ad) + ext)
        frags = [(a, b) for a, b in ((0, gs), (ge, n - ge)) if b > 0]
        got = [(int(res["frag_start"][i, f]), int(res["frag_len"][i, f])) for f in range(int(res["n_frag"][i]))]
        return None if got == frags else "the oracle's fragments are %s, not %s" % (got, frags)

    def verify(self, orc):
        """the CPU-side assertions on every duel; rebuilds the few whose flanks got in the way.  -> (want_res, want_cnt)"""
        cfg = self.config(orc)
        for attempt in range(6):
            res, cnt = orc.process_batch(cfg, self.seq, self.qual, self.off, max_cycles=self.C)
            bad = [(i, p) for i in self.duels for p in [self._problem(i, res)] if p]
            if not bad:
                self.check_geometry(res)
                assert self.regenerated <= REGEN_CAP * len(self.duels), (self.name, self.regenerated, len(self.duels))
                return res, cnt
            assert attempt < 5, (self.name, bad[:5])
            for i, _ in bad:
                if self.seeds[i] < 1 << 40:
                    self.regenerated += 1
                self.seeds[i] += 1 << 40
            self._pack()


def assert_duels_split(b, res):
    """the battery did what it is for: every duel that expects a copy to win is split there (Battery.verify checked where)"""
    won = [i for i in b.duels if b.recipes[i].expect is not None]
    inner = [i for i in won if b.recipes[i].want_pos() + len(b.adapters[b.recipes[i].ad]) + 10 < b.recipes[i].L]
    assert len(won) > 0 and (res["n_frag"][inner] == 2).all() and (res["n_frag"][won] >= 1).all()


_verified = {}


def verified(orc, key, make):
    """a battery and the oracle's results for it, built and checked once per session"""
    if key not in _verified:
        b = make()
        _verified[key] = (b,) + b.verify(orc)
    return _verified[key]


# ---- the batteries ---------------------------------------------------------------------------------------------------------------

def _ad_with(adapters, x, k, prefer):
    """the adapter (index) to duel with: `prefer` when it holds k letters x outside N"""
    return prefer if adapters[prefer].count(x) >= k else 1 - prefer


def bytes_battery(start=START, end=END, plant=False, ks=(1, 2, 3), orders=(0, 1)):
    """every (X, Y), k = 1, 2, 3, A before B and B before A; the three gaps are dealt in turn, ONE per duel (384 reads, not 1152).  plant: a lower-case base 40 bases in front of A
    and one 40 bases behind it -- whichever way the tiles fall (a read whose head rode in its predecessor's last tile starts its
    own tiles further in), one of the two lies in the 2048 bytes the tile of A's first base loads, so that tile builds its planes
    with the validity test (build_planes) instead of the three code planes"""
    adapters = (start, end)
    recipes = []
    for i, (x, y) in enumerate(xy_pairs()):
        for k in ks:
            for order in orders:
                ad = _ad_with(adapters, x, k, (i + k) % 2)
                alen = len(adapters[ad])
                gap = GAPS[(i + k + order) % 3]
                lead = FLANK + (7 * i + 3 * k) % 64
                first, second = lead, lead + alen + gap
                a_pos, b_pos = (first, second) if order == 0 else (second, first)
                L = second + alen + FLANK + (5 * i) % 50
                plants = ((a_pos - 40, "acgt"[i % 4]), (a_pos + alen + 40, "acgt"[(i + 1) % 4])) if plant else ()
                recipes.append(Duel(ad, L, a_pos, b_pos, k, x, y, plants=plants))
    return Battery("bytes", recipes, start, end, seed=11 + plant)


def head_bytes(rem):
    """bytes of the next read's r1 that ride in the last tile of a read whose last tile holds rem bytes (0: no head)"""
    la = (rem + CHUNK - 1) // CHUNK
    return CHUNK * (62 - la) if 62 - la >= 12 else 0


def _finish(name, protos, chunk, seed, start=START, end=END):
    """protos: (length, make(own_start) -> recipe) per read; own_start = the head the read gets under `chunk` (heads())"""
    hs = heads([L for L, _ in protos], chunk)
    b = Battery(name, [make(h) for (_, make), h in zip(protos, hs)], start, end, seed=seed, chunk=chunk)
    assert [r.L for r in b.recipes] == [L for L, _ in protos]
    b.check_geometry()
    return b


def _add_hosted(protos, chunk, host_len, L, make):
    """a Filler of host_len bases at the start of a dequeue chunk (so its own tiles start at 0) and the read make(head) behind it"""
    while chunk > 1 and len(protos) % chunk:
        protos.append((PAD, lambda h: Filler(PAD)))
    protos.append((host_len, lambda h: Filler(host_len)))
    protos.append((L, make))


def places_battery(chunk):
    """where B lies, laid out for FPL_SCAN_CHUNK = chunk (0: the hook cleared): every residue of the lane chunk; across the first
    boundary between two of the read's own tiles (at 1984 behind whatever head the read got: heads()); the last window the
    reference tests and one base further (not tested: A wins, or nothing); and, for chunk > 1, inside / up to / across the end of
    / right behind a head of 1952, 1664, 960 and 384 bytes that rides in the last tile of a predecessor placed at the start of a
    dequeue chunk (for chunk 0 the same reads, none hosted).  Battery.check_geometry asserts the heads and boundaries.  The reads
    of the last-window cases end where they end whatever head they got: their lengths modulo the tile are exact in the chunk 0
    battery only"""
    alen = len(START)
    protos = []
    xy = [("G", "N"), ("C", "c"), ("A", "N"), ("T", "U")]

    def duel(L, a_pos, b_pos, j, **kw):
        x, y = xy[j % 4]
        return Duel(0, L, a_pos, b_pos, 2, x, y, **kw)

    for r in range(CHUNK):  # residues (a head is a whole number of chunks: the residue holds whatever the read's own start)
        protos.append((1500, lambda h, r=r: duel(1500, 300 if r % 2 else 1100, 640 + r, r)))
    for j in range(alen + 1):  # across the boundary between the first two of the read's own tiles
        protos.append((4700, lambda h, j=j: duel(4700, 400 if j % 2 else h + TILE + 366, h + TILE - alen + j, j, edge=h + TILE)))
    for j, L in enumerate([700, 701, 733, TILE + 5, TILE + alen + 1, TILE + alen + 2, 2048, 2 * TILE - 3, 2 * TILE + 1]):
        protos.append((L, lambda h, j=j, L=L: duel(L, 300, L - alen - 1, j, note="last window")))
        protos.append((L, lambda h, j=j, L=L: duel(L, 300, L - alen, j, expect="a", note="whole but not tested")))
        protos.append((L, lambda h, j=j, L=L: duel(L, 300, L - alen + 1, j, expect="a", note="cut off")))
        protos.append((L, lambda h, j=j, L=L: duel(L, None, L - alen, j, expect=None, note="not tested, no A")))
    j = 0
    for rem in (1, 320, 1000, 1599):  # heads of 1952, 1664, 960, 384 bytes
        hb = head_bytes(rem)
        for b, where in ((FLANK + 20, "inside"), (hb - alen - 1, "inside"), (hb - alen, "ends at"), (hb - alen // 2, "across"),
                         (hb - 1, "across"), (hb, "at"), (hb + 1, "behind")):
            a = hb + 300 if where == "inside" else FLANK + 20  # (B inside the head: A in the read's own tiles, and the other way round)
            kw = dict(head=hb, where=where) if chunk > 1 else {}
            _add_hosted(protos, chunk, rem + (TILE if j % 3 == 0 else 0), hb + 900,
                        lambda h, a=a, b=b, j=j, kw=kw, hb=hb, where=where: duel(
                            hb + 900, a, b, j, note="B %s a head of %d bytes" % (where, hb), **kw))
            j += 1
    return _finish("places", protos, chunk, 21)


def ties_battery(start=START, end=END, chunk=0):
    """two copies with equally many ordinary substitutions, the first wins: in one lane's chunk, in two lanes of a tile, in the
    same lane of two tiles (both scans: 1984 / 1024 bytes apart), in two tiles, and -- chunk > 1, two adapters of <= 32 bases:
    the instance that packs pairs -- the first inside a head and the second in the read's own tiles, or the first up against the
    end of the head and the second right at it (Battery.check_geometry asserts the heads)"""
    adapters = (start, end)
    protos = []
    j = 0
    for ad in (0, 1):
        alen = len(adapters[ad])
        for k in (0, 1, 2):
            for dist in (alen + 1, alen + 76, 1024, TILE, TILE + 16, 2 * TILE + 40):
                first = 288 if dist == alen + 1 else 288 + 5 * j % 32  # (288 = 9 chunks: copies alen + 1 apart share a chunk when alen < 31)
                L = first + dist + alen + FLANK + j % 9
                protos.append((L, lambda h, ad=ad, L=L, first=first, dist=dist, k=k:
                               Duel(ad, L, first, first + dist, k, kb=k, expect="a", tie=True)))
                j += 1
    alen = len(adapters[0])
    if max(len(start), len(end)) <= 32:
        for rem in (320, 1000):
            hb = head_bytes(rem)
            for k in (0, 2):
                # (check_geometry looks at the copy named by `which`: the first copy inside the head, the second right at its end)
                kw1 = dict(head=hb, where="inside", which="a") if chunk > 1 else {}
                kw2 = dict(head=hb, where="at", which="b") if chunk > 1 else {}
                _add_hosted(protos, chunk, rem, hb + 900, lambda h, hb=hb, k=k, kw=kw1: Duel(
                    0, hb + 900, FLANK + 40, hb + 200, k, kb=k, expect="a", tie=True, note="head, then own tiles", **kw))
                _add_hosted(protos, chunk, rem + TILE, hb + 900, lambda h, hb=hb, k=k, kw=kw2: Duel(
                    0, hb + 900, hb - alen - 5, hb, k, kb=k, expect="a", tie=True, note="end of the head, right behind it", **kw))
    return _finish("ties", protos, chunk, 31, start, end)


EXTREME_PAIRS = [(32, 17), (64, 16), (24, 25), (31, 33), (40, 48), (63, 64)]


def extremes_battery(la, lb):
    """adapters of la / lb bases: a perfect copy alone (count = length: 32 fills the sixth count plane of the short form, 64 the
    seventh), a copy with exactly one substitution in front of / behind a perfect one, and duels with k = 1 .. 3 whose second copy
    lies across byte 1984 -- the boundary of the first two tiles of a read that starts its own tiles at 0: every read when both
    adapters are no longer than 32 bases and the chunk hook is cleared, or when one is longer (no pair packing); the tests run
    both"""
    start, end = random_adapter(1000 + la, la), random_adapter(2000 + lb, lb)
    adapters = (start, end)
    recipes = []
    for ad in (0, 1):
        alen = len(adapters[ad])
        recipes.append(Duel(ad, 1400 + alen, None, 600, 1, kb=0))
        for order in (0, 1):
            a_pos, b_pos = (400, 1300) if order == 0 else (1300, 400)
            recipes.append(Duel(ad, 1700 + alen, a_pos, b_pos, 1))  # one substitution against none
            for k, (x, y) in ((2, ("G", "N")), (3, ("A", "n")), (2, ("T", "U")), (3, ("C", "N"))):
                near, far = 400 + 11 * k, TILE - alen // 2  # (the second copy lies across the boundary of the first two tiles)
                a_pos, b_pos = (near, far) if order == 0 else (far, near)
                recipes.append(Duel(ad, TILE + 2 * alen + FLANK + 37 * k, a_pos, b_pos, k, x, y))
    return Battery("extremes_%d_%d" % (la, lb), recipes, start, end, seed=41 + la)


def split_battery():
    """three copies, the middle one with the Y bytes: C (k ordinary substitutions), A (k times Y for X), B (k - 1) -- or B, A, C:
    the read splits at B, and k_redo scans the pieces -- the one with C and A fails or passes by its N count under
    n_base_limit = 2 (A holds k = 1 .. 3 N's)"""
    recipes = []
    alen = len(START)
    for j, (x, y) in enumerate([("G", "N"), ("A", "N"), ("C", "N"), ("T", "N"), ("G", "n"), ("T", "U")]):
        for k in (1, 2, 3):
            for order in (0, 1):  # C, A, B / B, A, C
                c, a, b = (300, 300 + alen + 200, 300 + 2 * alen + 900) if order == 0 else (1300 + alen + 300, 1300, 320)
                recipes.append(Duel(0, 2600 + 13 * j, a, b, k, x, y, c_pos=c))
    return Battery("split", recipes, opt=dict(n_base_limit=2), seed=51)


FOLD_OPTS = [dict(n_base_percent_limit=100, n_base_limit=65535, complexity_filter=1, complexity_percent=100),
             dict(n_base_percent_limit=50)]


def fold_battery():
    """reads of exactly 65535 and 65536 bases: k_scan reduces the N count and the complexity sum as one 16-bit pair below 65536.
    -> (seq, qual, off), to run under each of FOLD_OPTS.  Filter codes that hang on the exact sums: all N under n_base_limit 65535
    (passes at 65535, fails at 65536) with the percent limit at 100; half N under n_base_percent_limit 50 (nn * 100 == len * 50
    passes, one more N fails); ACAC.. and GNGN.. under complexity 100 % (diff == len - 1 passes, one repeated base fails)"""
    rng = np.random.default_rng(61)
    reads = []
    for L in (65535, 65536):
        acac = np.resize(np.frombuffer(b"AC", np.uint8), L).copy()
        alln = np.full(L, ord("N"), np.uint8)
        rep = acac.copy()
        rep[L // 2] = rep[L // 2 - 1]  # (equal to both its neighbours now: diff = L - 3)
        half = acac.copy()
        half[:L // 2] = ord("N")
        more = half.copy()
        more[L // 2] = ord("N")
        gngn = np.resize(np.frombuffer(b"GN", np.uint8), L).copy()  # (an N differs from the G beside it, whose code bits it shares)
        for s in (alln, acac, rep, half, more, gngn):
            reads.append((s, rng.integers(33 + 20, 33 + 42, L).astype(np.uint8)))
    return synth.pack(reads)
