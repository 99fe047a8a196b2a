"""TEST INFRASTRUCTURE ONLY -- the deflate streams the BGZF inflate kernel is checked with, on the emulator
(tests/test_bgzf_inflate_emu.py) and on the device (tests/test_gpu_bgzf.py), and the packing and checking both share.

The yardstick is zlib's raw inflate: a case's expected bytes are what zlib makes of the payload, and `zlib_ok` says whether zlib
accepts the stream at all.  A case says what the kernel must do with it: "ok" (status 0), "refuse" (status != 0) or "any" (a
mutation: whatever the status, a 0 means zlib's bytes)."""
import random
import zlib

import numpy as np

BLOCK_DTYPE = np.dtype([("comp_off", "<u8"), ("out_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("status", "<u4")])
GUARD = 64
FILL = 0xA5


def zlib_inflate(payload):
    """-> (bytes zlib makes of a raw deflate stream, whether it reached the end of a valid stream)"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(payload), 1 << 20)
        return out, bool(d.eof)
    except zlib.error:
        return b"", False


class Case:
    def __init__(self, name, payload, expect="ok", isize=None, crc=None):
        self.name, self.payload, self.expect = name, bytes(payload), expect
        self.data, self.zlib_ok = zlib_inflate(self.payload)
        self.isize = len(self.data) if isize is None else isize
        self.crc = zlib.crc32(self.data[:self.isize]) if crc is None else crc
        # what a correct inflater may give status 0 for: zlib accepts the stream and the trailer agrees with its bytes
        self.may_pass = self.zlib_ok and self.isize == len(self.data) and self.crc == zlib.crc32(self.data)

    def __repr__(self):
        return "Case(%s)" % self.name


# ---------------------------------------------------------------- payloads
def bam_like(n, seed):
    """what a uBAM record stream looks like to deflate: packed 4-bit bases, then qualities with a skewed distribution"""
    r = np.random.RandomState(seed)
    out = bytearray()
    while len(out) < n:
        l = int(r.randint(200, 3000))
        name = ("read_%08x/%d/ccs" % (int(r.randint(0, 1 << 30)), l)).encode() + b"\0"
        hdr = np.zeros(36, np.uint8)
        hdr[12] = len(name)
        nib = r.choice(np.array([1, 2, 4, 8], np.uint8), size=l + (l & 1))
        packed = (nib[0::2] << 4) | nib[1::2]
        q = np.clip(r.normal(30, 8, l), 2, 50).astype(np.uint8)
        out += hdr.tobytes() + name + packed.tobytes() + q.tobytes()
    return bytes(out[:n])


def text(n, seed):
    r = random.Random(seed)
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"BGZF", b"inflate", b"wave", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def payload(kind, n, seed=1):
    if kind == "bam":
        return bam_like(n, seed)
    if kind == "text":
        return text(n, seed)
    if kind == "zero":
        return bytes(n)
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    out = b""
    if flush_every:
        for i in range(0, len(data), flush_every):
            out += c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    else:
        out = c.compress(data)
    return out + c.flush()


# ---------------------------------------------------------------- a bit writer and the codes of RFC 1951
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        """n bits of v, lowest first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """a Huffman code: highest bit first"""
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def done(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (no check of completeness: the bad sets are written with it too)"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


class Coder:
    """literals, matches and the end of the block in the codes of one block"""

    def __init__(self, bw, lit_lens, dist_lens):
        self.bw, self.lit, self.dist = bw, canonical(lit_lens), canonical(dist_lens)

    def sym(self, s):
        self.bw.code(*self.lit[s])

    def lits(self, data):
        for b in data:
            self.sym(b)

    def match(self, length, dist):
        k = max(i for i in range(29) if LEN_BASE[i] <= length) if length != 258 else 28
        self.sym(257 + k)
        self.bw.put(length - LEN_BASE[k], LEN_EXTRA[k])
        d = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.bw.code(*self.dist[d])
        self.bw.put(dist - DIST_BASE[d], DIST_EXTRA[d])

    def dsym(self, d):
        self.bw.code(*self.dist[d])

    def eob(self):
        self.sym(256)


def fixed_block(bw, last=1):
    bw.put(last, 1)
    bw.put(1, 2)
    return Coder(bw, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, last=1, nlen=None):
    bw.put(last, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    bw.raw(data)


CL_FULL = [4] * 13 + [5] * 6  # a complete code over all 19 code-length symbols


def rle(lens):
    """the code-length sequence of lens as (symbol, extra value) pairs: greedy, blind to where HLIT ends"""
    seq, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                seq.append((18, r - 11))
                run -= r
            if run >= 3:
                seq.append((17, run - 3))
                run = 0
            seq += [(0, 0)] * run
        else:
            seq.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                seq.append((16, r - 3))
                run -= r
            seq += [(v, 0)] * run
        i = j
    return seq


def dynamic_block(bw, lit_lens, dist_lens, last=1, cl_lens=None, seq=None, hclen=None, hlit=None, hdist=None):
    """a dynamic header; every part can be overridden to write a bad one"""
    cl_lens = CL_FULL if cl_lens is None else cl_lens
    seq = rle(list(lit_lens) + list(dist_lens)) if seq is None else seq
    if hclen is None:
        hclen = max(i for i in range(19) if cl_lens[CL_ORDER[i]]) + 1
    bw.put(last, 1)
    bw.put(2, 2)
    bw.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
    bw.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
    bw.put(max(hclen, 4) - 4, 4)
    for i in range(max(hclen, 4)):
        bw.put(cl_lens[CL_ORDER[i]], 3)
    cl = canonical(cl_lens)
    for s, x in seq:
        bw.code(*cl[s])
        if s >= 16:
            bw.put(x, {16: 2, 17: 3, 18: 7}[s])
    return Coder(bw, lit_lens, dist_lens)


# ---------------------------------------------------------------- the sets
def writer_cases():
    """streams zlib's deflate writes: the kernel must take every one (refused count 0)"""
    out = []
    strategies = [("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)]
    for kind in ("bam", "text", "zero", "random"):
        data = payload(kind, 5000 if kind != "zero" else 20000, 7)
        for level in (0, 1, 6, 9):
            for sname, s in strategies:
                out.append(Case("writer/%s/l%d/%s" % (kind, level, sname), deflate(data, level, s)))
    out.append(Case("writer/full_flush", deflate(payload("bam", 9000, 3), 6, flush_every=1500)))
    out.append(Case("writer/full_flush_l1", deflate(payload("text", 9000, 3), 1, flush_every=777)))
    out.append(Case("writer/trailing_bytes", deflate(payload("text", 300, 5), 6) + b"\x13\x37\xff"))
    return out


def shape_cases():
    """isize 0, 1, 63, 64, 65, 65280 and 65536"""
    out = []
    for n in (0, 1, 63, 64, 65, 65280, 65536):
        out.append(Case("shape/%d" % n, deflate(payload("bam", n, 11), 1)))
    return out


def hand_cases():
    out = []
    noise = payload("random", 32768 + 300, 21)
    for length in (3, 258):
        for dist in (1, 2, 63, 64, 65, 32768):
            bw = Bits()
            c = fixed_block(bw)
            c.lits(noise[:dist + 7] if dist < 32768 else noise[:32768])
            c.match(length, dist)
            c.lits(b"xy")
            c.match(length, dist)
            c.eob()
            out.append(Case("hand/match_len%d_dist%d" % (length, dist), bw.done()))
    bw = Bits()
    c = fixed_block(bw)
    for k in range(1, 70, 7):  # the source is the literals decoded just before: still in the lanes' registers when the match comes
        c.lits(noise[k:2 * k + 1])
        c.match(k + 3, k + 1)
    c.eob()
    out.append(Case("hand/match_of_fresh_literals", bw.done()))
    bw = Bits()
    stored_block(bw, b"", last=0)
    stored_block(bw, b"abc", last=0)
    stored_block(bw, b"")
    out.append(Case("hand/stored_len0", bw.done()))
    bw = Bits()
    stored_block(bw, noise[:65535] if len(noise) >= 65535 else (noise * 3)[:65535])
    out.append(Case("hand/stored_len65535", bw.done()))
    bw = Bits()
    c = fixed_block(bw, last=0)
    c.lits(b"q")
    c.eob()  # 3 + 8 + 7 bits: the stored block's header starts at bit 18
    stored_block(bw, b"stored after a fixed block", last=0)
    c = fixed_block(bw)
    c.match(10, 5)
    c.eob()
    out.append(Case("hand/stored_at_odd_bit", bw.done()))
    # dynamic: HCLEN 19, repeat code 16 running from the literal lengths into the distance lengths
    lit = [8] * 254 + [9] * 4
    dist = [9, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    bw = Bits()
    c = dynamic_block(bw, lit, dist)
    c.lits(noise[:100])
    c.match(3, 1)    # distance symbol 0: a 9-bit distance code (longer than the distance table's 8 bits)
    c.match(3, 7)    # distance symbol 5
    c.sym(255)
    c.sym(254)
    c.eob()
    out.append(Case("hand/dynamic_hclen19_rep16_across", bw.done()))
    assert (9, 0) in rle(lit + dist) and (16, 2) in rle(lit + dist)
    # repeat code 18 running across the boundary
    lit = [8] * 254 + [9] * 4 + [0] * 12
    dist = [0, 0, 0, 1, 1]
    bw = Bits()
    c = dynamic_block(bw, lit, dist)
    c.lits(b"zeros run across the boundary")
    c.match(3, 4)
    c.match(3, 5)
    c.eob()
    out.append(Case("hand/dynamic_rep18_across", bw.done()))
    assert (18, 4) in rle(lit + dist)
    # 15-bit codes: lengths 1 .. 13 and four of 15, the end-of-block code and length 258 among the longest
    lit = [0] * 286
    for k in range(13):
        lit[97 + k] = k + 1
    lit[110] = lit[111] = lit[256] = lit[285] = 15
    bw = Bits()
    c = dynamic_block(bw, lit, [1, 1])
    c.lits(b"abcdefghijklmnoonmlkjihgfedcba" * 3)
    c.match(258, 2)
    c.lits(b"o")
    c.eob()
    out.append(Case("hand/dynamic_15bit_codes", bw.done()))
    return out


def hclen4_case():
    """HCLEN 4 gives lengths to the code-length symbols 16, 17, 18 and 0 only, so every literal length it can describe is 0: there is
    no legal stream with it.  zlib rejects it, and the kernel must refuse it."""
    bw = Bits()
    cl = [0] * 19
    cl[16] = cl[17] = cl[18] = cl[0] = 2
    dynamic_block(bw, [0] * 257, [0], cl_lens=cl, hclen=4)
    bw.put(0, 16)
    return Case("refuse/dynamic_hclen4", bw.done(), "refuse")


def refuse_cases():
    out = [hclen4_case()]
    bw = Bits()
    bw.put(1, 1)
    bw.put(3, 2)
    bw.put(0, 29)
    out.append(Case("refuse/block_type_3", bw.done(), "refuse", isize=0, crc=0))
    bw = Bits()
    stored_block(bw, b"abcd", nlen=0x1234)
    out.append(Case("refuse/len_not_nlen", bw.done(), "refuse", isize=4, crc=zlib.crc32(b"abcd")))
    ok_lit = [8] * 254 + [9] * 4

    def dyn(name, lit, dist, tail=b"", isize=0, **kw):
        bw = Bits()
        dynamic_block(bw, lit, dist, **kw)
        bw.out += tail
        bw.put(0, 32)
        out.append(Case("refuse/" + name, bw.done(), "refuse", isize=isize, crc=0))

    dyn("oversubscribed_lit", [1, 1, 1] + [0] * 253 + [8], [1, 1])
    dyn("oversubscribed_dist", ok_lit, [1, 1, 1])
    dyn("incomplete_lit", [8] * 254 + [9] * 3, [1, 1])
    dyn("incomplete_dist_two", ok_lit, [2, 2])
    dyn("no_dist_code", ok_lit, [0])
    cl = list(CL_FULL)
    cl[18] = 0
    dyn("incomplete_cl", ok_lit, [1, 1], cl_lens=cl)
    cl = list(CL_FULL)
    cl[18] = 4
    dyn("oversubscribed_cl", ok_lit, [1, 1], cl_lens=cl)
    dyn("rep16_without_previous", ok_lit, [1, 1], seq=[(16, 0)] + rle(ok_lit + [1, 1])[1:])
    dyn("lengths_past_the_end", ok_lit, [1, 1], seq=rle(ok_lit) + [(1, 0), (16, 3)])
    dyn("zeros_past_the_end", ok_lit, [1, 1], seq=rle(ok_lit) + [(1, 0), (18, 0)])
    dyn("no_end_of_block", [8] * 256 + [0], [1, 1])
    # the single 1-bit distance code: zlib takes it, this kernel does not (every incomplete set is refused)
    bw = Bits()
    c = dynamic_block(bw, ok_lit, [1])
    c.lits(b"one distance code")
    c.eob()
    single = Case("refuse/single_distance_code", bw.done(), "refuse")
    assert single.zlib_ok and single.data == b"one distance code"
    out.append(single)
    for s in (286, 287):
        bw = Bits()
        c = fixed_block(bw)
        c.lits(b"ab")
        c.sym(s)
        bw.put(0, 5)
        bw.put(0, 32)
        out.append(Case("refuse/symbol_%d" % s, bw.done(), "refuse", isize=5, crc=0))
    for d in (30, 31):
        bw = Bits()
        c = fixed_block(bw)
        c.lits(b"abcdefgh")
        c.sym(257)
        c.dsym(d)
        bw.put(0, 32)
        out.append(Case("refuse/distance_code_%d" % d, bw.done(), "refuse", isize=11, crc=0))
    bw = Bits()
    c = fixed_block(bw)
    c.lits(b"a")
    c.match(3, 2)
    c.eob()
    out.append(Case("refuse/distance_before_start", bw.done(), "refuse", isize=4, crc=0))
    good = payload("text", 400, 9)
    z = deflate(good, 6)
    out.append(Case("refuse/more_than_isize", z, "refuse", isize=399, crc=zlib.crc32(good[:399])))
    out.append(Case("refuse/more_than_isize_match", deflate(bytes(500), 6), "refuse", isize=300, crc=zlib.crc32(bytes(300))))
    out.append(Case("refuse/less_than_isize", z, "refuse", isize=401, crc=zlib.crc32(good)))
    out.append(Case("refuse/stored_more_than_isize", deflate(good, 0), "refuse", isize=100, crc=zlib.crc32(good[:100])))
    out.append(Case("refuse/crc", z, "refuse", isize=400, crc=zlib.crc32(good) ^ 1))
    out.append(Case("refuse/input_overrun_cut_in_data", z[:len(z) // 2], "refuse", isize=400, crc=zlib.crc32(good)))
    # (the end-of-block code of the fixed code is seven zero bits: cut off, the zeros behind the end would decode as it)
    bw = Bits()
    c = fixed_block(bw)
    c.lits(b"ends with the fixed end-of-block code")
    bw.align()
    whole = Bits()
    c2 = fixed_block(whole)
    c2.lits(b"ends with the fixed end-of-block code")
    c2.eob()
    assert Case("x", whole.done()).zlib_ok
    out.append(Case("refuse/input_overrun_cut_before_eob", bytes(bw.out), "refuse", isize=37, crc=zlib.crc32(b"ends with the fixed end-of-block code")))
    zs = deflate(good, 0)
    out.append(Case("refuse/input_overrun_stored", zs[:-10], "refuse", isize=400, crc=zlib.crc32(good)))
    return out


def mutation_cases(seed=5):
    """every single bit of the first 200 payload bytes of a few valid blocks flipped, plus 2000 seeded random positions"""
    bases = [deflate(payload("bam", 700, 31), 1), deflate(payload("text", 600, 32), 6), deflate(payload("text", 500, 33), 6, zlib.Z_FIXED),
             deflate(payload("random", 300, 34), 0)]
    out = []
    r = random.Random(seed)
    for bi, z in enumerate(bases):
        data = zlib_inflate(z)[0]
        pos = [(i, b) for i in range(min(200, len(z))) for b in range(8)]
        pos += [(r.randrange(len(z)), r.randrange(8)) for _ in range(2000 // len(bases))]
        for i, b in pos:
            m = bytearray(z)
            m[i] ^= 1 << b
            out.append(Case("mut/%d/%d.%d" % (bi, i, b), bytes(m), "any", isize=len(data), crc=zlib.crc32(data)))
    return out


# ---------------------------------------------------------------- packing and checking
def pack(cases, seed=1):
    """-> (comp, blocks, out): payloads at odd offsets with gaps between them, output ranges in an order of their own, GUARD bytes
    of FILL around each"""
    r = random.Random(seed)
    blocks = np.zeros(len(cases), BLOCK_DTYPE)
    comp = bytearray()
    for i, c in enumerate(cases):
        comp += bytes([FILL]) * (GUARD + r.randrange(1, 8))
        blocks[i]["comp_off"] = len(comp)
        blocks[i]["comp_len"] = len(c.payload)
        comp += c.payload
    comp += bytes([FILL]) * GUARD
    order = list(range(len(cases)))
    r.shuffle(order)
    at = 0
    for i in order:
        at += GUARD + r.randrange(0, 8)
        blocks[i]["out_off"] = at
        blocks[i]["isize"] = cases[i].isize
        blocks[i]["crc32"] = cases[i].crc & 0xFFFFFFFF
        blocks[i]["status"] = 0xDEAD
        at += cases[i].isize
    out = np.full(at + GUARD, FILL, np.uint8)
    return np.frombuffer(bytes(comp), np.uint8).copy(), blocks, out


def check(cases, blocks_in, out, status):
    """the rules: nothing outside the ranges is touched; status as the case expects; a 0 only with zlib's bytes and zlib's consent"""
    mask = np.ones(len(out), bool)
    for b in blocks_in:
        mask[int(b["out_off"]):int(b["out_off"]) + int(b["isize"])] = False
    assert (out[mask] == FILL).all(), "bytes outside the blocks' output ranges were written"
    refused = 0
    for c, b, st in zip(cases, blocks_in, status):
        st = int(st)
        if c.expect == "ok":
            assert c.may_pass, c.name
            assert st == 0, "%s: status %d" % (c.name, st)
        elif c.expect == "refuse":
            assert st != 0, "%s: status 0" % c.name
        if st == 0:
            assert c.may_pass, "%s: status 0 for a stream zlib rejects or a trailer that disagrees" % c.name
            got = out[int(b["out_off"]):int(b["out_off"]) + c.isize].tobytes()
            assert got == c.data, "%s: bytes differ from zlib's" % c.name
        else:
            refused += 1
    return refused
