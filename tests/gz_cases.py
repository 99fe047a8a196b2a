"""Test helpers shared by the emulator and the device tests of the deflate kernels (fastplong_amd/csrc/gz_emit.h: k_gz_block,
k_gz_block_bgzf, k_gz_finish, k_gz_finish_bgzf): a reference written from RFC 1951 alone, the inputs that reach the limits of the
coder, and the assertions every coded block has to meet.

Nothing here is derived from gz_emit.h.  What is taken from its DOCUMENTED format: a device block is byte-aligned -- a dynamic
block followed by the empty stored block 00 00 00 FF FF, or one stored block --, blocks start at every multiple of 16 384 of the
text and at the name line and the '+' line of a record whose bases line has at least 1 024 bytes, and the header writes zero runs
as symbols 18 (11..138), then 17 (3..10), then literal zeros, and never symbol 16.

MARGIN: the coder limits code lengths with a heuristic (fold everything deeper than 15 into 15, then repair the Kraft sum), so a
block whose unlimited Huffman tree is deeper than 15 may cost more than the length-limited optimum (package-merge).  The worst
excess over the whole battery -- every block of as_fastq(block_battery()) in both framings and every battery block alone --
measured on the emulator is 0.0539 % (the Lucas block inside as_fastq, with its '@', line end and 'A's: 40 866 bits against
40 844; alone it is 39 573 against 39 566, 0.0177 %; docs/kernels.md has the table); rounded up to the next 0.05 percentage
point that is MARGIN.  A block whose unlimited tree fits 15 bits must cost exactly the optimum."""
import functools
import heapq
import struct
import zlib

import numpy as np

from tests.bgzf_out_cases import STRIPE, rand_read, split_blocks

GZ_B, GZ_L, GZ_STRETCH = 16384, 1024, 64
MARGIN = 0.001  # 0.10 %
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# lengths of a last block at the edges of the 16-byte loads and stores and of a thread's stretch of S symbols
TAIL_LENGTHS = (lambda S, B: sorted({1, 2, 3, 15, 16, 17, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1, 77 * S - 1, 77 * S + 1, B - S - 1, B - S + 1,
                                     B - 1}))(GZ_STRETCH, GZ_B)


# ---- the reference ----
class Bits:
    """deflate's bit order: fields from the low bit of every byte up, Huffman codes from their most significant bit"""

    def __init__(self, buf, pos=0):
        self.buf, self.pos = buf, pos

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.buf[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v

    def symbol(self, table):
        code, n = 0, 0
        while True:
            code, n = (code << 1) | self.take(1), n + 1
            assert n <= 15, "no code matches"
            if (n, code) in table:
                return table[(n, code)]


def canonical(lens):
    """{(length, code): symbol} of RFC 1951 3.2.2"""
    lens = [int(l) for l in lens]
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, first = 0, [0] * 17
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        first[l] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, first[l])] = s
            first[l] += 1
    return table


def parse_dynamic_header(buf, bitpos=0):
    """the header of the dynamic block at bit `bitpos` of buf (RFC 1951 3.2.7) -> dict: final, lit (the HLIT literal/length code
    lengths), dist (the HDIST distance code lengths), cl (the 19 lengths of the code-length code), cl_hist (how often each of the 19
    symbols was used) and end, the bit behind the header"""
    r = Bits(buf, bitpos)
    final, btype = r.take(1), r.take(2)
    assert btype == 2, "not a dynamic block: BTYPE %d" % btype
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = r.take(3)
    table = canonical(cl)
    lens, hist = [], [0] * 19
    while len(lens) < hlit + hdist:
        s = r.symbol(table)
        hist[s] += 1
        if s < 16:
            lens.append(s)
        elif s == 16:
            assert lens, "repeat with nothing in front"
            lens += [lens[-1]] * (3 + r.take(2))
        elif s == 17:
            lens += [0] * (3 + r.take(3))
        else:
            lens += [0] * (11 + r.take(7))
    assert len(lens) == hlit + hdist, "code lengths run past HLIT + HDIST"
    return dict(final=final, lit=lens[:hlit], dist=lens[hlit:], cl=cl, cl_hist=hist, end=r.pos)


def huffman_depth(freqs):
    """the depth of the plain, unlimited Huffman tree over the counts that are not 0 (ties go to the shallower subtree, which
    gives the least depth any optimal tree has); one symbol: 1"""
    heap = [(int(f), 0) for f in freqs if f]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def huffman_cost(freqs):
    """sum(count * length) of the unlimited Huffman code"""
    heap = [int(f) for f in freqs if f]
    if len(heap) < 2:
        return sum(heap)
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        cost += s
        heapq.heappush(heap, s)
    return cost


def package_merge(freqs, limit):
    """the least sum(count * length) any prefix code with no length above `limit` has (Larmore & Hirschberg's package-merge: the
    2 n - 2 cheapest items of the last of `limit` merged lists; an item's weight is the sum of the leaves in it, and a leaf's code
    length is the number of chosen items it is in, so the chosen weights add up to the cost)"""
    leaves = sorted(int(f) for f in freqs if f)
    n = len(leaves)
    if n < 2:
        return sum(leaves)
    assert n <= 1 << limit, "no code of that length limit exists"
    cur = leaves
    for _ in range(limit - 1):
        packages = [cur[k] + cur[k + 1] for k in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packages)
    return sum(cur[:2 * n - 2])


def cl_freqs(lens, n_dist):
    """how often each of the 19 code-length symbols appears when the 257 literal lengths `lens` and n_dist distance lengths of 1
    are written by the documented rule: a run of zeros as 18s of 11..138, then one 17 of 3..10, then literal zeros; no 16"""
    seq = [int(l) for l in lens] + [1] * n_dist
    hist, i = [0] * 19, 0
    while i < len(seq):
        if seq[i]:
            hist[seq[i]] += 1
            i += 1
            continue
        run = 0
        while i < len(seq) and seq[i] == 0:
            run, i = run + 1, i + 1
        while run >= 11:
            hist[18] += 1
            run -= min(run, 138)
        if run >= 3:
            hist[17] += 1
            run = 0
        hist[0] += run
    return hist


def block_starts(want):
    """where the layout cuts the formatted text into deflate blocks (the rule of tests/test_gpu_bgzf_out.py::deflate_blocks):
    every multiple of GZ_B, and the name line and the '+' line of a record whose bases line has at least GZ_L bytes"""
    starts, o = set(range(0, len(want), GZ_B)), 0
    lines = want.split(b"\n")
    for i in range(0, len(lines) - 1, 4):
        a = len(lines[i]) + len(lines[i + 1]) + 2
        if len(lines[i + 1]) + 1 >= GZ_L:
            starts.update((o, o + a))
        o += a + len(lines[i + 2]) + len(lines[i + 3]) + 2
    return sorted(starts)


def walk(stream, text, starts, at=0):
    """a deflate stream of device blocks, block by block: starts are where the blocks begin in the whole text, of which `text`
    is the part from `at` on that the stream holds.  Every block is checked to be what the format says (byte-aligned, closed by
    the empty stored block or stored whole, zero padding) and is inflated ALONE with zlib.  -> a dict per block"""
    starts = [s - at for s in starts if at <= s < at + len(text)] + [len(text)]
    assert starts[0] == 0
    out, p = [], 0
    for s, e in zip(starts, starts[1:]):
        t = text[s:e]
        n = len(t)
        assert 1 <= n <= GZ_B
        freqs = np.bincount(np.frombuffer(t, np.uint8), minlength=257)
        freqs[256] = 1
        blk = dict(start=at + s, n=n, freqs=freqs)
        btype = (stream[p] >> 1) & 3
        assert stream[p] & 1 == 0, "BFINAL inside the stream"
        if btype == 0:
            assert stream[p:p + 5] == struct.pack("<BHH", 0, n, ~n & 0xFFFF), "stored header of block at %d" % blk["start"]
            assert stream[p + 5:p + 5 + n] == t
            size = 5 + n
            blk.update(stored=True)
        else:
            h = parse_dynamic_header(stream, 8 * p)
            assert len(h["lit"]) == 257
            lens = np.array(h["lit"])
            assert (lens[freqs > 0] > 0).all(), "a symbol that occurs has no code"
            body = int((freqs * lens).sum())
            end_bits = h["end"] - 8 * p + body
            size = (end_bits + 3 + 7) // 8 + 4
            r = Bits(stream, 8 * p + end_bits)
            assert r.take(8 * (size - 4) - end_bits) == 0, "the stored header and the padding are zero bits"
            assert stream[p + size - 4:p + size] == b"\x00\x00\xff\xff"
            blk.update(stored=False, hdr=h, body=body, hdr_bits=h["end"] - 8 * p)
        raw = stream[p:p + size]
        d = zlib.decompressobj(-15)
        assert d.decompress(raw + b"\x01\x00\x00\xff\xff") == t and d.eof and d.unused_data == b"", "block at %d alone" % blk["start"]
        blk.update(raw=raw, size=size)
        out.append(blk)
        p += size
    assert stream[p:] == b"\x01\x00\x00\xff\xff", "the final empty block"
    return out


def member_blocks(member, text, starts=None):
    """the deflate blocks of a device member; header and trailer checked.  starts: where the blocks begin when the text is not
    FASTQ the layout cut (emu_gz.deflate cuts any bytes at the multiples of GZ_B)"""
    assert member[:10] == bytes.fromhex("1f8b08000000000000ff")
    assert member[-8:] == struct.pack("<II", zlib.crc32(text), len(text) % 2 ** 32), "CRC-32 and ISIZE"
    return walk(member[10:-8], text, block_starts(text) if starts is None else starts)


def bgzf_blocks(data, text):
    """the deflate blocks of the device's BGZF blocks, stripe by stripe; every frame's trailer checked"""
    starts, out = block_starts(text), []
    frames = split_blocks(data)
    assert len(frames) == -(-len(text) // STRIPE)
    for k, f in enumerate(frames):
        t = text[k * STRIPE:(k + 1) * STRIPE]
        assert f[-8:] == struct.pack("<II", zlib.crc32(t), len(t)), "CRC-32 and ISIZE of BGZF block %d" % k
        out += walk(f[18:-8], t, starts, at=k * STRIPE)
    return out


def kraft(lens, maxbits):
    return sum(1 << (maxbits - int(l)) for l in lens if l)


def min_dynamic_bytes(freqs, n_dist):
    """a lower bound of what ANY dynamic block for these counts takes in the device's form, whatever code it picks: 17 bits in
    front; 18 entries of 3 bits (the distance lengths are 1, and 1 is the 18th entry); the zero runs, which the counts alone
    decide, at one bit a symbol and 3 or 7 extra bits; one bit for every length that is not 0; the length-limited optimum for
    the body; 3 bits of stored header; 4 bytes"""
    hist = cl_freqs((np.asarray(freqs) > 0).astype(int), n_dist)
    bits = 17 + 3 * 18 + hist[0] + 4 * hist[17] + 8 * hist[18] + hist[1] + package_merge(freqs, 15) + 3
    return (bits + 7) // 8 + 4


def check_block(blk, n_dist):
    """the assertions on one block of walk() (n_dist: 1 in a member, 2 in BGZF) -> dict of what was measured: stored, depth (the
    unlimited tree's), longest (the longest code), cl_depth, cl_longest, cost, optimum, excess"""
    freqs, n = blk["freqs"], blk["n"]
    where = "block at %d" % blk["start"]
    optimum = package_merge(freqs, 15)
    depth = huffman_depth(freqs)
    if blk["stored"]:
        # stored exactly when a dynamic block would not be smaller: no dynamic block at all can be
        low = min_dynamic_bytes(freqs, n_dist)
        assert low >= n + 5, "%s is stored in %d bytes, a dynamic block might take %d" % (where, n + 5, low)
        return dict(stored=True, depth=depth, optimum=optimum)
    assert blk["size"] < n + 5, "%s: coded in %d bytes, stored is %d" % (where, blk["size"], n + 5)
    h = blk["hdr"]
    lens, cl = np.array(h["lit"]), np.array(h["cl"])
    assert ((lens > 0) == (freqs > 0)).all(), where + ": codes exactly for the symbols that occur, and end-of-block"
    assert lens.max() <= 15 and cl.max() <= 7, where
    assert h["dist"] == [1] * n_dist, where
    assert kraft(lens, 15) == 1 << 15, where + ": the literal code is complete"  # (end-of-block and a byte: never one symbol)
    hist = cl_freqs(lens, n_dist)
    assert h["cl_hist"] == hist and hist[16] == 0, where + ": the run-length symbols of the documented rule"
    assert ((cl > 0) == (np.array(hist) > 0)).all(), where
    if (cl > 0).sum() >= 2:
        assert kraft(cl, 7) == 1 << 7, where + ": the code-length code is complete"
    else:
        assert cl.max() == 1, where
    cost = int((freqs * lens).sum())
    assert cost >= optimum, "%s: cost %d below the optimum %d -- the reference is wrong" % (where, cost, optimum)
    if depth <= 15:
        assert cost == optimum, "%s: the unlimited tree has depth %d, cost %d, optimum %d" % (where, depth, cost, optimum)
    assert cost <= (1 + MARGIN) * optimum, "%s: cost %d, optimum %d: %.4f %% over" % (where, cost, optimum, 100.0 * (cost - optimum) / optimum)
    cl_cost, cl_opt = int((np.array(hist) * cl).sum()), package_merge(hist, 7)
    assert cl_cost >= cl_opt, where
    if huffman_depth(hist) <= 7:
        assert cl_cost == cl_opt, where + ": the code-length code's tree fits 7 bits and is not the optimum"
    return dict(stored=False, depth=depth, longest=int(lens.max()), cl_depth=huffman_depth(hist), cl_longest=int(cl.max()), cost=cost,
                optimum=optimum, excess=(cost - optimum) / optimum, n_lens=int((lens > 0).sum()))


def check_case(name, m, alone=False):
    """the preconditions of a battery case on the block that holds it (m: check_block's result; alone: the block by itself, not
    in a name line): that the input reaches what it was made for.  They FAIL, never skip."""
    if name.startswith("lucas"):
        assert not m["stored"] and m["depth"] > 15 and m["longest"] == 15, (name, m)
    elif name.startswith("deep_header"):
        assert not m["stored"] and m["cl_depth"] > 7 and m["cl_longest"] == 7, (name, m)
    elif name == "stored_256x64":
        assert m["stored"], (name, m)
    else:
        assert not m["stored"], (name, m)
    if name == "two_heavy_254_singletons":  # (a name line holds neither line end; the block in as_fastq has the '\n' behind it)
        assert m["n_lens"] == (257 if alone else 256), (name, m)
    if name == "fib17_200_singletons":
        assert m["n_lens"] >= 218, (name, m)


def check_battery(blocks, where, n_dist):
    """check_block on every block of as_fastq(block_battery())'s output (member_blocks / bgzf_blocks), check_case on the blocks
    that carry a case -> {name: check_block's result}"""
    by_start = {b["start"]: check_block(b, n_dist) for b in blocks}
    out = {}
    for name, at in where.items():
        check_case(name, by_start[at])
        out[name] = by_start[at]
    assert tuple(out) == BATTERY_NAMES
    return out


def excess_line(name, m):
    if m["stored"]:
        return "%-26s stored (unlimited depth %d)" % (name, m["depth"])
    return "%-26s depth %2d, longest %2d, header code depth %d -> %d, %6d bits, optimum %6d, %.4f %% over" % (
        name, m["depth"], m["longest"], m["cl_depth"], m["cl_longest"], m["cost"], m["optimum"], 100.0 * m["excess"])


# ---- the inputs ----
def lucas_counts(limit=GZ_B):
    c = [1, 3]
    while sum(c) + c[-1] + c[-2] <= limit:
        c.append(c[-1] + c[-2])
    return c


def _spread(counts, values, rng=None):
    a = np.concatenate([np.full(c, v, np.uint8) for c, v in zip(counts, values)])
    if rng is not None:
        rng.shuffle(a)
    return a.tobytes()


NAME_BYTES = [v for v in range(256) if v not in (10, 13)]
# seeds of dyadic_block whose header, alone and inside as_fastq(block_battery()) in either framing, needs a code-length code
# deeper than 7 bits (found by a search over the seeds 0..; only the parameters are kept)
DEEP_HEADER_SEEDS = (0, 5, 14)


def dyadic_block(seed):
    """GZ_B - 1 bytes whose counts are powers of two, 2^(14 - l) for a random complete set of code lengths l <= 14 (one code of 14
    bits is left for end-of-block): the Huffman code IS that set, so the seed decides how many codes of each length the header
    has to write -- the counts the code-length code is built from"""
    rng = np.random.default_rng([seed, 77])
    lens = [1, 1]
    target = int(rng.integers(24, 200))
    skew = float(rng.uniform(0.0, 3.0))
    while len(lens) < target or max(lens) < 14:
        open_ = [k for k, l in enumerate(lens) if l < 14]
        if len(lens) >= target:
            k = max(open_, key=lambda k: lens[k])
        else:
            w = np.array([lens[k] for k in open_], float) ** skew
            k = open_[int(rng.choice(len(open_), p=w / w.sum()))]
        lens[k] += 1
        lens.append(lens[k])
    lens.remove(14)
    values = rng.permutation(NAME_BYTES)[:len(lens)]
    return _spread([1 << (14 - l) for l in lens], values, rng)


BATTERY_NAMES = ("lucas_shuffled", "lucas_sorted", "lucas_topped_up", "fib17_200_singletons", "two_heavy_254_singletons", "stored_256x64",
                 "one_symbol", "two_alternating", "high_bytes", "deep_header_0", "deep_header_1", "deep_header_2")


@functools.lru_cache(maxsize=None)
def _battery():
    return tuple(_build_battery().items())


def block_battery():
    """{name: bytes}, each at most GZ_B bytes: the inputs that reach the coder's limits"""
    return dict(_battery())


def _build_battery():
    rng = np.random.default_rng(2024)
    luc = lucas_counts()
    assert len(luc) == 18 and sum(luc) == 15124  # (19 symbols with end-of-block)
    alpha = list(range(0x30, 0x30 + len(luc)))
    out = {}
    out["lucas_shuffled"] = _spread(luc, alpha, rng)
    out["lucas_sorted"] = _spread(luc, alpha)
    out["lucas_topped_up"] = _spread(luc[:-1] + [luc[-1] + GZ_B - sum(luc)], alpha, rng)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    out["fib17_200_singletons"] = _spread(fib + [1] * 200, NAME_BYTES[20:20 + 217], rng)
    heavy = [GZ_B // 2 - 100, GZ_B - 2 - 254 - (GZ_B // 2 - 100)]  # (GZ_B - 2 bytes: in as_fastq the '@' and a line end fit beside them)
    out["two_heavy_254_singletons"] = _spread(heavy + [1] * 254, [65, 67] + [v for v in range(256) if v not in (65, 67)], rng)
    out["stored_256x64"] = _spread([64] * 256, range(256), rng)
    out["one_symbol"] = b"G" * GZ_B
    out["two_alternating"] = b"AB" * (GZ_B // 2)
    hi = np.minimum(rng.geometric(0.06, 12345) - 1, 127).astype(np.uint8) + 0x80
    out["high_bytes"] = hi.tobytes()
    for k, seed in enumerate(DEEP_HEADER_SEEDS):
        out["deep_header_%d" % k] = dyadic_block(seed)
    assert all(1 <= len(b) <= GZ_B for b in out.values()) and tuple(out) == BATTERY_NAMES
    return out


def _record(name, n=1):
    return b"@" + name + b"\n" + b"A" * n + b"\n+\n" + b"I" * n + b"\n"


def as_fastq(blocks):
    """regular FASTQ that carries every block in a name line -> (text, {name: where the deflate block with it starts}).  A name
    holds no line end: bytes 10 and 13 of a block go in as 11 and 14.  In front of every carrying record stands a padding record
    whose name is sized so that the carrying record's '@' falls on a multiple of GZ_B -- a block start -- and the block's first
    byte is the one behind it.  The carrying record's bases line, all 'A', reaches over the next multiple of GZ_B, so the deflate
    block holds the '@', GZ_B - 1 bytes of the name at most, and for a shorter name one line end and 'A's: a count of 1 more
    and a larger count for 'A' (the Lucas blocks' most frequent byte), which a chain of Lucas counts survives; the five line ends
    and the other lines of a one-base record would cut its depth to 12.  Whoever checks a block counts the bytes of the TEXT."""
    text, where = b"", {}
    swap = bytes.maketrans(b"\n\r", b"\x0b\x0e")
    for name, blk in blocks.items():
        pad = -(len(text) + len(_record(b""))) % GZ_B
        text += _record(b"p" * (pad if pad else GZ_B))
        assert len(text) % GZ_B == 0
        where[name] = len(text)
        text += _record(bytes(blk).translate(swap), max(1, GZ_B - len(blk) - 1))
    return text, where


def tail_text(r, seed=11):
    """regular FASTQ of exactly 3 * GZ_B + r bytes whose last deflate block holds exactly r: bgzf_out_cases.exact_text with every
    read below GZ_L bases (exact_text's last read may reach 1 246 bases, and its forced starts would cut the tail)"""
    rng = np.random.default_rng(seed)
    total, out, i = 3 * GZ_B + r, b"", 0
    while total - len(out) > 1900:
        out += rand_read(rng, 600, b"@e%d" % i)
        i += 1
    left = total - len(out)
    name = b"@z" if left % 2 else b"@zz"
    out += rand_read(rng, (left - len(name) - 5) // 2, name)
    assert len(out) == total and block_starts(out) == [0, GZ_B, 2 * GZ_B, 3 * GZ_B]
    return out


def many_blocks_text(n_reads, seed=21):
    """reads of 1 024 .. 1 039 bases: every record forces two block starts"""
    rng = np.random.default_rng(seed)
    return b"".join(rand_read(rng, int(n), b"@m%d" % i) for i, n in enumerate(rng.integers(1024, 1040, n_reads)))


def per_thread_runs(n_blocks):
    """`per` of k_gz_finish_bgzf: the blocks each of its 1 024 threads takes"""
    return -(-n_blocks // 1024)
