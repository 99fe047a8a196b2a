"""TEST INFRASTRUCTURE ONLY -- the record streams the device's BAM walk (fastplong_amd/csrc/bam_walk.h) is checked with on the
emulator (tests/test_bam_walk_emu.py), and a pure-Python model of k_bam_find + k_bam_chain that says how many segments the chain
has to walk again.

Records are realistic where it matters to the guess: bases are A/C/G/T (codes 1, 2, 4, 8, so a packed byte is 0x11 .. 0x88),
qualities 20 .. 60, names printable, filler tags 0xFF.  A position inside such bytes never passes the filter: its block_size would
have a fourth byte of 0x11 or more (over 2^28), or l_seq read out of name / base bytes is far larger than block_size.  So in a
plain stream the only candidates are true record starts and the model's rewalk count is 0 by construction; a case that wants a
false candidate plants one (planted_tags)."""
import struct

import numpy as np

from tests import bamio

MAX_TAG_BYTES = 256 << 20
FIND_MAX_BS = 1 << 28
NO_CAND = (1 << 64) - 1
TAKE, SKIP, NEED, BAD = 0, 1, 2, 3


def record(rng, i, l_seq, flag=0, tags=b"", name=None):
    """the bytes of one record"""
    codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), l_seq).tobytes()
    qual = rng.integers(20, 61, l_seq, dtype=np.uint8).tobytes()
    nm = (b"read%d/x" % i) if name is None else name
    return bamio.encode_record(nm, flag, codes, qual, tags=tags)


def records(rng, n, lens=(0, 3, 40, 77, 150, 260, 500), flags=(0, 0x10, 0, 0x4, 0, 0x10)):
    return [record(rng, i, int(lens[i % len(lens)]), flags[i % len(flags)]) for i in range(n)]


def pad_record(rng, i, total_len, flag=0):
    """a record of exactly total_len bytes (>= 60): a short read and filler tags"""
    base = record(rng, i, 8, flag)
    assert total_len >= len(base)
    return record(rng, i, 8, flag, tags=b"\xff" * (total_len - len(base)))


def fake_head(bs, l_name=1, l_seq=0):
    return struct.pack("<IiiBBHHHIiii", bs, -1, -1, l_name, 255, 4680, 0, 0, l_seq, -1, -1, 0)


def planted_tags(before, after):
    """tags that hold a false candidate `before` bytes into them: a record head whose one-byte name is NUL, block_size 33, and
    behind it (where its block_size points) a second plausible head -- all k_bam_find looks at"""
    return b"\xff" * before + fake_head(33) + b"\0" + fake_head(40) + b"\xff" * after


# ---------------------------------------------------------------- the rules, read off the record bytes once more (csrc/bam_rules.h)
def _fields(get, p):
    b = bytes(get(p + k) for k in range(36))
    bs, l_name, n_cigar, flag, l_seq = struct.unpack_from("<I", b, 0)[0], b[12], struct.unpack_from("<H", b, 16)[0], \
        struct.unpack_from("<H", b, 18)[0], struct.unpack_from("<I", b, 20)[0]
    fixed = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    return bs, l_name, n_cigar, flag, l_seq, fixed


def walk_one(get, p, hi):
    avail = hi - p
    if avail < 4:
        return NEED, 0
    bs = struct.unpack("<I", bytes(get(p + k) for k in range(4)))[0]
    if bs < 32:
        return BAD, 0
    if avail < 36:
        return NEED, 0
    bs, l_name, n_cigar, flag, l_seq, fixed = _fields(get, p)
    if l_name < 1 or l_seq > 0x7FFFFFFF or fixed > bs or bs - fixed > MAX_TAG_BYTES + 16 * fixed:
        return BAD, 0
    if avail < 4 + bs:
        return NEED, 0
    if flag & 0x900:
        return SKIP, bs
    if flag & 1:
        return BAD, 0
    if l_seq > 0 and get(p + 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2) == 0xFF:
        return BAD, 0
    return TAKE, bs


def find_ok(get, p, hi):
    avail = hi - p
    if avail < 36:
        return False
    bs, l_name, _, _, l_seq, fixed = _fields(get, p)
    if bs < 32 or bs > FIND_MAX_BS or avail < 4 + bs:
        return False
    if l_name < 1 or l_seq > 0x7FFFFFFF or fixed > bs:
        return False
    if get(p + 36 + l_name - 1) != 0:
        return False
    q = p + 4 + bs
    if q < hi and hi - q >= 36:
        gbs, gl_name, _, _, gl_seq, gfixed = _fields(get, q)
        if gbs < 32 or gbs > FIND_MAX_BS or gl_name < 1 or gl_seq > 0x7FFFFFFF or gfixed > gbs:
            return False
    return True


def model(tail, data, tail_cap, seg, skip=0):
    """k_bam_find and k_bam_chain over [tail | data] as the kernels lay it out -> (rewalked, candidates per segment)"""
    stream = bytes(tail) + bytes(data)
    lo, hi = tail_cap - len(tail), tail_cap + len(data)

    def get(p):
        assert lo <= p < hi, "the model itself reads outside the buffer"
        return stream[p - lo]

    entry = lo + skip
    n_seg = (hi + seg - 1) // seg
    cand = []
    for s in range(n_seg):
        a, b = s * seg, min((s + 1) * seg, hi)
        c = NO_CAND
        if entry < b:
            c = entry if entry >= a else next((p for p in range(a, b) if find_ok(get, p, hi)), NO_CAND)
        cand.append(c)
    e, rew = entry, 0
    for s in range(n_seg):
        a, b = s * seg, min((s + 1) * seg, hi)
        if e >= b:
            continue
        if cand[s] != e:
            if walk_one(get, e, hi)[0] == NEED:  # an incomplete record ends the chain: nothing is walked again
                break
            rew += 1
        stop = False
        while e < b:
            kind, bs = walk_one(get, e, hi)
            if kind in (NEED, BAD):
                stop = True
                break
            e += 4 + bs
        if stop:
            break
    return rew, cand


# ---------------------------------------------------------------- the damaged records of the rule list
def damaged(rng, i, kind):
    good = bytearray(record(rng, i, 50))
    if kind == "block_size_below_32":
        return struct.pack("<I", 20) + bytes(good[4:])
    if kind == "l_name_0":
        good[12] = 0
    elif kind == "l_seq_over_2_31":
        good[20:24] = struct.pack("<I", 0x80000000)
    elif kind == "fields_longer_than_block_size":
        good[0:4] = struct.pack("<I", struct.unpack_from("<I", good, 0)[0] - 8)
    elif kind == "too_many_tag_bytes":
        fixed = 32 + good[12] + 25 + 50
        good[0:4] = struct.pack("<I", fixed + MAX_TAG_BYTES + 16 * fixed + 1)
    elif kind == "flag_0x1":
        good[18:20] = struct.pack("<H", 0x1)
    elif kind == "no_qualities":
        good[36 + good[12] + 25] = 0xFF
    else:
        raise ValueError(kind)
    return bytes(good)


DAMAGE = ["block_size_below_32", "l_name_0", "l_seq_over_2_31", "fields_longer_than_block_size", "too_many_tag_bytes", "flag_0x1",
          "no_qualities"]
