"""TEST HELPER: a pure-Python BAM writer (zlib + struct) with controllable BGZF block cuts, an independent bam_to_fastq that
implements the project's twin rule (README "BAM input"), and a random record generator over all 16 base codes.

The twin rule: records with flag 0x100 / 0x800 are skipped; every other record is "@name\\nbases\\n+\\nqual+33\\n" with bases from
"=ACMGRSVTWYHKDBN" (high nibble first), phred values above 93 clamped to 93, and for flag 0x10 the bases reverse-complemented
and the qualities reversed.  Flag 0x1, a first quality byte of 0xFF, a block_size that disagrees with the fields and a file cut
inside a record are errors (BamError)."""
import gzip
import struct
import zlib

import numpy as np

CODES = b"=ACMGRSVTWYHKDBN"
COMP = b"=TGKCYSBAWRDMHVN"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class BamError(ValueError):
    pass


def encode_record(name, flag, codes, qual, n_cigar=0, tags=b"", block_size_delta=0):
    """one BAM record (block_size included).  codes: sequence of 4-bit codes; qual: raw phred bytes (len == len(codes))"""
    codes = bytes(codes)
    l_seq = len(codes)
    packed = bytearray((l_seq + 1) // 2)
    for i, c in enumerate(codes):
        packed[i >> 1] |= (c << 4) if i % 2 == 0 else c
    rname = name + b"\0"
    cigar = b"".join(struct.pack("<I", (10 << 4) | 0) for _ in range(n_cigar))
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(rname), 255, 4680, n_cigar, flag, l_seq, -1, -1, 0)
    body += rname + cigar + bytes(packed) + bytes(qual) + tags
    return struct.pack("<I", len(body) + block_size_delta) + body


def header(text=b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:basecaller\tPN:test\n", refs=((b"chr1", 1000), (b"chrM", 16569))):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for nm, ln in refs:
        h += struct.pack("<i", len(nm) + 1) + nm + b"\0" + struct.pack("<i", ln)
    return h


def bgzf_block(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    bsize = 12 + 6 + len(cdata) + 8 - 1
    assert bsize < 65536
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + cdata +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf(data, cuts=None, block=65280, eof=True, level=6):
    """BGZF of `data`: blocks end at the uncompressed positions `cuts` (sorted), and every `block` bytes in between"""
    out, pos = [], 0
    cuts = sorted(set(c for c in (cuts or ()) if 0 < c < len(data)))
    ci = 0
    while pos < len(data):
        end = min(pos + block, len(data))
        while ci < len(cuts) and cuts[ci] <= pos:
            ci += 1
        if ci < len(cuts) and cuts[ci] < end:
            end = cuts[ci]
        out.append(bgzf_block(data[pos:end], level))
        pos = end
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def random_records(rng, n, max_len=300, flags=(0, 0x4, 0x10, 0x14, 0x100, 0x800), lengths=None):
    """[(name, flag, codes, qual)]: all 16 codes, qualities 0..254 (never 0xFF first), l_seq 0, 1, odd and even"""
    recs = []
    for i in range(n):
        L = lengths[i % len(lengths)] if lengths is not None else int(rng.choice([0, 1, 2, 3, int(rng.integers(4, max_len + 1))]))
        codes = rng.integers(0, 16, L, dtype=np.uint8).tobytes()
        qual = rng.integers(0, 255, L, dtype=np.uint8)  # (0..254: 0xFF only where a test asks for it)
        if L and rng.random() < 0.5:
            qual = np.minimum(qual, 60)
        flag = int(flags[int(rng.integers(0, len(flags)))])
        name = b"r%d_%s" % (i, bytes(rng.choice(list(b"ABCxyz:/_0123"), int(rng.integers(1, 20)))))
        recs.append((name, flag, codes, qual.tobytes()))
    return recs


def bam_bytes(records, cuts=None, block=65280, eof=True, hdr=None, level=6, n_cigar=0, tags=b""):
    """the BAM file of `records` and the uncompressed stream's record start offsets"""
    raw = bytearray(header() if hdr is None else hdr)
    starts = []
    for rec in records:
        starts.append(len(raw))
        raw += encode_record(*rec, n_cigar=n_cigar, tags=tags) if len(rec) == 4 else rec[4]
    return bgzf(bytes(raw), cuts=cuts, block=block, eof=eof, level=level), starts, bytes(raw)


def twin_record(name, flag, codes, qual):
    seq = bytes(CODES[c] for c in codes)
    q = bytes(min(v, 93) + 33 for v in qual)
    if flag & 0x10:
        seq = bytes(COMP[c] for c in reversed(codes))
        q = q[::-1]
    return b"@" + name + b"\n" + seq + b"\n+\n" + q + b"\n"


def parse(data):
    """BAM file bytes -> [(index, name, flag, codes, qual)] of every record (skipped ones included); BamError on damage"""
    try:
        raw = gzip.decompress(data)
    except Exception as e:  # noqa: BLE001
        raise BamError("BGZF: %s" % e)
    if raw[:4] != b"BAM\1":
        raise BamError("not BAM")
    (l_text,) = struct.unpack_from("<i", raw, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", raw, p)
    p += 4
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, p)
        p += 4 + ln + 4
    out, i = [], 0
    while p < len(raw):
        if len(raw) - p < 4:
            raise BamError("record %d: truncated" % i)
        (bs,) = struct.unpack_from("<I", raw, p)
        if len(raw) - p - 4 < bs:
            raise BamError("record %d: truncated" % i)
        r = raw[p + 4:p + 4 + bs]
        if bs < 32:
            raise BamError("record %d: block_size" % i)
        l_name, n_cigar, flag, l_seq = r[8], struct.unpack_from("<H", r, 12)[0], struct.unpack_from("<H", r, 14)[0], \
            struct.unpack_from("<i", r, 16)[0]
        if l_name < 1 or l_seq < 0 or 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > bs:
            raise BamError("record %d: block_size" % i)
        name = r[32:32 + l_name].split(b"\0")[0]
        s = 32 + l_name + 4 * n_cigar
        packed = r[s:s + (l_seq + 1) // 2]
        codes = bytes((packed[k >> 1] >> 4) if k % 2 == 0 else (packed[k >> 1] & 15) for k in range(l_seq))
        qual = r[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq]
        out.append((i, name, flag, codes, qual))
        p += 4 + bs
        i += 1
    return out


def twin_records(data):
    """the records of the twin: [(name, flag, codes, qual)] after the skip rule, errors raised"""
    out = []
    for i, name, flag, codes, qual in parse(data):
        if flag & 0x900:
            continue
        if flag & 0x1:
            raise BamError("record %d (%s): paired" % (i, name.decode()))
        if codes and qual[0] == 0xFF:
            raise BamError("record %d (%s): no qualities" % (i, name.decode()))
        out.append((name, flag, codes, qual))
    return out


def bam_to_fastq(data):
    """the FASTQ twin of a BAM file's bytes"""
    return b"".join(twin_record(*r) for r in twin_records(data))


def twin_csr(data):
    """the twin as CSR arrays (bases, qualities, offsets) and the names"""
    recs = twin_records(data)
    seqs, quals = [], []
    for name, flag, codes, qual in recs:
        t = twin_record(name, flag, codes, qual).split(b"\n")
        seqs.append(t[1])
        quals.append(t[3])
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs]) if recs else []
    seq = np.frombuffer(b"".join(seqs), np.uint8).copy()
    qual = np.frombuffer(b"".join(quals), np.uint8).copy()
    return seq, qual, off, [r[0] for r in recs]


def fastq_to_records(text):
    """FASTQ text -> [(name, 0, codes, phred)] (the inverse of the twin for forward records); bases outside the 16 codes -> N"""
    lines = text.split(b"\n")
    look = {c: i for i, c in enumerate(CODES)}
    out = []
    for k in range(0, len(lines) - 3, 4):
        name = lines[k][1:]
        codes = bytes(look.get(c, 15) for c in lines[k + 1])
        qual = bytes(max(0, c - 33) for c in lines[k + 3])
        out.append((name, 0, codes, qual))
    return out


def reverse_record(name, codes, qual):
    """a flag-0x10 record whose twin is the forward read (name, codes, qual)"""
    comp = {i: CODES.index(COMP[i]) for i in range(16)}
    return (name, 0x10, bytes(comp[c] for c in reversed(codes)), bytes(reversed(qual)))
