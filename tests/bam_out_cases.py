"""Test helpers shared by the BAM output tests (tests/test_host_bam_out.py, tests/test_bam_out_emu.py, tests/test_cli_bam_out_stub.py,
tests/test_gpu_bam_out.py): an INDEPENDENT restatement of the output rule (README "BAM output") in plain Python -- the record of a
FASTQ record, the name cut, the cut rule of the deflate blocks -- and the checks every BAM output has to meet.  The judge of a
file is tests/bamio.py (parse, bam_to_fastq) and gzip.decompress per block, never the code under test."""
import re
import struct

from tests import bamio
from tests.bgzf_out_cases import STRIPE, check_blocks

HEADER_TEXT = b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:fastplong_amd\tPN:fastplong_amd\n"
HEADER_RAW = b"BAM\1" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT + struct.pack("<i", 0)
GZ_B, GZ_L = 16384, 1024  # fpl::GZ_B, fpl::GZ_L

# htslib's seq_nt16_table, from the sixteen letters
TABLE = [15] * 256
for _i, _c in enumerate(bamio.CODES):
    TABLE[_c] = _i
    TABLE[ord(chr(_c).lower())] = _i


def cut_name(line):
    """the record's name of a FASTQ name line (the '@' included): cut at the first space or tab, 254 bytes, '*' when empty"""
    return re.split(b"[ \t]", line[1:], maxsplit=1)[0][:254] or b"*"


def fastq_records(text):
    """FASTQ text -> [(name line, bases, qualities)]"""
    lines = text.split(b"\n")
    return [(lines[k], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def record(name_line, seq, qual):
    """the BAM record of one FASTQ record, field by field"""
    name = cut_name(name_line)
    l_seq = len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i, c in enumerate(seq):
        packed[i >> 1] |= TABLE[c] << 4 if i % 2 == 0 else TABLE[c]
    q = bytes(max(c, 33) - 33 for c in qual)
    body = struct.pack("<iiBBHHHiiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, l_seq, -1, -1, 0) + name + b"\0" + bytes(packed) + q
    return struct.pack("<I", len(body)) + body


def records(text):
    return b"".join(record(*r) for r in fastq_records(text))


def cut_text(text):
    """what bam_to_fastq gives for the BAM of `text`: names cut, '+' lines bare, bases as their code's upper-case letter (N for
    what has no code), qualities in 33 .. 126"""
    return b"".join(b"@" + cut_name(n) + b"\n" + bytes(bamio.CODES[TABLE[c]] for c in s) + b"\n+\n" + bytes(min(max(c, 33), 126) for c in q) + b"\n"
                    for n, s, q in fastq_records(text))


def check_fixed_fields(raw):
    """every record of an uncompressed record stream parses and carries the rule's fixed fields -> the number of records"""
    p, n = 0, 0
    while p < len(raw):
        bs, ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<IiiBBHHHiiii", raw, p)
        assert (ref, pos, mapq, bin_, n_cigar, flag, nref, npos, tlen) == (-1, -1, 0, 4680, 0, 4, -1, -1, 0), n
        assert 2 <= l_name <= 255 and raw[p + 36 + l_name - 1] == 0 and 0 not in raw[p + 36:p + 36 + l_name - 1]
        assert bs == 32 + l_name + (l_seq + 1) // 2 + l_seq, n  # no tags
        if l_seq % 2:
            assert raw[p + 36 + l_name + l_seq // 2] & 15 == 0
        p += 4 + bs
        n += 1
    assert p == len(raw)
    return n


def file_bytes(record_blocks, header_block=None):
    """header block + the batches' BGZF blocks + the EOF block"""
    return (bamio.bgzf_block(HEADER_RAW) if header_block is None else header_block) + record_blocks + bamio.EOF_BLOCK


def deflate_blocks(text):
    """how many deflate blocks the layout cuts the records of `text` into: every multiple of GZ_B starts one, and a record with
    l_seq + 1 >= GZ_L starts one at its first byte and one at its first quality byte"""
    starts, o = set(), 0
    for n, s, q in fastq_records(text):
        r = len(record(n, s, q))
        if len(s) + 1 >= GZ_L:
            starts.add(o)
            if len(s):
                starts.add(o + r - len(s))
        o += r
    starts.update(range(0, o, GZ_B))
    return len(starts), o


def check_device_blocks(data, want_records):
    """the device's BGZF blocks of a batch: stripes of 49 152 record bytes that gzip takes one by one, inside the size condition"""
    if not want_records:
        assert data == b""
        return []
    blocks = check_blocks(data, want_records, piece=STRIPE)
    assert all(len(b) <= 65536 for b in blocks)
    return blocks


# ---- the input texts of the cases ----
import numpy as np  # noqa: E402

from tests.bgzf_out_cases import rand_read  # noqa: E402

FRAG_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1022, 1023, 1024]  # the lane's 32-base unit, the forced cut
NAME_TAILS = [b"", b" runid=ab ch=3", b"\tx", b"_" + b"n" * 300]


def lengths_text(extra=0, seed=21):
    """one read per (fragment length, front trim 0..3), extra + trim bases longer than the fragment; names with every kind of tail
    -> (text, [(length, trim)])"""
    rng = np.random.default_rng(seed)
    out, plan = [], []
    for k, fl in enumerate(FRAG_LENGTHS):
        for trim in range(4):
            out.append(rand_read(rng, fl + (trim + extra if extra else 0), b"@L%d.%d%s" % (fl, trim, NAME_TAILS[(k + trim) % 4])))
            plan.append((fl, trim))
    return b"".join(out), plan


def record_len(name_len, fl):
    return 36 + name_len + 1 + (fl + 1) // 2 + fl


def fit_read(rng, left, tag):
    """a read whose record has exactly `left` bytes (left >= 60)"""
    for name_len in range(len(tag), len(tag) + 3):
        fl = (left - 37 - name_len) * 2 // 3
        for f in range(max(fl - 2, 0), fl + 3):
            if record_len(name_len, f) == left:
                return rand_read(rng, f, b"@" + tag + b"x" * (name_len - len(tag)))
    raise AssertionError(left)


def fill_to(rng, out, at, upto, tag=b"f"):
    """append reads of 3 000 bases to `out` until the records of the text have exactly `upto` bytes; at: what they have now"""
    i = 0
    while upto - at > 9000:
        r = rand_read(rng, 3000, b"@%s%d" % (tag, i))
        out.append(r)
        at += record_len(len(tag) + len(b"%d" % i), 3000)
        i += 1
    if upto > at:
        out.append(fit_read(rng, upto - at, tag + b"z"))
    return upto


def exact_records_text(total, seed=22):
    """FASTQ text whose records have exactly `total` bytes"""
    out = []
    fill_to(np.random.default_rng(seed), out, 0, total)
    text = b"".join(out)
    assert len(records(text)) == total
    return text


def straddle_text(seed=23):
    """records whose fixed bytes, name, packed bases (mid byte) and qualities each lie across a multiple of 16 384 and across a
    multiple of 49 152 -> (text, [(record start, part start, part end, the multiple)])"""
    rng = np.random.default_rng(seed)
    name = b"@" + b"straddling_name_of_forty_bytes_in_length"
    assert len(name) == 41
    parts = {"fixed": (0, 36), "name": (36, 76), "packed": (77, 177), "qual": (177, 377)}
    targets = [(16384, "fixed"), (32768, "name"), (65536, "packed"), (81920, "qual"),
               (49152, "fixed"), (98304, "name"), (147456, "packed"), (196608, "qual")]
    out, at, where = [], 0, []
    for k, (t, part) in enumerate(sorted(targets)):
        p0, p1 = parts[part]
        start = t - p0 - (p1 - p0) // 2 - (1 if part == "packed" else 0)
        at = fill_to(rng, out, at, start, b"s%d" % k)
        out.append(rand_read(rng, 200, name))
        where.append((at, at + p0, at + p1, t))
        assert at + p0 < t < at + p1
        at += record_len(40, 200)
    text = b"".join(out)
    assert len(records(text)) == at
    return text, where
