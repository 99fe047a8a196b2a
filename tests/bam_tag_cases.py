"""Test helpers of --keep_tags (README "BAM output"): an INDEPENDENT restatement of the tag rule in plain Python -- the walk of
an aux region, the positional set, the changed test, the header with @RG lines, the records an input BAM and its per-read results
give -- and the case list the host, emulator and GPU tests share.  Written from the rule's text, not from csrc/bam_tag_rules.h."""
import struct

import numpy as np

from fastplong_amd import abi
from tests import bam_out_cases as bc
from tests import bamio

SCALAR = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
SUBTYPE = {k: v for k, v in SCALAR.items() if k != b"A"}
POSITIONAL_TAGS = (b"MM", b"Mm", b"ML", b"Ml", b"MN")
PREFIX = {0: b"", 1: b"split-by-adapter-left-", 2: b"split-by-adapter-right-"}


# ---- the rule ----
def field_len(region, at):
    """bytes of the field at region[at:], 0 when it does not parse"""
    left = len(region) - at
    if left < 3:
        return 0
    t = region[at + 2:at + 3]
    if t in SCALAR:
        n = 3 + SCALAR[t]
    elif t in (b"Z", b"H"):
        z = region.find(b"\0", at + 3)
        if z < 0:
            return 0
        n = z + 1 - at
    elif t == b"B":
        if left < 8 or region[at + 3:at + 4] not in SUBTYPE:
            return 0
        n = 8 + struct.unpack_from("<I", region, at + 4)[0] * SUBTYPE[region[at + 3:at + 4]]
    else:
        return 0
    return n if n <= left else 0


def walk(region):
    """-> ([(start, length, positional)] of the parsed prefix, its length)"""
    fields, at = [], 0
    while at < len(region):
        n = field_len(region, at)
        if not n:
            break
        fields.append((at, n, region[at + 2:at + 3] == b"B" or region[at:at + 2] in POSITIONAL_TAGS))
        at += n
    return fields, at


def pick(region, changed):
    """what an output record gets of its input record's region"""
    fields, prefix = walk(region)
    if not changed:
        return region[:prefix]
    return b"".join(region[a:a + n] for a, n, pos in fields if not pos)


def is_changed(n_frag, kind, start, length, l_seq, flag, fragment_mode=False):
    return not (n_frag == 1 and kind == 0 and start == 0 and length == l_seq and not flag & 0x10 and not fragment_mode)


def aux_region(rec):
    """the aux region of one encoded record (block_size included)"""
    bs, l_name, n_cigar, l_seq = struct.unpack_from("<I", rec)[0], rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    return rec[36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:4 + bs]


def read_group_lines(text):
    text = text.split(b"\0", 1)[0]
    lines = [l for l in text.splitlines(keepends=True) if l.startswith(b"@RG\t")]
    if lines and not lines[-1].endswith(b"\n"):
        lines[-1] += b"\n"
    return b"".join(lines)


def header_raw(input_header_text=b""):
    hd, pg = bc.HEADER_TEXT.split(b"\n")[0] + b"\n", bc.HEADER_TEXT.split(b"\n")[1] + b"\n"
    text = hd + read_group_lines(input_header_text) + pg
    return b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)


def with_tags(record, tags):
    """an output record of the no-tag rule with `tags` behind its qualities"""
    return struct.pack("<I", struct.unpack_from("<I", record)[0] + len(tags)) + record[4:] + tags


class Stats:
    def __init__(self):
        self.v = [0, 0, 0, 0]

    def note(self, region, changed, wrote):
        fields, prefix = walk(region)
        lost = changed and any(pos for _, _, pos in fields)
        self.v[1 if lost else 0] += 1
        self.v[2] += len(wrote)
        self.v[3] += prefix != len(region)


def expected(recs, res, fragment_mode=False, frags=None):
    """recs: [(name, flag, codes, qual, encoded record)] as written to the input, res: one result per record the reader does not skip
    -> (records of --out, records of --failed_out, Stats of each)"""
    out, failed, so, sf = [], [], Stats(), Stats()
    kept = [r for r in recs if not r[1] & 0x900]
    assert len(kept) == len(res)
    for i, ((name, flag, codes, qual, enc), r) in enumerate(zip(kept, res)):
        if r["dropped"]:
            continue
        region = aux_region(enc)
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        if fragment_mode:
            mine = frags[frags["read"] == i]
            for fr in mine:
                a, n = int(fr["start"]), int(fr["len"])
                if fr["code"] == abi.FPL_PASS_FILTER:
                    line = b"@" + (b"r%d-" % fr["break_no"] if fr["break_no"] else b"") + PREFIX[int(fr["kind"])] + name
                    t = pick(region, True)
                    out.append(with_tags(bc.record(line, seq[a:a + n], q[a:a + n]), t))
                    so.note(region, True, t)
                elif len(mine) == 1:
                    a, n = int(r["r1_start"]), int(r["r1_len"])
                    t = pick(region, True)
                    failed.append(with_tags(bc.record(b"@" + name, seq[a:a + n], q[a:a + n]), t))
                    sf.note(region, True, t)
            continue
        for f in range(int(r["n_frag"])):
            a, n = int(r["frag_start"][f]), int(r["frag_len"][f])
            if r["code"][f] == abi.FPL_PASS_FILTER:
                ch = is_changed(int(r["n_frag"]), int(r["kind"][f]), a, n, len(codes), flag)
                t = pick(region, ch)
                out.append(with_tags(bc.record(b"@" + PREFIX[int(r["kind"][f])] + name, seq[a:a + n], q[a:a + n]), t))
                so.note(region, ch, t)
            elif r["n_frag"] == 1:
                a, n = int(r["r1_start"]), int(r["r1_len"])
                ch = is_changed(1, 0, a, n, len(codes), flag)
                t = pick(region, ch)
                failed.append(with_tags(bc.record(b"@" + name, seq[a:a + n], q[a:a + n]), t))
                sf.note(region, ch, t)
    return b"".join(out), b"".join(failed), so.v, sf.v


# ---- fields ----
FMT = {b"A": "c", b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I", b"f": "f"}


def scalar(tag, t, v):
    return tag + t + struct.pack("<" + FMT[t], v)


def zfield(tag, s, t=b"Z"):
    return tag + t + s + b"\0"


def barray(tag, sub, values):
    return tag + b"B" + sub + struct.pack("<I", len(values)) + b"".join(struct.pack("<" + FMT[sub], v) for v in values)


def region_of_length(n, k):
    """a region of exactly n bytes that parses (n == 0 or n >= 4); every other one (k odd) has a B array in front of a kept field"""
    if n == 0:
        return b""
    assert n >= 4
    if k % 2 and n >= 12:
        return barray(b"mv", b"C", [(3 * j + k) & 255 for j in range(n - 12)]) + scalar(b"xA", b"A", b"q")
    return zfield(b"st", bytes(65 + (j + k) % 26 for j in range(n - 4)))


K1 = scalar(b"qs", b"f", 17.25)
K2 = zfield(b"RG", b"run7_grp")
K3 = scalar(b"ch", b"S", 407)
P1 = zfield(b"MM", b"C+m,5,12,0;")
P2 = barray(b"ML", b"C", [200, 13, 255])
P3 = scalar(b"MN", b"i", 120)
P4 = barray(b"mv", b"c", [5, 1, 0, 1, 1, 0])

# name -> the aux bytes of one record; all of them parse
REGIONS = {
    "none": b"",
    "scalars": (scalar(b"xA", b"A", b"Z") + scalar(b"xc", b"c", -7) + scalar(b"xC", b"C", 250) + scalar(b"xs", b"s", -3000) +
                scalar(b"xS", b"S", 65000) + scalar(b"xi", b"i", -2 ** 31) + scalar(b"xI", b"I", 2 ** 32 - 1) + scalar(b"xf", b"f", 0.5)),
    "mods": K2 + P1 + P2 + P3,
    "mods_lower": zfield(b"Mm", b"C+m,1;") + barray(b"Ml", b"C", [9]) + K1,
    "pos_first": P4 + K1 + K2,
    "pos_last": K1 + K2 + P4,
    "pos_middle": K1 + P2 + K2,
    "alternating": P1 + K1 + P2 + K2 + K3 + P3 + K1 + K2 + K3 + P4,  # kept runs of 1, 2 and 3
    "only_positional": P1 + P2 + P3 + P4,
    "mm_like_kept": zfield(b"MX", b"not positional") + scalar(b"mN", b"i", 5),  # (neither tag is in the positional set)
    "mv_50000": K2 + barray(b"mv", b"c", [(j * 7) % 3 for j in range(50000)]) + K1,
    "mv_100000": barray(b"mv", b"c", [(j * 5) % 3 for j in range(100000)]) + K3,
}
for _t in (b"Z", b"H"):
    for _n in (0, 7, 8, 9, 300):
        REGIONS["%s_%d" % (_t.decode(), _n)] = K3 + zfield(b"z" + _t.lower(), (b"0123456789ABCDEF" * 20)[:_n], _t) + K1
for _s in sorted(SUBTYPE):
    for _n in (0, 1, 1000):
        _v = [0.25 * j for j in range(_n)] if _s == b"f" else [j % 100 for j in range(_n)]
        REGIONS["B%s_%d" % (_s.decode(), _n)] = K1 + barray(b"b" + _s, _s, _v) + K3
for _k, _n in enumerate([0, *range(4, 66), 1023, 1024, 1025, 16383, 16384, 16385]):
    REGIONS["len_%d" % _n] = region_of_length(_n, _k)

# regions that do NOT parse to their end (library-level tests only: the CLI's reader refuses them) -> the parsed prefix
MALFORMED = {
    "ends_1_into_a_field": (K1 + K2[:1], len(K1)),
    "ends_2_into_a_field": (K1 + K2[:2], len(K1)),
    "value_cut": (K2 + K1[:-1], len(K2)),
    "unknown_type": (K1 + b"xxQ\1\2\3\4" + K2, len(K1)),
    "unknown_subtype": (K3 + b"bxBZ" + struct.pack("<I", 1) + b"\0" + K1, len(K3)),
    "z_without_nul": (K1 + P2 + b"zzZabcdefghijklmnopq", len(K1 + P2)),
    "b_count_past_the_end": (K2 + b"bcBc" + struct.pack("<I", 100) + b"\1" * 50, len(K2)),
    "b_count_ffffffff": (P1 + K3 + b"biBi" + struct.pack("<I", 0xFFFFFFFF) + b"\1" * 64, len(P1 + K3)),
    "b_header_cut": (K1 + b"bsBs\1\0", len(K1)),
    "first_field_bad": (b"a", 0),
}

PLANS = ("whole", "front", "tail", "split_both", "split_one_fails", "fails", "fails_trimmed", "dropped")


def result_of(plan, l_seq):
    """one fpl_read_result of the plan for a read of l_seq bases (a read too short for the plan passes whole)"""
    r = np.zeros(1, np.dtype(abi.RESULT_DTYPE))[0]
    r["n_frag"], r["r1_start"], r["r1_len"] = 1, 0, l_seq
    r["frag_start"][0], r["frag_len"][0], r["code"][0] = 0, l_seq, abi.FPL_PASS_FILTER
    if l_seq < 8 and plan not in ("whole", "fails", "dropped"):
        plan = "whole"
    if plan == "front":
        r["r1_start"], r["r1_len"] = 3, l_seq - 3
        r["frag_start"][0], r["frag_len"][0] = 3, l_seq - 3
    elif plan == "tail":
        r["r1_len"] = l_seq - 2
        r["frag_len"][0] = l_seq - 2
    elif plan in ("split_both", "split_one_fails"):
        h = l_seq // 2
        r["n_frag"] = 2
        r["frag_start"][:] = (0, h + 1)
        r["frag_len"][:] = (h - 1, l_seq - h - 1)
        r["kind"][:] = (1, 2)
        r["code"][1] = abi.FPL_FAIL_LENGTH if plan == "split_one_fails" else abi.FPL_PASS_FILTER
    elif plan == "fails":
        r["code"][0] = abi.FPL_FAIL_QUALITY
    elif plan == "fails_trimmed":
        r["code"][0] = abi.FPL_FAIL_LENGTH
        r["r1_start"], r["r1_len"] = 1, l_seq - 4
        r["frag_start"][0], r["frag_len"][0] = 1, l_seq - 4
    elif plan == "dropped":
        r["dropped"], r["n_frag"] = 1, 0
    return r


def case_list(malformed=False, seed=31):
    """the case list: -> (recs [(name, flag, codes, qual, encoded record)], res (one per record that is not skipped)).
    Every region of REGIONS under plans that rotate, so that every kind of region meets whole, trimmed, split and failed reads;
    l_seq 0, odd and even; n_cigar 2; flag 0x10; skipped records with tags between kept ones.  malformed: MALFORMED's too."""
    rng = np.random.default_rng(seed)
    recs, res = [], []

    def add(name, tags, l_seq, plan, flag=0x4, n_cigar=0):
        codes = rng.integers(1, 16, l_seq, dtype=np.uint8).tobytes()
        qual = rng.integers(2, 60, l_seq, dtype=np.uint8).tobytes()
        recs.append((name, flag, codes, qual, bamio.encode_record(name, flag, codes, qual, n_cigar=n_cigar, tags=tags)))
        if not flag & 0x900:
            res.append(result_of(plan, l_seq))

    k = 0
    for key in sorted(REGIONS):
        big = len(REGIONS[key]) > 20000
        for plan in (("whole", "split_both") if big else PLANS[k % 3::3] + ("whole",)):
            add(b"%s.%s" % (key.encode(), plan.encode()), REGIONS[key], [41, 40, 1030, 77][k % 4], plan)
            k += 1
        if k % 5 == 0:
            add(b"skipped%d" % k, K1 + P1, 30, "whole", flag=0x100 if k % 2 else 0x800)
    for plan in PLANS:
        add(b"alt.%s" % plan.encode(), REGIONS["alternating"], 64, plan)
        add(b"rev.%s" % plan.encode(), REGIONS["mods"], 65, plan, flag=0x10)
        add(b"cigar.%s" % plan.encode(), REGIONS["pos_middle"], 33, plan, n_cigar=2)
    add(b"empty_read", REGIONS["mods"], 0, "whole")
    add(b"empty_read_fails", REGIONS["alternating"], 0, "fails")
    add(b"one_base", REGIONS["pos_last"], 1, "whole")
    if malformed:
        for j, key in enumerate(sorted(MALFORMED)):
            for plan in ("whole", "front", "split_both"):
                add(b"bad.%s.%s" % (key.encode(), plan.encode()), MALFORMED[key][0], 52 + j % 2, plan)
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE))


def input_bam(recs, header_text=None, block=65280):
    """the input file's bytes"""
    hdr = None if header_text is None else bamio.header(text=header_text)
    raw = bytearray(bamio.header() if hdr is None else hdr)
    for r in recs:
        raw += r[4]
    return bamio.bgzf(bytes(raw), block=block)


RG_HEADER = (b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:run7_grp\tPL:ONT\tSM:s1\n@PG\tID:basecaller\tPN:dorado\n@CO\t@RG\tnot a line start\n"
             b"@RG\tID:second\tDS:basecall_model=x\n@SQ\tSN:none\tLN:1\n")
