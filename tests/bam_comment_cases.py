"""Test helpers of --comment_tags (README "Tags as FASTQ comments"): an INDEPENDENT plain-Python model of the rule -- which fields an
output read's comment is made from, the SAM text of a field, where the comment goes, what is left out, the counters -- and the case
list the host, emulator and GPU tests share.  Written from the rule's wording, not from csrc/bam_comment_rules.h: the tag bytes
come from tests/bam_tag_cases.pick and tests/bam_mod_cases.rewrite, the float text from Python's '%g' with an explicit -nan."""
import math
import struct

import numpy as np

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc
from tests import bamio

INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
SIZE = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


# ---- the rule ----
def float_text(raw):
    """the bytes of C's printf("%g", (double)v) for the float in raw"""
    v = struct.unpack("<f", raw)[0]
    if math.isnan(v):
        return b"-nan" if raw[3] & 0x80 else b"nan"
    return b"%g" % v


def value_text(t, raw):
    return float_text(raw) if t == b"f" else b"%d" % struct.unpack(INT_FMT[t], raw)[0]


def has_control(value):
    return any(c < 0x20 or c == 0x7F for c in value)


def field_text(field):
    """the text of one field (its bytes, tag first), the tab in front included; None: left out for control bytes"""
    tag, t, value = field[:2], field[2:3], field[3:]
    if t == b"A":
        return None if has_control(value) else b"\t" + tag + b":A:" + value
    if t in (b"Z", b"H"):
        assert value.endswith(b"\0")
        return None if has_control(value[:-1]) else b"\t" + tag + b":" + t + b":" + value[:-1]
    if t == b"B":
        sub, n = value[:1], struct.unpack_from("<I", value, 1)[0]
        w = SIZE[sub]
        assert len(value) == 5 + n * w
        return b"\t" + tag + b":B:" + sub + b"".join(b"," + value_text(sub, value[5 + k * w:5 + (k + 1) * w]) for k in range(n))
    return b"\t" + tag + (b":f:" if t == b"f" else b":i:") + value_text(t, value)


def is_selected(sel, tag):
    return sel == "*" or (sel is not None and tag in sel)


def comment(tag_bytes, sel):
    """the comment of a record's tag bytes under a selection (None: off, "*": every field, a list of two-byte tags)
    -> (text, fields written, fields left out)"""
    fields, prefix = tc.walk(tag_bytes)
    assert prefix == len(tag_bytes)  # (the rules only ever give fields that parse)
    out, n, left = b"", 0, 0
    for a, ln, _ in fields:
        if not is_selected(sel, tag_bytes[a:a + 2]):
            continue
        t = field_text(tag_bytes[a:a + ln])
        if t is None:
            left += 1
        else:
            out, n = out + t, n + 1
    return out, n, left


def tag_bytes_of(region, codes, flag, s, n, changed, fragment_mode=False):
    """the auxiliary fields the same run's .bam record would carry under --keep_tags --keep_mods"""
    if not changed:
        return tc.pick(region, False)
    return mc.rewrite(region, codes, flag, s, n, fragment_mode)[0]


def note(stats, text, n, left):
    stats[0] += n > 0
    stats[1] += n
    stats[2] += len(text)
    stats[3] += left


def expected(recs, res, sel, fragment_mode=False, frags=None):
    """recs: [(name, flag, codes, qual, encoded record)] as written to the input, res: one result per record the reader does not skip
    -> (text of --out, text of --failed_out, the four counts of each)"""
    out, failed, so, sf = [], [], [0] * 4, [0] * 4
    kept = [r for r in recs if not r[1] & 0x900]
    assert len(kept) == len(res)

    def one(dst, st, line, seq, q, a, n, tags):
        c, k, left = comment(tags, sel)
        note(st, c, k, left)
        dst.append(line + c + b"\n" + seq[a:a + n] + b"\n+\n" + q[a:a + n] + b"\n")

    for i, ((name, flag, codes, qual, enc), r) in enumerate(zip(kept, res)):
        if r["dropped"]:
            continue
        region = tc.aux_region(enc)
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        if fragment_mode:
            mine = frags[frags["read"] == i]
            for fr in mine:
                a, n = int(fr["start"]), int(fr["len"])
                if fr["code"] == abi.FPL_PASS_FILTER:
                    line = b"@" + (b"r%d-" % fr["break_no"] if fr["break_no"] else b"") + tc.PREFIX[int(fr["kind"])] + name
                    one(out, so, line, seq, q, a, n, tag_bytes_of(region, codes, flag, a, n, True, True))
                elif len(mine) == 1:
                    a, n = int(r["r1_start"]), int(r["r1_len"])
                    one(failed, sf, b"@" + name + b" " + abi.FAILED_TYPES[int(fr["code"])].encode(), seq, q, a, n,
                        tag_bytes_of(region, codes, flag, a, n, True, True))
            continue
        for f in range(int(r["n_frag"])):
            a, n = int(r["frag_start"][f]), int(r["frag_len"][f])
            if r["code"][f] == abi.FPL_PASS_FILTER:
                ch = tc.is_changed(int(r["n_frag"]), int(r["kind"][f]), a, n, len(codes), flag)
                one(out, so, b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq, q, a, n, tag_bytes_of(region, codes, flag, a, n, ch))
            elif r["n_frag"] == 1:
                a, n = int(r["r1_start"]), int(r["r1_len"])
                ch = tc.is_changed(1, 0, a, n, len(codes), flag)
                one(failed, sf, b"@" + name + b" " + abi.FAILED_TYPES[int(r["code"][f])].encode(), seq, q, a, n,
                    tag_bytes_of(region, codes, flag, a, n, ch))
    return b"".join(out), b"".join(failed), so, sf


# ---- fields ----
def float_bits(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


FLT_MAX = float_bits(0x7F7FFFFF)
# (value, the text the libc gives): the issue's examples, checked by the model below
FLOAT_EXAMPLES = [(100000.5, b"100000"), (100001.5, b"100002"), (999999.5, b"1e+06"), (2.0 ** -149, b"1.4013e-45"), (FLT_MAX, b"3.40282e+38"),
                  (-0.0, b"-0")]
FLOATS = [0.0, -0.0, 17.25, 100000.5, 100001.5, 999999.5, 1e-5, 1e-4, 2.0 ** -149, FLT_MAX, math.inf, -math.inf]
NAN_BITS = (0x7FC00000, 0xFFC00000)
ARRAY_COUNTS = (0, 1, 63, 64, 65, 128, 4097)
EXTREMES = {b"c": (-128, 127), b"C": (0, 255), b"s": (-32768, 32767), b"S": (0, 65535), b"i": (-2147483648, 2147483647), b"I": (0, 4294967295)}


def ffield(tag, bits):
    return tag + b"f" + struct.pack("<I", bits)


def float_fields():
    out = b""
    for k, v in enumerate(FLOATS):
        out += tc.scalar(b"f%s" % bytes([65 + k]), b"f", v)
    return out + ffield(b"n0", NAN_BITS[0]) + ffield(b"n1", NAN_BITS[1])


def array_values(sub, n, rng):
    if sub == b"f":
        pool = FLOATS + [float_bits(int(b)) for b in rng.integers(0, 0x7F800000, 40)]
        return [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    lo, hi = EXTREMES[sub]
    v = [int(x) for x in rng.integers(lo, hi + 1, n)]
    if n:  # (the extremes are among them: the widest text first and last)
        v[0], v[-1] = hi, lo
    return v


def integer_fields():
    out = b""
    for k, (t, (lo, hi)) in enumerate(sorted(EXTREMES.items())):
        out += tc.scalar(b"l%d" % k, t, lo) + tc.scalar(b"h%d" % k, t, hi)
    return out


REGIONS = {
    "integers": integer_fields(),
    "floats": float_fields(),
    "z_empty": tc.K3 + tc.zfield(b"ze", b"") + tc.K1,
    "z_tab": tc.K1 + tc.zfield(b"zt", b"a\tb") + tc.K3,
    "z_newline": tc.zfield(b"zn", b"line\nbreak") + tc.K2,
    "z_del_and_a_ctl": tc.zfield(b"zd", b"x\x7f") + tc.scalar(b"ac", b"A", b"\x1f") + tc.scalar(b"ok", b"A", b"~") + tc.zfield(b"hc", b"0A\x01", b"H"),
    "h_field": tc.K2 + tc.zfield(b"hx", b"1AE301", b"H") + tc.K3,
    "first_and_last": tc.scalar(b"fi", b"C", 7) + tc.K1 + tc.K2 + tc.zfield(b"la", b"the last field"),
}
# selections: every field; the modification fields; nothing; only the first field of "first_and_last"; only its last; 32 tags
TAGS_32 = [b"MM", b"ML", b"MN", b"qs", b"RG", b"ch", b"mv", b"xA", b"xc", b"xC", b"xs", b"xS", b"xi", b"xI", b"xf", b"zt", b"zn", b"ze", b"hx", b"fA",
           b"fB", b"n0", b"n1", b"l0", b"h5", b"bc", b"bf", b"st", b"Mm", b"Ml", b"zz", b"zh"]
SELECTIONS = {"all": "*", "mods": [b"MM", b"ML"], "nothing": [b"Zq", b"mm"], "first": [b"fi"], "last": [b"la"], "32": TAGS_32}
assert len(TAGS_32) == len(set(TAGS_32)) == 32


def selection_args(sel):
    """-> (tag bytes, n_tags) as the C calls take a selection"""
    if sel is None:
        return b"", 0
    if sel == "*":
        return b"", -1
    return b"".join(sel), len(sel)


def case_list(long_ml=True, seed=77):
    """-> (recs, res): the lists of --keep_mods and --keep_tags (regions that do not parse included), then records that hold every
    integer type at its extremes, the floats, B arrays of every subtype and count, Z with control bytes, an H field, one ML of 20 000
    values (its comment passes a 16 384-byte deflate cut and a 49 152-byte stripe), flag 0x10"""
    rng = np.random.default_rng(seed)
    recs, res = [], []
    for lst in (mc.case_list()[:2], tc.case_list(malformed=True), mc.malformed_list()):
        recs += lst[0]
        res += list(lst[1])

    def add(name, tags, l_seq, plan, flag=0x4, codes=None):
        codes = rng.integers(1, 16, l_seq, dtype=np.uint8).tobytes() if codes is None else codes
        qual = rng.integers(2, 60, l_seq, dtype=np.uint8).tobytes()
        recs.append((name, flag, codes, qual, bamio.encode_record(name, flag, codes, qual, tags=tags)))
        res.append(tc.result_of(plan, l_seq))

    k = 0
    for key in sorted(REGIONS):
        for plan in tc.PLANS[k % 3::3] + ("whole",):
            add(b"c.%s.%s" % (key.encode(), plan.encode()), REGIONS[key], [41, 40, 77][k % 3], plan)
            k += 1
    for sub in sorted(tc.SUBTYPE):
        for n in ARRAY_COUNTS:
            tags = tc.K1 + tc.barray(b"b" + sub, sub, array_values(sub, n, rng)) + tc.K3
            for plan in ("whole", "front") if n != 4097 else ("whole",):  # (a changed record drops a B array: "front" shows that)
                add(b"arr.%s.%d.%s" % (sub, n, plan.encode()), tags, 33 + n % 7, plan)
    for plan in ("whole", "split_both", "fails_trimmed"):
        add(b"rev.%s" % plan.encode(), REGIONS["floats"] + tc.P1 + tc.P2, 52, plan, flag=0x14)
    if long_ml:
        # one ML of 20 000 values on a read that passes whole (the text of the verbatim field) and on one that is trimmed (the
        # re-indexed field): an N+n group on every base
        for plan in ("whole", "front"):
            codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), 20000).tobytes()
            add(b"long_ml.%s" % plan.encode(), mc.fields_of(codes, [(b"N+n?", [0] * 20000)], rng), 20000, plan, codes=codes)
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE))


def bound_holds(recs):
    """the 5x bound, for every record of a list: the comment of its whole parsed prefix under "*" against its region's bytes"""
    for r in recs:
        region = tc.aux_region(r[4])
        text = comment(tc.pick(region, False), "*")[0]
        assert len(text) <= 5 * len(region), r[0]
    return True


# ---- the model against the issue's examples ----
for _v, _t in FLOAT_EXAMPLES:
    assert float_text(struct.pack("<f", _v)) == _t, (_v, _t)
assert float_text(struct.pack("<I", 0xFFC00000)) == b"-nan" and float_text(struct.pack("<I", 0x7FC00000)) == b"nan"
assert field_text(tc.barray(b"xb", b"C", [])) == b"\txb:B:C" and field_text(tc.barray(b"xb", b"c", [-128, 5])) == b"\txb:B:c,-128,5"
assert field_text(tc.scalar(b"xA", b"A", b"Q")) == b"\txA:A:Q" and field_text(tc.zfield(b"zt", b"a\tb")) is None
assert max(len(float_text(struct.pack("<f", v))) for v in (-FLT_MAX, -1.23456e-4, -2.0 ** -149)) == 12
