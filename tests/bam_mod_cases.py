"""Test helpers of --keep_mods (README "BAM output"): two INDEPENDENT plain-Python pieces, written from the SAM tags text
(section 1.7, base modifications) and the rule's wording, not from csrc/bam_mod_rules.h --

  (a) the byte rule: which records are re-indexable and the exact bytes a changed record [s, s + n) gets (rewrite, expected);
  (b) a decoder (decode): a record's fields -> the multiset of (absolute base position, base, strand, code, flag, probability),
      the ordered group headers and MN.  The semantic property (check_semantics): the output's multiset shifted by s equals the
      input's restricted to [s, s + n), the headers are equal, MN is n.

-- and the case list the host and CLI tests share, with the conditions it must meet asserted at the end of this module."""
import bisect
import re
import struct
from collections import Counter

import numpy as np

from fastplong_amd import abi
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio

NIBBLE = {b"A": 1, b"C": 2, b"G": 4, b"T": 8}
INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
MOD_TAGS = (b"MM", b"Mm", b"ML", b"Ml", b"MN", b"Mn")
GROUP = re.compile(rb"([ACGTN])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]{1,9})*);")
DELTA = re.compile(rb",([0-9]+)")


# ---- (a) the byte rule ----
def occurrences(codes, base):
    """the positions of the group's base in the read's 4-bit codes: exact matches, N takes every base"""
    if base == b"N":
        return list(range(len(codes)))
    return [i for i, c in enumerate(codes) if c == NIBBLE[base]]


def parse_mm(value):
    """the MM value without its NUL -> [(header bytes, base, k, [(delta, span start, span end)])], None when not of the grammar"""
    groups, at = [], 0
    while at < len(value):
        m = GROUP.match(value, at)
        if not m:
            return None
        k = len(m.group(3)) if m.group(3).isalpha() else 1
        deltas = [(int(d.group(1)), m.start(5) + d.start(), m.start(5) + d.end()) for d in DELTA.finditer(m.group(5))]
        groups.append((value[m.start():m.start(5)], m.group(1), k, deltas))
        at = m.end()
    return groups if len(groups) <= 16 else None


def why_not(region, codes, flag, fragment_mode=False):
    """-> (None, parsed) for a re-indexable record, (a cause, None) for any other; ("no fields", None) when it has none of the tags"""
    fields, _ = tc.walk(region)
    tagged = [(a, n) for a, n, _ in fields if region[a:a + 2] in MOD_TAGS]
    if not tagged:
        return "no fields", None
    if flag & 0x10:
        return "flag", None
    if fragment_mode:
        return "run", None
    mm = [(a, n) for a, n in tagged if region[a:a + 2] in (b"MM", b"Mm")]
    ml = [(a, n) for a, n in tagged if region[a:a + 2] in (b"ML", b"Ml")]
    mn = [(a, n) for a, n in tagged if region[a:a + 2] in (b"MN", b"Mn")]
    if len(mm) != 1 or region[mm[0][0] + 2:mm[0][0] + 3] != b"Z":
        return "MM fields", None
    if len(ml) != 1 or region[ml[0][0] + 2:ml[0][0] + 4] != b"BC":
        return "ML fields", None
    if len(mn) > 1:
        return "MN fields", None
    if mn:
        t = region[mn[0][0] + 2:mn[0][0] + 3]
        if t not in INT_FMT or struct.unpack_from(INT_FMT[t], region, mn[0][0] + 3)[0] != len(codes):
            return "MN value", None
    value = region[mm[0][0] + 3:mm[0][0] + mm[0][1] - 1]
    groups = parse_mm(value)
    if groups is None:
        return "grammar", None
    n_ml = 0
    for _, base, k, deltas in groups:
        if sum(d + 1 for d, _, _ in deltas) > len(occurrences(codes, base)):
            return "delta sum", None
        n_ml += len(deltas) * k
    if n_ml != struct.unpack_from("<I", region, ml[0][0] + 4)[0]:
        return "ML count", None
    return None, (mm[0], ml[0], mn[0] if mn else None, value, groups)


def rewrite(region, codes, flag, s, n, fragment_mode=False):
    """the tag bytes of the CHANGED output record [s, s + n) -> (bytes, re-indexed?, positions kept, positions cut, lost a field?)"""
    cause, parsed = why_not(region, codes, flag, fragment_mode)
    fields, _ = tc.walk(region)
    if cause:
        return tc.pick(region, True), False, 0, 0, any(pos for _, _, pos in fields)
    mm, ml, mn, value, groups = parsed
    new_mm, new_ml, kept, cut, ml_at = region[mm[0]:mm[0] + 3], b"", 0, 0, ml[0] + 8
    for header, base, k, deltas in groups:
        occ = occurrences(codes, base)
        c0, c1 = bisect.bisect_left(occ, s), bisect.bisect_left(occ, s + n)
        o, js = -1, []
        for j, (d, _, _) in enumerate(deltas):
            o += d + 1
            if c0 <= o < c1:
                js.append((j, o))
        new_mm += header
        if js:
            (j0, o0), j1 = js[0], js[-1][0] + 1
            assert [j for j, _ in js] == list(range(j0, j1))
            new_mm += b",%d" % (o0 - c0) + value[deltas[j0][2]:deltas[j1 - 1][2]]
            new_ml += region[ml_at + j0 * k:ml_at + j1 * k]
        new_mm += b";"
        kept, cut, ml_at = kept + len(js), cut + len(deltas) - len(js), ml_at + len(deltas) * k
    new_mm += b"\0"
    new_ml = region[ml[0]:ml[0] + 4] + struct.pack("<I", len(new_ml)) + new_ml
    out, lost = b"", False
    for a, ln, pos in fields:
        if (a, ln) == mm:
            out += new_mm
        elif (a, ln) == ml:
            out += new_ml
        elif (a, ln) == mn:
            out += region[a:a + 3] + struct.pack(INT_FMT[region[a + 2:a + 3]], n)
        elif not pos:
            out += region[a:a + ln]
        else:
            lost = True
    return out, True, kept, cut, lost


# ---- (b) the decoder ----
def decode(region, codes):
    """-> (Counter of (position, base, strand, code, flag, probability), [group headers], MN or None) of a record's fields"""
    fields, _ = tc.walk(region)
    by_tag = {}
    for a, n, _ in fields:
        by_tag.setdefault(region[a:a + 2].upper(), []).append(region[a:a + n])
    assert len(by_tag.get(b"MM", [])) == 1 and len(by_tag.get(b"ML", [])) == 1
    text = by_tag[b"MM"][0][3:-1].decode()
    probs = by_tag[b"ML"][0]
    assert probs[2:4] == b"BC" and struct.unpack_from("<I", probs, 4)[0] == len(probs) - 8
    probs, at, calls, headers = probs[8:], 0, Counter(), []
    assert text == "" or text.endswith(";")
    for part in text.split(";")[:-1]:
        head, *steps = part.split(",")
        headers.append(head)
        base, strand, rest = head[0], head[1], head[2:]
        how = rest[-1] if rest[-1] in ".?" else ""
        rest = rest[:len(rest) - len(how)]
        names = [rest] if rest.isdigit() else list(rest)
        where = [i for i, c in enumerate(codes) if base == "N" or c == NIBBLE[base.encode()]]
        seen = -1
        for step in steps:
            seen += int(step) + 1
            for name in names:
                calls[(where[seen], base, strand, name, how, probs[at])] += 1
                at += 1
    assert at == len(probs)
    mn = None
    if b"MN" in by_tag:
        assert len(by_tag[b"MN"]) == 1
        f = by_tag[b"MN"][0]
        mn = struct.unpack(INT_FMT[f[2:3]], f[3:])[0]
    return calls, headers, mn


def check_semantics(region, codes, s, n, out_region):
    """the semantic property of a re-indexed record"""
    a, ha, mna = decode(region, codes)
    b, hb, mnb = decode(out_region, codes[s:s + n])
    want, got = Counter(), b
    for (p, *rest), c in a.items():
        if s <= p < s + n:
            want[(p - s, *rest)] += c
    assert got == want, (sorted(got.items())[:5], sorted(want.items())[:5])
    assert ha == hb
    assert (mna is None and mnb is None) or mnb == n
    return sum(b.values())


# ---- the records a run writes ----
def expected(recs, res, mods=True):
    """as tc.expected, with the switch on -> (--out records, --failed_out records, tag stats of each, mod stats of each, and
    [(name, region, codes, s, n, out region)] of every re-indexed record, for the decoder)"""
    out, failed, so, sf, mo, mf, done = [], [], [0] * 4, [0] * 4, [0] * 4, [0] * 4, []
    kept = [r for r in recs if not r[1] & 0x900]
    assert len(kept) == len(res)

    def one(name, flag, codes, region, line, seq, q, a, n, changed, dst, st, ms):
        fields, prefix = tc.walk(region)
        if changed and mods:
            t, re_indexed, k, c, lost = rewrite(region, codes, flag, a, n)
            if re_indexed:
                ms[0], ms[2], ms[3] = ms[0] + 1, ms[2] + k, ms[3] + c
                done.append((name, region, codes, a, n, t))
            elif why_not(region, codes, flag)[0] != "no fields":
                ms[1] += 1
        else:
            t = tc.pick(region, changed)
            lost = changed and any(pos for _, _, pos in fields)
        dst.append(tc.with_tags(bc.record(line, seq[a:a + n], q[a:a + n]), t))
        st[1 if lost else 0] += 1
        st[2] += len(t)
        st[3] += prefix != len(region)

    for (name, flag, codes, qual, enc), r in zip(kept, res):
        if r["dropped"]:
            continue
        region = tc.aux_region(enc)
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        for f in range(int(r["n_frag"])):
            a, n = int(r["frag_start"][f]), int(r["frag_len"][f])
            if r["code"][f] == abi.FPL_PASS_FILTER:
                ch = tc.is_changed(int(r["n_frag"]), int(r["kind"][f]), a, n, len(codes), flag)
                one(name, flag, codes, region, b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq, q, a, n, ch, out, so, mo)
            elif r["n_frag"] == 1:
                a, n = int(r["r1_start"]), int(r["r1_len"])
                one(name, flag, codes, region, b"@" + name, seq, q, a, n, tc.is_changed(1, 0, a, n, len(codes), flag), failed, sf, mf)
    return b"".join(out), b"".join(failed), so, sf, mo, mf, done


# ---- fields ----
def mm_field(groups, tag=b"MM"):
    """groups: [(header bytes, [delta as int or as the bytes to write])]"""
    return tc.zfield(tag, b"".join(h + b"".join(b"," + (d if isinstance(d, bytes) else b"%d" % d) for d in ds) + b";" for h, ds in groups))


def ml_field(values, tag=b"ML", sub=b"C"):
    return tc.barray(tag, sub, values)


def k_of(header):
    rest = header[2:].rstrip(b".?")
    return 1 if rest.isdigit() else len(rest)


def every(codes, base, step, first=0):
    """deltas that mark every step-th occurrence of base, from occurrence `first` on"""
    n = len(occurrences(codes, base))
    marks = list(range(first, n, step))
    return [m - (marks[i - 1] + 1 if i else 0) for i, m in enumerate(marks)]


def fields_of(codes, spec, rng, mn=b"i", tag=(b"MM", b"ML", b"MN"), order="MLN", between=tc.K1):
    """spec: [(header, deltas)] -> the three fields with ML values drawn from rng, in `order`, kept fields around them"""
    n = sum(len(ds) * k_of(h) for h, ds in spec)
    f = {"M": mm_field(spec, tag[0]), "L": ml_field([int(x) for x in rng.integers(0, 256, n)], tag[1]),
         "N": tc.scalar(tag[2], mn, len(codes)) if mn else b""}
    return tc.K2 + f[order[0]] + between + f[order[1]] + f[order[2]] + tc.K3


def mm_of_length(n):
    """an N+n? group whose MM VALUE (without the NUL) has exactly n bytes: ',0' deltas, one of them ',00' where n is even"""
    body = n - 5
    ds = [b"0"] * (body // 2)
    if body % 2:
        ds[len(ds) // 2] = b"00"
    spec = [(b"N+n?", ds)]
    assert len(mm_field(spec)) - 4 == n
    return spec


LENGTHS = (1, 8, 40, 41, 77, 1030)
BIG = 70000
CAUSES = ("flag", "MM fields", "ML fields", "MN value", "grammar", "delta sum", "ML count")


def case_list(seed=47):
    """-> (recs [(name, flag, codes, qual, encoded record)], res, {name: the cause a record is not re-indexable for})"""
    rng = np.random.default_rng(seed)
    recs, res, causes = [], [], {}

    def read(l_seq):
        codes = rng.choice(np.array([1, 2, 4, 8, 1, 2, 4, 8, 15, 3], np.uint8), l_seq)
        codes[:3] = 2  # (C in front: a front trim always takes occurrences of C away)
        return codes.tobytes()

    def add(name, codes, tags, plan, flag=0x4, cause=None):
        qual = rng.integers(2, 60, len(codes), dtype=np.uint8).tobytes()
        recs.append((name, flag, codes, qual, bamio.encode_record(name, flag, codes, qual, tags=tags)))
        res.append(tc.result_of(plan, len(codes)))
        if cause:
            causes[name] = cause

    def under_plans(name, codes, tags, plans=tc.PLANS, **kw):
        for plan in plans:
            add(b"%s.%d.%s" % (name, len(codes), plan.encode()), codes, tags, plan, **kw)

    for l_seq in LENGTHS:
        codes = read(l_seq)
        nC, nG, nT = (len(occurrences(codes, b)) for b in (b"C", b"G", b"T"))
        # every group shape of the grammar in one record: every occurrence, every other one, two codes, a ChEBI id, an empty group
        spec = [(b"C+m?", every(codes, b"C", 1)), (b"C+mh", every(codes, b"C", 2)), (b"G-m.", every(codes, b"G", 3, 1 if nG > 1 else 0)),
                (b"T+17802", every(codes, b"T", 2)), (b"N+n?", every(codes, b"N", 1)), (b"A-a", [])]
        under_plans(b"shapes", codes, fields_of(codes, spec, rng))
        under_plans(b"lower", codes, fields_of(codes, spec[:2], rng, mn=b"C" if l_seq < 256 else b"S", tag=(b"Mm", b"Ml", b"MN")),
                    ("front", "split_both", "fails_trimmed"))
        under_plans(b"ml_first", codes, fields_of(codes, spec[2:5], rng, mn=b"S", order="LNM", tag=(b"MM", b"ML", b"Mn")), ("tail", "split_one_fails", "whole"))
        under_plans(b"no_mn", codes, fields_of(codes, spec[1:4], rng, mn=None, between=tc.P4), ("front", "tail", "split_both"))
        under_plans(b"zero_groups", codes, fields_of(codes, [], rng), ("front", "split_both"))
        under_plans(b"16_groups", codes, fields_of(codes, [(b"N+%s?" % bytes([97 + g]), every(codes, b"N", 16, g)) for g in range(16)], rng),
                    ("front", "tail", "split_both", "fails_trimmed"))
        # all modifications in front of a fragment (the first base only) and all behind one (the last base only)
        under_plans(b"first_base", codes, fields_of(codes, [(b"N+n", [0])], rng), ("front", "split_both", "fails_trimmed"))
        under_plans(b"last_base", codes, fields_of(codes, [(b"N+n.", [l_seq - 1])], rng), ("tail", "split_both", "front"))
        if l_seq >= 77:
            for n in (63, 64, 65, 127, 128, 129):
                under_plans(b"mm_%d" % n, codes, fields_of(codes, mm_of_length(n), rng), ("front", "split_both", "tail"))
            # digits across byte 64 of the value; nine digits, leading zeros; a first delta that loses a digit (C's in front)
            under_plans(b"straddle", codes, fields_of(codes, [(b"N+n?", [b"0"] * 28 + [b"000000002", 1, 0])], rng), ("front", "split_both"))
            under_plans(b"nine_digits", codes, fields_of(codes, [(b"N+n", [b"000000005", b"007", 0, b"00"]), (b"C+m", [b"000000000"])], rng),
                        ("front", "split_both", "tail"))
            assert nC > 12
            under_plans(b"shrinks", codes, fields_of(codes, [(b"C+m?", [10, 0]), (b"N+n", [100 if l_seq > 1000 else 10, 1])], rng),
                        ("front", "fails_trimmed", "split_both"))
        # ---- not re-indexable ----
        ok = [(b"C+m?", every(codes, b"C", 2))]
        n_ok = len(ok[0][1])
        plans = ("front", "split_both", "whole", "fails_trimmed") if l_seq in (41, 1030) else ("tail",)
        bad = {
            b"17_groups": (fields_of(codes, [(b"N+%s" % bytes([97 + g]), []) for g in range(17)], rng), "grammar"),
            b"two_mm": (fields_of(codes, ok, rng) + mm_field(ok), "MM fields"),
            b"ml_S": (tc.K1 + mm_field(ok) + ml_field([7] * n_ok, sub=b"S"), "ML fields"),
            b"mn_off": (mm_field(ok) + ml_field([7] * n_ok) + tc.scalar(b"MN", b"i", l_seq + 1) + tc.K1, "MN value"),
            b"sum_past": (fields_of(codes, [(b"C+m", [nC])], rng), "delta sum"),
            b"ten_digits": (fields_of(codes, [(b"C+m", [b"0000000000"])], rng), "grammar"),
            b"no_semicolon": (tc.zfield(b"MM", b"C+m,0") + ml_field([1]) + tc.K1, "grammar"),
            b"lower_base": (tc.zfield(b"MM", b"c+m,0;") + ml_field([1]), "grammar"),
            b"base_U": (tc.K3 + tc.zfield(b"MM", b"U+m;") + ml_field([]), "grammar"),
            b"ml_one_more": (tc.K2 + mm_field(ok) + ml_field([9] * (n_ok + 1)), "ML count"),
            b"ml_one_less": (mm_field([(b"N+n", [0, 0] if l_seq > 1 else [0])]) + ml_field([9] if l_seq > 1 else []) + tc.K2, "ML count"),
        }
        for key, (tags, cause) in bad.items():
            under_plans(key, codes, tags, plans, cause=cause)
        under_plans(b"reversed", codes, fields_of(codes, ok, rng), plans, flag=0x14, cause="flag")
    # one long read: an A+a? group on every second A, across many 64-byte steps of the value and many 16-byte steps of the bases
    codes = read(BIG)
    under_plans(b"big", codes, fields_of(codes, [(b"A+a?", every(codes, b"A", 2)), (b"N+n", [1000, 60000])], rng), ("front", "split_both", "tail"))
    # a failed read trimmed to nothing: its --failed_out record keeps the headers, no position, MN 0
    codes = read(40)
    add(b"trimmed_to_nothing", codes, fields_of(codes, [(b"C+mh?", every(codes, b"C", 1)), (b"N+n", [0, 5])], rng), "fails")
    res[-1]["r1_start"], res[-1]["r1_len"] = 17, 0
    res[-1]["frag_start"][0], res[-1]["frag_len"][0] = 17, 0
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE)), causes


def malformed_list(seed=5):
    """records whose region does not parse behind the MM field (library-level tests only: the CLI's reader refuses them)"""
    rng = np.random.default_rng(seed)
    recs, res = [], []
    for l_seq, plan in ((40, "front"), (41, "split_both"), (77, "whole"), (77, "fails_trimmed")):
        codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), l_seq).tobytes()
        qual = bytes([30]) * l_seq
        tags = tc.K1 + mm_field([(b"N+n", [0])]) + b"xxQ\1\2\3" + ml_field([5]) + tc.scalar(b"MN", b"i", l_seq)
        name = b"cut_behind_mm.%d.%s" % (l_seq, plan.encode())
        recs.append((name, 0x4, codes, qual, bamio.encode_record(name, 0x4, codes, qual, tags=tags)))
        res.append(tc.result_of(plan, l_seq))
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE))


# ---- the conditions the fixed-plan list must meet ----
def _conditions():
    recs, res, causes = case_list()
    want = expected(recs, res)
    both = 0
    for name, region, codes, s, n, t in want[6]:
        _, _, kept, cut, _ = rewrite(region, codes, 0x4, s, n)
        both += kept > 0 and cut > 0
    assert want[4][0] + want[5][0] >= 40 and both >= 10, (want[4], want[5], both)
    assert want[5][0] >= 5 and want[4][1] >= 10 and want[5][1] >= 1
    by_name = {r[0]: r for r in recs}
    seen = set()
    for name, cause in causes.items():
        _, flag, codes, _, enc = by_name[name]
        assert why_not(tc.aux_region(enc), codes, flag)[0] == cause, name
        seen.add(cause)
    assert seen == set(CAUSES)
    mrecs, _ = malformed_list()
    assert all(why_not(tc.aux_region(r[4]), r[2], r[1])[0] == "ML fields" and tc.walk(tc.aux_region(r[4]))[1] < len(tc.aux_region(r[4])) for r in mrecs)
    return True


CONDITIONS_HOLD = _conditions()
