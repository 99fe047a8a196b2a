"""Test helpers of --reindex_comments (README "Comments of a FASTQ input"): a plain-Python model of the rule, written from the rule's
wording and the SAM tags text (section 1.7), not from csrc/fq_comment_rules.h -- which name lines are tags, which reads are
re-indexable, the exact line an output read gets and the five counts -- and the case list the host and CLI tests share,
with the conditions it must meet asserted at the end of this module.  The grammar of an MM value is tests/bam_mod_cases.py's
(parse_mm): the bytes are the same in a BAM field and in a comment.  tests/test_cli_fq_comments_stub.py holds this model against
the BAM side (--comment_tags) once."""
import bisect
import re

import numpy as np

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc

FIELD = re.compile(rb"[A-Za-z][A-Za-z0-9]:(?:[AifZH]:.*|B:[cCsSiIf](?:,.*)?)", re.S)
MN_VALUE = re.compile(rb"[0-9]{1,10}")
ML_VALUE = re.compile(rb"(?:,[0-9]{1,3})*")
MM_TAGS, ML_TAGS, MN_TAGS = (b"MM", b"Mm"), (b"ML", b"Ml"), (b"MN", b"Mn")
COUNTS = ("re-indexed", "lost", "kept", "cut", "left")


# ---- the rule ----
def fields_of(line):
    """the name line without its line end -> (name part, [field]) or (line, None) when it has no TAB (or nothing in front of it)"""
    name, tab, rest = line.partition(b"\t")
    return (name, rest.split(b"\t")) if tab and name else (line, None)


def is_tags(fields):
    return all(FIELD.fullmatch(f) for f in fields)


def positional(f):
    return f[3:4] == b"B" or f[:2] in MM_TAGS + ML_TAGS + MN_TAGS


def occurrences(bases, base):
    if base == b"N":
        return list(range(len(bases)))
    return [i for i, c in enumerate(bases) if c & 0xDF == base[0]]


def why_not(fields, bases, fragment_mode=False):
    """-> (None, (index of MM, of ML, of MN or None, groups)) for a re-indexable read, (a cause, None) for any other; "no fields" when
    it has none of the three tags"""
    at = {t: [k for k, f in enumerate(fields) if f[:2] in t] for t in (MM_TAGS, ML_TAGS, MN_TAGS)}
    mm, ml, mn = at[MM_TAGS], at[ML_TAGS], at[MN_TAGS]
    if not mm + ml + mn:
        return "no fields", None
    if fragment_mode:
        return "run", None
    if len(mm) != 1 or fields[mm[0]][3:4] != b"Z":
        return "MM fields", None
    if len(ml) != 1 or fields[ml[0]][3:6] != b"B:C":
        return "ML fields", None
    if len(mn) > 1:
        return "MN fields", None
    if mn:
        f = fields[mn[0]]
        if f[3:4] != b"i" or not MN_VALUE.fullmatch(f[5:]) or int(f[5:]) != len(bases):
            return "MN value", None
    groups = mc.parse_mm(fields[mm[0]][5:])
    if groups is None:
        return "grammar", None
    n_ml = 0
    for _, base, k, deltas in groups:
        if sum(d + 1 for d, _, _ in deltas) > len(occurrences(bases, base)):
            return "delta sum", None
        n_ml += len(deltas) * k
    value = fields[ml[0]][6:]
    if not ML_VALUE.fullmatch(value):
        return "ML value", None
    if value.count(b",") != n_ml:
        return "ML count", None
    return None, (mm[0], ml[0], mn[0] if mn else None, groups)


def rewrite(fields, bases, s, n, parsed):
    """the fields of the CHANGED output read [s, s + n) of a re-indexable read -> ([field], positions kept, positions cut)"""
    mm, ml, mn, groups = parsed
    value = fields[mm][5:]
    elems = [b"," + e for e in fields[ml][6:].split(b",")[1:]]
    new_mm, new_ml, kept, cut, at = fields[mm][:5], fields[ml][:6], 0, 0, 0
    for header, base, k, deltas in groups:
        occ = occurrences(bases, base)
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
            new_ml += b"".join(elems[at + j0 * k:at + j1 * k])
        new_mm += b";"
        kept, cut, at = kept + len(js), cut + len(deltas) - len(js), at + len(deltas) * k
    out = []
    for i, f in enumerate(fields):
        if i == mm:
            out.append(new_mm)
        elif i == ml:
            out.append(new_ml)
        elif i == mn:
            out.append(f[:5] + b"%d" % n)
        elif not positional(f):
            out.append(f)
    return out, kept, cut


def line_of(line, bases, s, n, changed, prefix=b"", word=None, fragment_mode=False, st=None):
    """the name line of one output read: line, bases: the input read's; [s, s + n): its range; prefix: what the formatter puts behind
    the '@'; word: --failed_out's failure word.  st: the five counts, added to"""
    st = [0] * 5 if st is None else st
    formatted = line[:1] + prefix + line[1:] + (b" " + word if word is not None else b"")
    name, fields = fields_of(line)
    if fields is None:
        return formatted
    if not is_tags(fields):
        st[4] += 1
        return formatted
    head = name[:1] + prefix + name[1:] + (b" " + word if word is not None else b"")
    if not changed:
        return b"\t".join([head] + fields)
    cause, parsed = why_not(fields, bases, fragment_mode)
    if cause is None:
        fields, kept, cut = rewrite(fields, bases, s, n, parsed)
        st[0], st[2], st[3] = st[0] + 1, st[2] + kept, st[3] + cut
    else:
        st[1] += cause != "no fields"
        fields = [f for f in fields if not positional(f)]
    return b"\t".join([head] + fields)


def expected(reads, res, fragment_mode=False, frags=None):
    """reads: [(name line, bases, qualities)], res: one result per read -> (text of --out, text of --failed_out, the five counts of each)"""
    out, failed, so, sf = [], [], [0] * 5, [0] * 5
    assert len(reads) == len(res)

    def one(dst, st, line, seq, q, a, n, changed, prefix=b"", word=None):
        dst.append(line_of(line, seq, a, n, changed, prefix, word, fragment_mode, st) + b"\n" + seq[a:a + n] + b"\n+\n" + q[a:a + n] + b"\n")

    for i, ((line, seq, q), r) in enumerate(zip(reads, res)):
        if r["dropped"]:
            continue
        if fragment_mode:
            mine = frags[frags["read"] == i]
            for fr in mine:
                if fr["code"] == abi.FPL_PASS_FILTER:
                    prefix = (b"r%d-" % fr["break_no"] if fr["break_no"] else b"") + tc.PREFIX[int(fr["kind"])]
                    one(out, so, line, seq, q, int(fr["start"]), int(fr["len"]), True, prefix)
                elif len(mine) == 1:
                    one(failed, sf, line, seq, q, int(r["r1_start"]), int(r["r1_len"]), True, word=abi.FAILED_TYPES[int(fr["code"])].encode())
            continue
        for f in range(int(r["n_frag"])):
            a, n = int(r["frag_start"][f]), int(r["frag_len"][f])
            if r["code"][f] == abi.FPL_PASS_FILTER:
                ch = tc.is_changed(int(r["n_frag"]), int(r["kind"][f]), a, n, len(seq), 0)
                one(out, so, line, seq, q, a, n, ch, tc.PREFIX[int(r["kind"][f])])
            elif r["n_frag"] == 1:
                a, n = int(r["r1_start"]), int(r["r1_len"])
                one(failed, sf, line, seq, q, a, n, tc.is_changed(1, 0, a, n, len(seq), 0), word=abi.FAILED_TYPES[int(r["code"][f])].encode())
    return b"".join(out), b"".join(failed), so, sf


def fastq(reads, crlf=()):
    """the input file; crlf: the names (first word of the line) of the reads written with CRLF line ends"""
    parts = []
    for line, seq, q in reads:
        nl = b"\r\n" if line.split(b"\t")[0] in crlf else b"\n"
        parts += [line, nl, seq, nl, b"+", nl, q, nl]
    return b"".join(parts)


# ---- fields ----
def mm_text(spec, tag=b"MM"):
    """spec: [(header bytes, [delta as int or as the bytes to write])]"""
    return tag + b":Z:" + b"".join(h + b"".join(b"," + (d if isinstance(d, bytes) else b"%d" % d) for d in ds) + b";" for h, ds in spec)


def ml_text(values, tag=b"ML", sub=b"C"):
    return tag + b":B:" + sub + b"".join(b"," + (v if isinstance(v, bytes) else b"%d" % v) for v in values)


def mods(bases, spec, rng, mn=True, values=None):
    """[MM, ML, MN] for the spec, ML values drawn from rng (all three widths of a decimal occur) or `values`, repeated"""
    n = sum(len(ds) * mc.k_of(h) for h, ds in spec)
    values = [int(x) for x in rng.choice(np.array([0, 7, 42, 99, 100, 255]), n)] if values is None else (values * (n // len(values) + 1))[:n]
    return [mm_text(spec), ml_text(values)] + ([b"MN:i:%d" % len(bases)] if mn else [])


def every(bases, base, step, first=0):
    """deltas that mark every step-th occurrence of base, from occurrence `first` on"""
    marks = list(range(first, len(occurrences(bases, base)), step))
    return [m - (marks[i - 1] + 1 if i else 0) for i, m in enumerate(marks)]


def frag(l_seq, s, n, code=abi.FPL_PASS_FILTER):
    """one output read [s, s + n) of a read of l_seq bases (a failed one: --failed_out's trimmed read)"""
    r = tc.result_of("whole", l_seq)
    r["r1_start"], r["r1_len"], r["frag_start"][0], r["frag_len"][0], r["code"][0] = s, n, s, n, code
    return r


def split(l_seq, left, right, right_code=abi.FPL_PASS_FILTER):
    r = tc.result_of("split_both", max(l_seq, 8))
    r["r1_len"] = l_seq
    r["frag_start"][:], r["frag_len"][:] = (left[0], right[0]), (left[1], right[1])
    r["code"][1] = right_code
    return r


WORKED = (b"@r1\tRG:Z:a\tMM:Z:C+m?,1,0,1;\tML:B:C,10,20,30\tMN:i:12", b"ACGCCATCGCTA", 4, 8, b"@r1\tRG:Z:a\tMM:Z:C+m?,0,1;\tML:B:C,20,30\tMN:i:8")
KEPT = [b"RG:Z:run7_grp", b"qs:f:17.25", b"ch:i:407"]
NOT_TAGS = {  # name -> the bytes behind the name part
    "trailing_tab": b"\tRG:Z:a\t", "doubled_tab": b"\tRG:Z:a\t\tqs:i:1", "four_bytes": b"\tRG:Z", "bad_type": b"\tRG:Q:a\tMM:Z:C+m;",
    "b_no_subtype": b"\tmv:B:", "b_bad_subtype": b"\tmv:B:Z,1", "b_no_comma": b"\tmv:B:c1", "bad_tag": b"\t1G:Z:a", "no_colon": b"\tRG-Z:a",
    "only_a_tab": b"\t", "space_comment": b"\trunid=7 ch=3",
}
CRLF = (b"@crlf_front", b"@crlf_split", b"@crlf_whole")
BIG = 12500  # (bases of the read whose name line is longer than 16 384 + 49 152 bytes)


def case_list(seed=53):
    """-> (reads [(name line, bases, qualities)], res, {name: the cause a read is not re-indexable for})"""
    rng = np.random.default_rng(seed)
    reads, res, causes = [], [], {}

    def read(l_seq, lower=False):
        s = rng.choice(np.frombuffer(b"ACGTACGTNM" if not lower else b"acgtACGTnm", np.uint8), l_seq)
        s[:3] = ord("c" if lower else "C")  # (C in front: a front trim always takes occurrences of C away)
        return s.tobytes()

    def add(name, bases, fields, r, cause=None):
        qual = (rng.integers(2, 60, len(bases), dtype=np.uint8) + 33).astype(np.uint8).tobytes()
        line = b"@" + name
        if fields is not None:
            line += (b"".join(b"\t" + f for f in fields) if isinstance(fields, list) else fields)
        reads.append((line, bases, qual))
        res.append(r if not isinstance(r, str) else tc.result_of(r, len(bases)))
        if cause:
            causes[b"@" + name] = cause

    def under_plans(name, bases, fields, plans=("front", "tail", "split_both", "fails_trimmed", "whole"), **kw):
        for plan in plans:
            add(b"%s.%d.%s" % (name, len(bases), plan.encode()), bases, fields, plan, **kw)

    # the worked example
    add(b"r1", WORKED[1], WORKED[0][3:], frag(12, WORKED[2], WORKED[3]))
    # lines that are not tags, and lines without a region
    b40 = read(40)
    for key, rest in NOT_TAGS.items():
        under_plans(key.encode(), b40, rest, ("front", "split_both", "fails_trimmed", "whole"))
    under_plans(b"no_tab", b40, None, ("front", "fails", "split_both"))
    under_plans(b"no_tab space comment", b40, None, ("front",))
    # fields without a modification: kept verbatim, B arrays dropped from changed reads
    under_plans(b"kept_only", b40, KEPT)
    under_plans(b"mv_beside", b40, KEPT[:1] + [b"mv:B:c,5,1,0,1,1,0"] + mods(b40, [(b"C+m?", every(b40, b"C", 2))], rng) + [b"bf:B:f"] + KEPT[1:])
    under_plans(b"empty_z", b40, [b"xz:Z:", b"xa:A:", b"xh:H:"] + mods(b40, [(b"A+a", [0])], rng))
    for l_seq in (1, 41, 77, 1023, 1024, 1025):
        bases = read(l_seq)
        nC = len(occurrences(bases, b"C"))
        spec = [(b"C+m?", every(bases, b"C", 1)), (b"C+mh?", every(bases, b"C", 2)), (b"G-m.", every(bases, b"G", 3)), (b"T+17802", every(bases, b"T", 2)),
                (b"N+n", every(bases, b"N", 5, 2 if l_seq > 2 else 0)), (b"A-a", [])]
        under_plans(b"shapes", bases, KEPT[:1] + mods(bases, spec, rng) + KEPT[1:], *((("front", "split_both", "fails_trimmed"),) if l_seq >= 1023 else ()))
        if l_seq < 41:
            continue
        f3 = mods(bases, spec[1:4], rng)
        under_plans(b"ml_first", bases, [f3[1], KEPT[0], f3[2], f3[0]], ("tail", "split_one_fails", "front"))
        under_plans(b"lower_tags", bases, [f.replace(b"MM:", b"Mm:").replace(b"ML:", b"Ml:").replace(b"MN:", b"Mn:") for f in f3], ("front", "split_both"))
        under_plans(b"no_mn", bases, mods(bases, spec[:2], rng, mn=False) + KEPT[2:], ("front", "split_both", "fails_trimmed"))
        for g in (0, 1, 16):
            under_plans(b"groups_%d" % g, bases, mods(bases, [(b"N+%s?" % bytes([97 + k]), every(bases, b"N", 16, k)) for k in range(g)], rng),
                        ("front", "split_both"))
        ok = [(b"C+m?", every(bases, b"C", 2))]
        n_ok = len(ok[0][1])
        plans = ("front", "split_both", "whole", "fails_trimmed") if l_seq == 41 else ("front",) if l_seq == 1025 else ("tail",) if l_seq == 77 else ()
        bad = {
            b"groups_17": (mods(bases, [(b"N+%s" % bytes([97 + k]), []) for k in range(17)], rng), "grammar"),
            b"two_mm": (mods(bases, ok, rng) + [mm_text(ok)], "MM fields"),
            b"mm_not_z": ([mm_text(ok).replace(b":Z:", b":H:"), ml_text([7] * n_ok)], "MM fields"),
            b"ml_c": ([mm_text(ok), ml_text([7] * n_ok, sub=b"c")] + KEPT, "ML fields"),
            b"ml_missing": ([mm_text(ok), KEPT[0]], "ML fields"),
            b"two_mn": (mods(bases, ok, rng) + [b"Mn:i:%d" % l_seq], "MN fields"),
            b"mn_off": (mods(bases, ok, rng, mn=False) + [b"MN:i:%d" % (l_seq + 1)], "MN value"),
            b"mn_f": (mods(bases, ok, rng, mn=False) + [b"MN:f:%d" % l_seq], "MN value"),
            b"mn_11_digits": (mods(bases, ok, rng, mn=False) + [b"MN:i:%011d" % l_seq], "MN value"),
            b"mn_empty": (mods(bases, ok, rng, mn=False) + [b"MN:i:"], "MN value"),
            b"sum_past": (mods(bases, [(b"C+m", [nC])], rng), "delta sum"),
            b"ten_digits": (mods(bases, [(b"C+m", [b"0000000000"])], rng), "grammar"),
            b"no_semicolon": ([b"MM:Z:C+m,0", ml_text([1])], "grammar"),
            b"lower_base": ([b"MM:Z:c+m,0;", ml_text([1])], "grammar"),
            b"ml_4_digits": ([mm_text(ok), ml_text([b"0255"] + [7] * (n_ok - 1))], "ML value"),
            b"ml_empty_element": ([mm_text(ok), ml_text([b""] + [7] * (n_ok - 1))], "ML value"),
            b"ml_minus": ([mm_text([(b"C+m", [0])]), ml_text([b"-1"])], "ML value"),
            b"ml_one_more": ([mm_text(ok), ml_text([9] * (n_ok + 1))], "ML count"),
            b"ml_one_less": ([mm_text(ok), ml_text([9] * (n_ok - 1))], "ML count"),
        }
        for key, (fields, cause) in bad.items():
            under_plans(key, bases, fields, plans, cause=cause)
        under_plans(b"mn_leading_zeros", bases, mods(bases, ok, rng, mn=False) + [b"MN:i:%010d" % l_seq], ("front", "split_both"))
    # MM values of 0, 63 .. 129 bytes, at every place of the line's 64-byte steps that a short pad reaches; the same for a delta whose
    # digits straddle a step and a 3-digit ML element that does
    b200 = read(200)
    under_plans(b"mm_0", b200, [b"MM:Z:", b"ML:B:C", b"MN:i:200"], ("front", "split_both"))
    for n in (63, 64, 65, 127, 128, 129):
        under_plans(b"mm_%d" % n, b200, mods(b200, mc.mm_of_length(n), rng), ("front", "split_both", "tail"))
    for pad in range(0, 64, 7):
        spec = [(b"N+n?", [b"0"] * 20 + [b"000000002", 1, 0, b"007"]), (b"C+m", [b"01", 2])]
        add(b"straddle.%s" % (b"x" * pad), b200, [b"pd:Z:" + b"y" * pad] + mods(b200, spec, rng, values=[255, 100]), "front")
        add(b"straddle_split.%s" % (b"x" * pad), b200, mods(b200, spec, rng, values=[100, 9, 255]), "split_both")
    # ML with 0 .. 256 elements
    b300 = read(300)
    for n in (0, 1, 15, 16, 17, 255, 256):
        under_plans(b"ml_%d" % n, b300, mods(b300, [(b"N+n", [0] * n)], rng), ("front", "split_both", "tail"))
    # lower-case bases count
    low = read(120, lower=True)
    under_plans(b"lower_bases", low, mods(low, [(b"C+m", every(low, b"C", 1)), (b"A+a", every(low, b"A", 2)), (b"T+t", every(low, b"T", 1))], rng))
    # fragments: on and behind a called base, keeping nothing, keeping a whole group, s = 0, s + n at the read's end
    bases = b"ACGCCATCGCTA" * 4  # (C at 1, 3, 4, 7, 9 of every 12)
    fields = KEPT[:1] + mods(bases, [(b"C+m?", [1, 0, 1, 6]), (b"G+g", [3])], rng)  # C calls on bases 3, 4, 9, 27; the G call on base 20
    for name, r in {
        b"cut_on": frag(48, 4, 30), b"cut_behind": frag(48, 5, 30), b"end_on": frag(48, 0, 10), b"end_behind": frag(48, 0, 9), b"nothing": frag(48, 10, 9),
        b"all_of_c": frag(48, 3, 26), b"only_g": frag(48, 10, 17), b"s_0": frag(48, 0, 40), b"to_the_end": frag(48, 21, 27), b"empty": frag(48, 17, 0),
        b"whole": frag(48, 0, 48), b"failed_trimmed": frag(48, 4, 30, abi.FPL_FAIL_LENGTH), b"failed_whole": frag(48, 0, 48, abi.FPL_FAIL_QUALITY),
        b"split_calls_in_both": split(48, (0, 8), (9, 39)), b"split_right_fails": split(48, (0, 20), (25, 4), abi.FPL_FAIL_LENGTH),
    }.items():
        add(b"frag_" + name, bases, fields, r)
    # CRLF line ends (tests write these reads with them)
    for name, plan in zip(CRLF, ("front", "split_both", "whole")):
        add(name[1:], b40, KEPT[:1] + mods(b40, [(b"C+m?", every(b40, b"C", 1))], rng), plan)
    # one name line longer than 16 384 + 49 152 bytes
    big = read(BIG)
    under_plans(b"big", big, KEPT + mods(big, [(b"N+n", [0] * BIG), (b"A+a?", every(big, b"A", 8))], rng, values=[255, 100, 7]), ("split_both",))
    # 1 100 records
    small = read(30)
    for i in range(1100):
        add(b"many%d" % i, small, mods(small, [(b"C+m", every(small, b"C", 1))], rng), ("front", "whole", "split_both", "fails", "dropped", "tail")[i % 6])
    return reads, np.array(res, np.dtype(abi.RESULT_DTYPE)), causes


def nothing_passes(seed=3):
    """a batch in which no output read passes"""
    reads, res, _ = case_list(seed)
    reads, res = reads[:60], res[:60].copy()
    for i, r in enumerate(res):
        if i % 3 == 0:
            r["dropped"], r["n_frag"] = 1, 0
        else:
            r["code"][:] = abi.FPL_FAIL_QUALITY
    return reads, res


# ---- the conditions the list must meet ----
CAUSES = ("MM fields", "ML fields", "MN fields", "MN value", "grammar", "delta sum", "ML value", "ML count")


def _conditions():
    st = [0] * 5
    assert line_of(WORKED[0], WORKED[1], WORKED[2], WORKED[3], True, st=st) == WORKED[4] and st == [1, 0, 2, 1, 0]
    assert line_of(WORKED[0], WORKED[1], 0, 12, False) == WORKED[0]
    assert line_of(WORKED[0], WORKED[1], 4, 8, True, word=b"failed_too_short") == WORKED[4].replace(b"@r1\t", b"@r1 failed_too_short\t")
    assert line_of(WORKED[0], WORKED[1], 0, 7, True, prefix=b"split-by-adapter-left-") == b"@split-by-adapter-left-r1\tRG:Z:a\tMM:Z:C+m?,1,0;\tML:B:C,10,20\tMN:i:7"
    reads, res, causes = case_list()
    by_name = {r[0].split(b"\t")[0]: r for r in reads}
    seen = set()
    for name, cause in causes.items():
        line, bases, _ = by_name[name]
        assert why_not(fields_of(line)[1], bases)[0] == cause, name
        seen.add(cause)
    assert seen == set(CAUSES)
    for key in NOT_TAGS:
        assert not is_tags(fields_of(by_name[b"@%s.40.front" % key.encode()][0])[1]), key
    out, failed, so, sf = expected(reads, res)
    assert so[0] > 500 and so[1] > 50 and so[2] > 10000 and so[3] > 10000 and so[4] > 20 and sf[0] > 10 and sf[1] > 5 and sf[4] > 5
    assert max(len(r[0]) for r in reads) > 16384 + 49152 and len(reads) > 1100 and sum(len(r[0]) + 2 * len(r[1]) for r in reads) < 640000  # (well under 1 MB)
    assert all(len(a) <= len(b) for a, b in zip(out.split(b"\n")[::4], expected_plain(reads, res)[0].split(b"\n")[::4]))  # (the SIZE argument)
    return True


def expected_plain(reads, res):
    """the formatter's text: the same run without the flag"""
    return expected([(line.replace(b"\t", b" "), s, q) for line, s, q in reads], res)[:2]


CONDITIONS_HOLD = _conditions()
