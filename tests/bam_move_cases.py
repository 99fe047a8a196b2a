"""Test helpers of --keep_moves (README "BAM output"): three plain-Python pieces, written from the rule's wording and not from
csrc/bam_move_rules.h --

  (a) the byte rule: which records are move-re-indexable and the exact bytes a changed record [s, s + n) gets in the places of mv
      and ts (why_not, cut), composed with --keep_mods' rule of tests/bam_mod_cases.py (tags_of, expected);
  (b) a decoder (spans): table + ts -> the span [first, end) of every base in absolute sample units.  The semantic property
      (check_semantics): base j of the output record [s, s + n) has the span of the input's base s + j, the stride is unchanged;
  (c) the case list the host, emulator and GPU tests share, with the conditions it must meet asserted at the end of this module."""
import struct

import numpy as np

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio

INT_FMT = mc.INT_FMT
INT_MAX = {b"c": 127, b"C": 255, b"s": 32767, b"S": 65535, b"i": 2 ** 31 - 1, b"I": 2 ** 32 - 1}
STEP = 64 * 16  # moves a wave takes in a step, 16 bytes a lane


# ---- (a) the byte rule ----
def why_not(region, l_seq, flag, fragment_mode=False):
    """-> (None, (mv field, ts field or None, stride, moves, ts or None)) for a move-re-indexable record, (a cause, None) for any
    other; ("no table", None) when no field is tagged mv"""
    fields, _ = tc.walk(region)
    mv = [(a, n) for a, n, _ in fields if region[a:a + 2] == b"mv"]
    ts = [(a, n) for a, n, _ in fields if region[a:a + 2] == b"ts"]
    if not mv:
        return "no table", None
    if flag & 0x10:
        return "flag", None
    if fragment_mode:
        return "run", None
    if len(mv) != 1:
        return "mv fields", None
    a, n = mv[0]
    if region[a + 2:a + 3] != b"B" or region[a + 3:a + 4] not in (b"c", b"C"):
        return "subtype", None
    if struct.unpack_from("<I", region, a + 4)[0] < 1:
        return "count", None
    el = np.frombuffer(region[a + 8:a + n], np.int8 if region[a + 3:a + 4] == b"c" else np.uint8).astype(np.int64)
    stride, moves = int(el[0]), el[1:]
    if not 1 <= stride <= 127:
        return "stride", None
    if ((moves != 0) & (moves != 1)).any():
        return "move", None
    if int(moves.sum()) != l_seq:
        return "ones", None
    if len(ts) > 1:
        return "ts fields", None
    value = None
    if ts:
        t = region[ts[0][0] + 2:ts[0][0] + 3]
        if t not in INT_FMT:
            return "ts type", None
        value = struct.unpack_from(INT_FMT[t], region, ts[0][0] + 3)[0]
        if value < 0:
            return "ts negative", None
    return None, (mv[0], ts[0] if ts else None, stride, moves, value)


def cut(region, l_seq, flag, s, n, fragment_mode=False):
    """the rewritten fields of the CHANGED output record [s, s + n) -> (cause or None, {field start: new bytes}, entries kept, cut)"""
    cause, parsed = why_not(region, l_seq, flag, fragment_mode)
    if cause:
        return cause, {}, 0, 0
    mv, ts, stride, moves, value = parsed
    m = len(moves)
    p = [0] + [int(i) + 1 for i in np.flatnonzero(moves)] + [m + 1]  # p[k], k = 1 .. l_seq + 1
    s, e = min(s, l_seq), min(s + n, l_seq)
    a = 1 if s == 0 else p[s + 1]
    b = a if e <= s else p[e + 1]
    new = {mv[0]: region[mv[0]:mv[0] + 4] + struct.pack("<I", 1 + b - a) + region[mv[0] + 8:mv[0] + 9] + region[mv[0] + 8 + a:mv[0] + 8 + b]}
    if ts:
        v = value + stride * (a - 1)
        if v > 2 ** 32 - 1:
            return "ts overflow", {}, 0, 0
        t = region[ts[0] + 2:ts[0] + 3]
        if v > INT_MAX[t]:
            t = b"S" if v <= 65535 else b"I"
        new[ts[0]] = b"ts" + t + struct.pack(INT_FMT[t], v)
        if len(new[mv[0]]) + len(new[ts[0]]) > mv[1] + ts[1]:
            return "size", {}, 0, 0
    return None, new, b - a, m - (b - a)


def mod_fields(region, codes, flag, s, n, fragment_mode=False):
    """--keep_mods' rule, field by field: -> (cause or None, {field start: new bytes}, positions kept, cut)"""
    cause, parsed = mc.why_not(region, codes, flag, fragment_mode)
    if cause:
        return cause, {}, 0, 0
    out, _, kept, gone, _ = mc.rewrite(region, codes, flag, s, n, fragment_mode)
    mine = {parsed[0][0], parsed[1][0]} | ({parsed[2][0]} if parsed[2] else set())
    new, rest = {}, tc.walk(out)[0]
    for a, ln, pos in tc.walk(region)[0]:  # (the output holds the three fields and the non-positional ones, in the input's order)
        if a in mine or not pos:
            b, bn, _ = rest.pop(0)
            if a in mine:
                new[a] = out[b:b + bn]
    assert not rest
    return None, new, kept, gone


def tags_of(region, codes, flag, s, n, mods, moves, fragment_mode=False):
    """the tag bytes of the CHANGED output record [s, s + n) under the two switches -> (bytes, lost a field?, mod verdict, move verdict);
    a verdict: None with the switch off or without the fields, else (re-indexed?, kept, cut)"""
    new, vm, vv = {}, None, None
    if mods:
        cause, f, kept, gone = mod_fields(region, codes, flag, s, n, fragment_mode)
        if cause != "no fields":
            vm = (cause is None, kept, gone)
            new.update(f)
    if moves:
        cause, f, kept, gone = cut(region, len(codes), flag, s, n, fragment_mode)
        if cause != "no table":
            vv = (cause is None, kept, gone)
            new.update(f)
    out, lost = b"", False
    for a, ln, pos in tc.walk(region)[0]:
        if a in new:
            out += new[a]
        elif not pos:
            out += region[a:a + ln]
        else:
            lost = True
    return out, lost, vm, vv


# ---- (b) the decoder ----
def spans(region):
    """-> (stride, [(first, end)] per base in absolute samples, ts present?) of a record's mv and ts (ts absent: counted from 0)"""
    by_tag = {}
    for a, n, _ in tc.walk(region)[0]:
        by_tag.setdefault(region[a:a + 2], []).append(region[a:a + n])
    assert len(by_tag.get(b"mv", [])) == 1 and len(by_tag.get(b"ts", [])) <= 1
    mv = by_tag[b"mv"][0]
    assert mv[2:4] in (b"Bc", b"BC") and struct.unpack_from("<I", mv, 4)[0] == len(mv) - 8 >= 1
    stride, at, out = mv[8], 0, []
    if b"ts" in by_tag:
        f = by_tag[b"ts"][0]
        at = struct.unpack(INT_FMT[f[2:3]], f[3:])[0]
    for e in mv[9:]:
        assert e in (0, 1)
        if e:
            out.append([at, at])
        if out:
            out[-1][1] += stride
        at += stride
    return stride, [tuple(x) for x in out], b"ts" in by_tag


def check_semantics(region, s, n, out_region):
    """the semantic property of a re-indexed record -> its bases"""
    stride, a, has_ts = spans(region)
    stride_b, b, has_ts_b = spans(out_region)
    assert stride == stride_b and has_ts == has_ts_b and len(b) == n
    want = a[s:s + n]
    if not has_ts and n:  # (no ts to carry the shift: the spans agree from the fragment's own first sample on)
        d = want[0][0] - b[0][0]
        assert d == 0 if s == 0 else d >= 0
        want = [(x - d, y - d) for x, y in want]
    assert b == want, (b[:3], want[:3])
    return n


# ---- the records a run writes ----
def expected(recs, res, mods=False, moves=True):
    """as mc.expected, under the two switches -> (--out records, --failed_out records, tag stats of each, mod stats of each, move
    stats of each, and [(name, region, s, n, out region)] of every record whose table was re-indexed, for the decoder)"""
    out, failed, done = [], [], []
    so, sf, mo, mf, vo, vf = ([0] * 4 for _ in range(6))
    kept = [r for r in recs if not r[1] & 0x900]
    assert len(kept) == len(res)

    def one(name, flag, codes, region, line, seq, q, a, n, changed, dst, st, ms, vs):
        fields, prefix = tc.walk(region)
        if changed:
            t, lost, vm, vv = tags_of(region, codes, flag, a, n, mods, moves)
            for v, c in ((vm, ms), (vv, vs)):
                if v:
                    c[0 if v[0] else 1] += 1
                    c[2], c[3] = (c[2] + v[1], c[3] + v[2]) if v[0] else (c[2], c[3])
            if vv and vv[0]:
                done.append((name, region, a, n, t))
        else:
            t, lost = tc.pick(region, False), False
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
                one(name, flag, codes, region, b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq, q, a, n, ch, out, so, mo, vo)
            elif r["n_frag"] == 1:
                a, n = int(r["r1_start"]), int(r["r1_len"])
                one(name, flag, codes, region, b"@" + name, seq, q, a, n, tc.is_changed(1, 0, a, n, len(codes), flag), failed, sf, mf, vf)
    return b"".join(out), b"".join(failed), so, sf, mo, mf, vo, vf, done


# ---- fields ----
def mv_field(stride, moves, sub=b"c", tag=b"mv"):
    return tc.barray(tag, sub, [stride] + [int(x) for x in moves])


def table(l_seq, m, rng, lead=0, ones_at=()):
    """m moves of which l_seq are 1: `lead` zeros in front, a one right behind them, ones at the 0-based places `ones_at`, the others drawn"""
    assert lead + l_seq <= m and (l_seq or not ones_at)
    moves = np.zeros(m, np.int64)
    fixed = sorted({lead, *ones_at}) if l_seq else []
    moves[fixed] = 1
    taken = set(fixed)
    free = np.array([i for i in range(lead + 1, m) if i not in taken], np.int64)
    moves[rng.choice(free, l_seq - len(fixed), replace=False)] = 1
    assert int(moves.sum()) == l_seq
    return moves


def fields_of(moves, stride=6, ts=(b"i", 40), sub=b"c", order="mt", pad=0, tail=11):
    """the fields of a basecalled read: kept fields around mv, ts and ns; order: mv in front of ts ("mt") or behind it; pad: bytes of a
    kept Z value in front, which moves the table through the byte alignments"""
    f = {"m": mv_field(stride, moves, sub), "t": tc.scalar(b"ts", *ts) if ts else b""}
    ns = tc.scalar(b"ns", b"i", min(2 ** 31 - 1, (ts[1] if ts else 0) + stride * len(moves) + tail))
    return tc.zfield(b"st", b"p" * pad) + f[order[0]] + tc.K1 + f[order[1]] + ns + tc.K3


def ranged(l_seq, *ranges, fail=False):
    """one fpl_read_result: a read of one passing (or failing) fragment [s, s + n), or of the two fragments of a split"""
    r = tc.result_of("whole", l_seq)
    if len(ranges) == 1:
        (s, n), = ranges
        r["r1_start"], r["r1_len"], r["frag_start"][0], r["frag_len"][0] = s, n, s, n
        if fail:
            r["code"][0] = abi.FPL_FAIL_LENGTH
    else:
        r["n_frag"] = 2
        r["frag_start"][:], r["frag_len"][:] = [x[0] for x in ranges], [x[1] for x in ranges]
        r["kind"][:], r["code"][1] = (1, 2), abi.FPL_PASS_FILTER
    return r


SIZES = (1, 2, 15, 16, 17, 1023, 1024, 1025, 2048, 2049, 5003)
CAUSES = ("flag", "mv fields", "subtype", "count", "stride", "move", "ones", "ts fields", "ts type", "ts negative", "ts overflow", "size")


def case_list(seed=53):
    """-> (recs [(name, flag, codes, qual, encoded record)], res, {name: the cause its table is not re-indexed for})"""
    rng = np.random.default_rng(seed)
    recs, res, causes = [], [], {}

    def read(l_seq):
        codes = rng.choice(np.array([1, 2, 4, 8, 1, 2, 4, 8, 15, 3], np.uint8), l_seq)
        codes[:3] = 2
        return codes.tobytes()

    def add(name, l_seq, tags, r, flag=0x4, cause=None, codes=None):
        codes = codes or read(l_seq)
        qual = rng.integers(2, 60, l_seq, dtype=np.uint8).tobytes()
        recs.append((name, flag, codes, qual, bamio.encode_record(name, flag, codes, qual, tags=tags)))
        res.append(r if not isinstance(r, str) else tc.result_of(r, l_seq))
        if cause:
            causes[name] = cause

    def under_plans(name, l_seq, tags, plans, **kw):
        for plan in plans:
            add(b"%s.%d.%s" % (name, l_seq, plan.encode()), l_seq, tags, plan, **kw)

    # ---- the sizes: one lane's bytes, one step of 64 x 16 bytes, the seams ----
    for k, m in enumerate(SIZES):
        l_seq = (m + 1) // 2
        mv = table(l_seq, m, rng, lead=min(3, m - l_seq) if k % 2 else 0)
        tags = fields_of(mv, ts=(b"iIsS"[k % 4:k % 4 + 1], 300 + k), sub=b"cC"[k % 2:k % 2 + 1], order=("mt", "tm")[k % 2], pad=k)
        if l_seq < 8:
            add(b"size.%d.to_nothing" % m, l_seq, tags, ranged(l_seq, (0, 0)))
            add(b"size.%d.tail_nothing" % m, l_seq, tags, ranged(l_seq, (l_seq, 0)))
            add(b"size.%d.whole" % m, l_seq, tags, "whole")
        else:
            under_plans(b"size.%d" % m, l_seq, tags, ("front", "tail", "split_both", "fails_trimmed", "whole", "split_one_fails"))
            add(b"size.%d.last_base" % m, l_seq, tags, ranged(l_seq, (l_seq - 1, 1)))  # s + n = l_seq from the last one on
            add(b"size.%d.first_base" % m, l_seq, tags, ranged(l_seq, (0, 1)))         # s = 0: the leading zeros stay
            add(b"size.%d.empty" % m, l_seq, tags, ranged(l_seq, (l_seq // 2, 0)))      # n = 0
    # ---- the ones looked for in a lane's first and last byte and in a step's first and last byte ----
    marks = (16 * 5, 16 * 5 + 15, 16 * 40, STEP - 1, STEP, STEP + 15, 2 * STEP - 1, 2 * STEP, 2 * STEP + 16 * 63 + 15)
    m, l_seq = 3 * STEP + 77, 1500
    mv = table(l_seq, m, rng, lead=2, ones_at=marks)
    before = [int(mv[:i].sum()) for i in marks]  # (the one at marks[k] is the (before[k] + 1)-th)
    for pad in (0, 5):
        tags = fields_of(mv, pad=pad)
        for i in range(len(marks)):
            for j in range(i + 1, len(marks), 3):
                add(b"marks.%d.%d.%d" % (pad, marks[i], marks[j]), l_seq, tags, ranged(l_seq, (before[i], before[j] - before[i])))
    # ---- split reads whose second fragment starts in a later step than the first ends, and in the same ----
    add(b"split.far", l_seq, fields_of(mv, pad=3), ranged(l_seq, (0, before[2]), (before[7] + 1, l_seq - before[7] - 1)))
    add(b"split.far.trimmed", l_seq, fields_of(mv, pad=9, order="tm"), ranged(l_seq, (7, before[3] - 7), (before[8], 10)))
    add(b"split.near", l_seq, fields_of(mv, ts=None), ranged(l_seq, (before[0], 9), (before[0] + 10, 30)))
    # ---- the field at every byte alignment; ts in front, behind and absent ----
    l_seq, m = 300, 700
    mv = table(l_seq, m, rng, lead=4)
    for pad in range(16):
        ts = None if pad % 4 == 3 else ((b"c", 100), (b"C", 200), (b"S", 40000))[pad % 3]
        under_plans(b"align.%d" % pad, l_seq, fields_of(mv, ts=ts, order=("mt", "tm")[pad % 2], pad=pad), (("front", "split_both", "tail")[pad % 3],))
    under_plans(b"no_ts", l_seq, fields_of(mv, ts=None), ("front", "tail", "split_both", "fails_trimmed"))
    # ---- ts in its type, and widened.  The first moves are ones: a front trim of s bases cuts s moves ----
    l_seq, m = 60, 130
    mv = table(l_seq, m, rng, ones_at=(1, 2, 3, 4))
    front = lambda s: ranged(l_seq, (s, l_seq - s))  # noqa: E731
    for key, ts, s, stride, cause in ((b"C_stays_255", (b"C", 237), 3, 6, None), (b"C_to_S", (b"C", 238), 3, 6, None), (b"c_to_S", (b"c", 120), 3, 6, None),
                                      (b"s_to_S", (b"s", 32760), 3, 6, None), (b"S_to_I_two_dropped", (b"S", 65530), 2, 6, None),
                                      (b"S_to_I_one_dropped", (b"S", 65532), 1, 6, "size"), (b"s_to_S_one_dropped", (b"s", 32700), 1, 127, None),
                                      (b"C_to_S_stride_127", (b"C", 255), 4, 127, None), (b"i_to_I", (b"i", 2 ** 31 - 3), 3, 6, None),
                                      (b"I_stays", (b"I", 2 ** 32 - 19), 3, 6, None), (b"I_overflow", (b"I", 2 ** 32 - 18), 3, 6, "ts overflow")):
        for order in ("mt", "tm"):
            add(b"ts.%s.%s" % (key, order.encode()), l_seq, fields_of(mv, stride=stride, ts=ts, order=order), front(s), cause=cause)
    # (a split read of which one fragment's ts overflows and the other's does not: each output record decides for itself)
    add(b"ts.split_one_overflows", l_seq, fields_of(mv, ts=(b"I", 2 ** 32 - 40)), ranged(l_seq, (0, 20), (30, 30)), cause="ts overflow")
    # ---- not re-indexable ----
    l_seq, m = 41, 90
    mv = table(l_seq, m, rng, lead=1)
    two, minus = mv.copy(), mv.copy()
    two[int(np.flatnonzero(mv == 0)[5])] = 2
    minus[m - 1 if mv[m - 1] == 0 else int(np.flatnonzero(mv == 0)[-1])] = -1
    more, fewer = mv.copy(), mv.copy()
    more[int(np.flatnonzero(mv == 0)[7])] = 1
    fewer[int(np.flatnonzero(mv == 1)[9])] = 0
    bad = {
        b"move_2": (fields_of(two), "move"), b"move_minus_1": (fields_of(minus), "move"),
        b"move_255": (fields_of(np.where(minus < 0, 255, minus), sub=b"C"), "move"),
        b"stride_0": (fields_of(mv, stride=0), "stride"), b"stride_minus_3": (fields_of(mv, stride=-3), "stride"),
        b"stride_200": (fields_of(mv, stride=200, sub=b"C"), "stride"),
        b"one_one_more": (fields_of(more), "ones"), b"one_one_less": (fields_of(fewer), "ones"),
        b"two_mv": (fields_of(mv) + mv_field(6, mv), "mv fields"),
        b"subtype_s": (tc.K1 + tc.barray(b"mv", b"s", [6] + [int(x) for x in mv]) + tc.scalar(b"ts", b"i", 5), "subtype"),
        b"count_0": (tc.K2 + tc.barray(b"mv", b"c", []) + tc.scalar(b"ts", b"i", 5), "count"),
        b"ts_negative": (fields_of(mv, ts=(b"i", -5)), "ts negative"), b"ts_negative_c": (fields_of(mv, ts=(b"c", -1), order="tm"), "ts negative"),
        b"two_ts": (fields_of(mv) + tc.scalar(b"ts", b"C", 9), "ts fields"),
        b"ts_Z": (tc.zfield(b"ts", b"40") + mv_field(6, mv) + tc.K1, "ts type"),
    }
    for key, (tags, cause) in bad.items():
        under_plans(key, l_seq, tags, ("front", "split_both", "whole", "fails_trimmed"), cause=cause)
    under_plans(b"reversed", l_seq, fields_of(mv), ("front", "split_both", "whole"), flag=0x14, cause="flag")
    # ---- records that carry both MM / ML and a table, whole and with each of them broken ----
    for l_seq in (77, 1030):
        codes = read(l_seq)
        m = 2 * l_seq + 9
        mv = table(l_seq, m, rng, lead=3)
        spec = [(b"C+m?", mc.every(codes, b"C", 2)), (b"N+n", mc.every(codes, b"N", 7, 2))]
        n_ml = sum(len(d) for _, d in spec)
        good_mods = lambda between: mc.fields_of(codes, spec, rng, between=between)  # noqa: E731
        short_ml = lambda between: tc.K2 + mc.mm_field(spec) + between + mc.ml_field([7] * (n_ml - 1))  # noqa: E731
        broken = mv.copy()
        broken[int(np.flatnonzero(mv == 0)[3])] = 2
        both = mv_field(6, mv) + tc.scalar(b"ts", b"S", 17)
        for key, tags, cause in ((b"both", good_mods(both), None), (b"both.mods_broken", short_ml(both), None),
                                 (b"both.moves_broken", good_mods(mv_field(6, broken) + tc.scalar(b"ts", b"S", 17)), "move"),
                                 (b"both.and_another_array", good_mods(both) + tc.barray(b"pt", b"S", [1, 2, 3]), None)):
            under_plans(key, l_seq, tags, ("front", "split_both", "tail", "fails_trimmed"), cause=cause, codes=codes)
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE)), causes


def malformed_list():
    """records whose region does not parse behind the table: the ts lies outside the parsed prefix, which holds one mv and is
    re-indexable by itself (library-level tests only: the CLI's reader refuses such records)"""
    rng = np.random.default_rng(6)
    recs, res = [], []
    for l_seq, plan in ((40, "front"), (41, "split_both"), (77, "whole"), (77, "fails_trimmed")):
        codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), l_seq).tobytes()
        qual = bytes([30]) * l_seq
        tags = tc.K1 + mv_field(5, table(l_seq, 2 * l_seq, rng, lead=1)) + b"xxQ\1\2\3" + tc.scalar(b"ts", b"i", 9)
        name = b"cut_behind_mv.%d.%s" % (l_seq, plan.encode())
        recs.append((name, 0x4, codes, qual, bamio.encode_record(name, 0x4, codes, qual, tags=tags)))
        res.append(tc.result_of(plan, l_seq))
    return recs, np.array(res, np.dtype(abi.RESULT_DTYPE))


# ---- the conditions the list must meet, by the Python rule alone ----
def _conditions():
    recs, res, causes = case_list()
    want = expected(recs, res)
    assert want[6][0] + want[7][0] >= 40 and want[7][0] >= 5 and want[6][1] >= 10 and want[7][1] >= 1, (want[6], want[7])
    by_name = {r[0]: (r, x) for r, x in zip(recs, res)}
    seen = set()
    for name, cause in causes.items():
        (_, flag, codes, _, enc), r = by_name[name]
        region = tc.aux_region(enc)
        mine = {cut(region, len(codes), flag, int(r["frag_start"][f]), int(r["frag_len"][f]))[0] for f in range(max(1, int(r["n_frag"])))}
        assert cause in mine, (name, mine)
        seen.add(cause)
    assert seen == set(CAUSES), set(CAUSES) ^ seen
    # every record's output tag bytes stay inside its input region, with --keep_mods beside the switch too
    for mods in (False, True):
        for (name, flag, codes, _, enc), r in zip(recs, res):
            region = tc.aux_region(enc)
            for s, n in [(int(r["frag_start"][f]), int(r["frag_len"][f])) for f in range(int(r["n_frag"]))] + [(int(r["r1_start"]), int(r["r1_len"]))]:
                assert len(tags_of(region, codes, flag, s, n, mods, True)[0]) <= len(region), name
    for name, region, s, n, t in want[8]:
        check_semantics(region, s, n, t)
    both = expected(recs, res, mods=True)
    assert both[4][0] >= 8 and both[4][1] >= 4 and both[6] == want[6]
    mrecs, mres = malformed_list()
    assert all(why_not(tc.aux_region(r[4]), len(r[2]), r[1])[0] is None and tc.walk(tc.aux_region(r[4]))[1] < len(tc.aux_region(r[4])) for r in mrecs)
    return True


CONDITIONS_HOLD = _conditions()
