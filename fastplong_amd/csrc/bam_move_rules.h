/*
 * bam_move_rules.h -- how the move table of an INPUT BAM record (mv:B:c, the basecaller's base-to-signal map) and its ts follow an
 * OUTPUT record that is a piece [s, s + n) of its read (README "BAM output", --keep_moves): one text for the host's converter
 * (host/bam_out.cpp) and for device code (csrc/bam_moves.h), as bam_mod_rules.h is for MM / ML / MN.  Plain C++, no HIP header.
 *
 * THE TABLE is a field tagged mv of type B, subtype c or C, with a count of at least 1.  Element 0 is the stride, elements 1..m
 * are the moves e_1..e_m.  p(k) is the index of the k-th move equal to 1, k = 1..l_seq, and p(l_seq + 1) = m + 1.  The table is
 * taken to run in the read's direction.
 *
 * MOVE-RE-INDEXABLE is a record of which all of this holds:
 *   flag     the input flag has no 0x10, and the run uses neither --mask nor --break
 *   fields   the parsed prefix of its aux region (bam_tag_rules.h) holds exactly one field tagged mv, of that type; at most one
 *            tagged ts, of an integer type (cCsSiI), its value not negative
 *   table    the stride is in 1..127, every move is 0 or 1, the moves equal to 1 number exactly l_seq
 * Any other record is handled by the other rules alone.
 *
 * A CHANGED output record [s, s + n) of such a record gets its other fields as those rules say and, in the places of mv and ts:
 *   mv   tag, 'B' and the subtype verbatim, the new count 1 + (b - a), the stride, the moves e_a .. e_(b-1).  a = 1 when s == 0
 *        (leading zeros stay), else p(s + 1); b = p(s + n + 1); for n == 0 b = a: the field is the stride alone
 *   ts   the tag and the value ts + stride x (a - 1), in its own type when the value fits it, else in the narrower of S and I that
 *        holds it.  An output record whose value lies above 2^32 - 1 is written as without the switch
 * ns and every other integer field travel verbatim: the samples cut from the tail are ns - ts' - stride x (b - a).
 *
 * SIZE.  An output record whose rewritten mv + ts bytes would exceed the bytes they replace is written as without the switch.
 * The new mv has (a - 1) + (m + 1 - b) bytes fewer than the old one.  ts grows by 1 byte (c C -> S), by 2 (s S -> I) or by 3
 * (c C -> I).  It grows only when stride x (a - 1) > 0, so a - 1 >= 1 and the growth of 1 is always paid for; a growth of 3 takes
 * a value above 65535 from one of at most 255, so stride x (a - 1) > 65280 and a - 1 > 514.  That leaves a growth of 2 with
 * a - 1 == 1 and b == m + 1: ts widens by two bytes while one move is dropped, and only then does the clause refuse.  So a
 * re-indexed record's tag bytes never exceed its input region, and the bound of csrc/bam_tags.h -- at most twice the input record
 * bytes more -- stands with the switch on, alone or beside --keep_mods (whose own SIZE argument covers its fields).
 */
#ifndef FPL_BAM_MOVE_RULES_H
#define FPL_BAM_MOVE_RULES_H

#include <stdint.h>

#include "bam_tag_rules.h"

namespace fpl {
namespace bammove {

/* f: the two tag bytes of a field */
FPL_BAMTAG_HD inline bool mv_tag(const uint8_t* f) { return f[0] == 'm' && f[1] == 'v'; }
FPL_BAMTAG_HD inline bool ts_tag(const uint8_t* f) { return f[0] == 't' && f[1] == 's'; }

/* the two fields of a parsed prefix: how many carry each tag, and where the last of each lies in the region */
struct Found {
    uint32_t n_mv, n_ts;
    uint64_t mv_at, mv_len, ts_at, ts_len; /* a field's first tag byte, its bytes */
};
FPL_BAMTAG_HD inline Found nothing_found() { return Found{0, 0, 0, 0, 0, 0}; }
/* the walk's step: the field of n bytes at p + at */
FPL_BAMTAG_HD inline void note(Found& fd, const uint8_t* p, uint64_t at, uint64_t n) {
    if (mv_tag(p + at)) fd.n_mv++, fd.mv_at = at, fd.mv_len = n;
    else if (ts_tag(p + at)) fd.n_ts++, fd.ts_at = at, fd.ts_len = n;
}
/* a record without a table is none of this rule's business, whatever its ts */
FPL_BAMTAG_HD inline bool any_found(const Found& fd) { return fd.n_mv != 0; }
template <class ZScan>
FPL_BAMTAG_HD inline Found find(const uint8_t* p, uint64_t prefix, const ZScan& zscan) {
    Found fd = nothing_found();
    for (uint64_t o = 0; o < prefix;) {
        const uint64_t n = bamtag::field_len(p + o, prefix - o, zscan);
        if (!n) break;
        note(fd, p, o, n);
        o += n;
    }
    return fd;
}
FPL_BAMTAG_HD inline bool integer_type(uint32_t t) { return t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I'; }
/* the value of the integer field at f, -1 where it is negative */
FPL_BAMTAG_HD inline int64_t integer_value(const uint8_t* f) {
    switch (f[2]) {
        case 'c': return (int8_t)f[3] < 0 ? -1 : f[3];
        case 'C': return f[3];
        case 's': return (int16_t)bamrule::rd16(f + 3) < 0 ? -1 : (int64_t)bamrule::rd16(f + 3);
        case 'S': return bamrule::rd16(f + 3);
        case 'i': return (int32_t)bamrule::rd32(f + 3) < 0 ? -1 : (int64_t)bamrule::rd32(f + 3);
        default: return bamrule::rd32(f + 3);
    }
}
/* the largest value of an integer type */
FPL_BAMTAG_HD inline uint64_t type_max(uint32_t t) {
    return t == 'c' ? 127u : t == 'C' ? 255u : t == 's' ? 32767u : t == 'S' ? 65535u : t == 'i' ? 0x7FFFFFFFu : 0xFFFFFFFFu;
}

/* what the fields say of a record's table */
struct Table {
    uint64_t m;      /* moves */
    uint32_t stride;
    bool has_ts;
    uint32_t ts_type;
    uint64_t ts;
};
/* the "flag" and "fields" conditions and the stride's; T: the table but for its moves, which the caller checks and counts */
FPL_BAMTAG_HD inline bool fields_ok(const Found& fd, const uint8_t* p, uint32_t flag, bool fragment_mode, Table& T) {
    if ((flag & 0x10u) || fragment_mode || fd.n_mv != 1 || fd.n_ts > 1) return false;
    const uint8_t* f = p + fd.mv_at;
    if (f[2] != 'B' || (f[3] != 'c' && f[3] != 'C')) return false;
    const uint32_t count = bamrule::rd32(f + 4);
    if (count < 1) return false;
    T.m = (uint64_t)count - 1;
    T.stride = f[8];
    if (T.stride < 1 || T.stride > 127) return false; /* (a negative c is above 127 as a byte) */
    T.has_ts = fd.n_ts != 0, T.ts_type = 0, T.ts = 0;
    if (T.has_ts) {
        const uint8_t* t = p + fd.ts_at;
        if (!integer_type(t[2])) return false;
        const int64_t v = integer_value(t);
        if (v < 0) return false;
        T.ts_type = t[2], T.ts = (uint64_t)v;
    }
    return true;
}
/* the moves e_1..e_m at mv: true when every one is 0 or 1; ones: how many are 1 */
FPL_BAMTAG_HD inline bool count_moves(const uint8_t* mv, uint64_t m, uint64_t& ones) {
    ones = 0;
    for (uint64_t k = 0; k < m; k++) {
        if (mv[k] > 1) return false;
        ones += mv[k];
    }
    return true;
}
/* p(k) for 1 <= k <= ones + 1 of checked moves */
FPL_BAMTAG_HD inline uint64_t position(const uint8_t* mv, uint64_t m, uint64_t k) {
    uint64_t seen = 0;
    for (uint64_t i = 0; i < m; i++) {
        seen += mv[i];
        if (seen == k) return i + 1;
    }
    return m + 1;
}

/* what an output record gets */
struct Cut {
    uint64_t a, b;    /* the moves e_a .. e_(b-1) */
    uint64_t ts;      /* the new value ... */
    uint32_t ts_type; /* ... and its type (a record with a ts) */
};
/* a and b are known: the new ts and the SIZE clause.  false: this output record is written as without the switch */
FPL_BAMTAG_HD inline bool finish(const Table& T, Cut& c) {
    c.ts = 0, c.ts_type = 0;
    if (!T.has_ts) return true;
    c.ts = T.ts + (uint64_t)T.stride * (c.a - 1);
    if (c.ts > 0xFFFFFFFFull) return false;
    c.ts_type = c.ts <= type_max(T.ts_type) ? T.ts_type : c.ts <= 65535u ? (uint32_t)'S' : (uint32_t)'I';
    const uint64_t grown = bamtag::scalar_size(c.ts_type) - bamtag::scalar_size(T.ts_type);
    return grown <= T.m - (c.b - c.a);
}
/* bytes of the rewritten fields less the bytes of the fields they replace, modulo 2^64 (never positive) */
FPL_BAMTAG_HD inline uint64_t growth(const Table& T, const Cut& c) {
    const uint64_t ts = T.has_ts ? (uint64_t)bamtag::scalar_size(c.ts_type) - bamtag::scalar_size(T.ts_type) : 0;
    return ts - (T.m - (c.b - c.a));
}
/* the ends of the fragment [start, start + len) inside the read */
FPL_BAMTAG_HD inline void clamp_range(uint64_t start, uint64_t len, uint64_t l_seq, uint64_t& s, uint64_t& e) {
    s = start < l_seq ? start : l_seq;
    e = start + len < l_seq ? start + len : l_seq;
}
/* a and b from p(s + 1) and p(e + 1), the fragment being [s, e) */
FPL_BAMTAG_HD inline void ends(uint64_t s, uint64_t e, uint64_t p_s1, uint64_t p_e1, Cut& c) {
    c.a = s == 0 ? 1 : p_s1;
    c.b = e <= s ? c.a : p_e1;
}

}  // namespace bammove
}  // namespace fpl
#endif
