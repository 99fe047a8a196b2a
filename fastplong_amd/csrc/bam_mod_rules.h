/*
 * bam_mod_rules.h -- how the base modification fields of an INPUT BAM record (MM / ML / MN, SAM tags text section 1.7) follow
 * an OUTPUT record that is a piece [s, s + n) of its read (README "BAM output", --keep_mods): one text for the host's converter
 * (host/bam_out.cpp) and for device code, as bam_tag_rules.h is for the fields that travel verbatim.  Plain C++, no HIP header.
 *
 * RE-INDEXABLE is a record of which all of this holds:
 *   flag     the input flag has no 0x10, and the run uses neither --mask nor --break
 *   fields   the parsed prefix of its aux region (bam_tag_rules.h) holds exactly one field tagged MM or Mm, of type Z; exactly one
 *            tagged ML or Ml, of type B and subtype C; at most one tagged MN or Mn, of an integer type (cCsSiI), its value l_seq
 *   grammar  the MM value without its NUL is zero to 16 groups.  A group: a base out of ACGTN, a strand + or -, codes -- one or
 *            more of a-z (k = how many) or one or more digits (a ChEBI id, k = 1) --, an optional . or ?, zero or more deltas,
 *            a ';'.  A delta: ',' and 1 to 9 decimal digits, leading zeros allowed
 *   sums     for every group the sum of (delta + 1) is at most the count of its base in the record's 4-bit codes: A 1, C 2, G 4,
 *            T 8, exact matches only; N counts every base
 *   ML       its count is the sum over the groups of deltas x k
 * Any other record is handled by bam_tag_rules.h alone: a changed output record drops its positional fields.
 *
 * A CHANGED output record [s, s + n) of a re-indexable record gets its non-positional fields as before and, in the places of the
 * three fields, rewritten ones; every other positional field is still dropped.  For a group of base b: c0 = the count of b in
 * [0, s), c1 = the count in [0, s + n); modification j sits on occurrence o_j = sum over i <= j of (d_i + 1), less 1; KEPT is the
 * contiguous range j0 <= j < j1 with c0 <= o_j < c1.
 *   MM   tag, type and the group's header bytes verbatim; when something is kept ',' and the decimal of o_j0 - c0 without leading
 *        zeros, then the input's bytes from the comma in front of delta j0 + 1 through the last digit of delta j1 - 1; then ';'.
 *        The value ends with a NUL
 *   ML   tag, 'B', 'C', the new count, and of every group's share its bytes [j0 k, j1 k), in group order
 *   MN   tag and type verbatim, the value n (n <= l_seq: it fits the type that held l_seq)
 *
 * SIZE.  o_j0 - c0 <= d_j0: o_j0 - d_j0 - 1 is the occurrence of modification j0 - 1 (or -1 when j0 is 0), which lies below c0
 * because j0 is the first that does not.  So the new first delta never has more digits than the one it replaces, every other
 * byte of a rewritten field is a byte of the input's field, and a record's tag bytes never exceed its input region.  The bound
 * of csrc/bam_tags.h -- at most twice the input record bytes more -- stands with the switch on.
 */
#ifndef FPL_BAM_MOD_RULES_H
#define FPL_BAM_MOD_RULES_H

#include <stdint.h>

#include "bam_tag_rules.h"

namespace fpl {
namespace bammod {

constexpr uint32_t MAX_GROUPS = 16;
constexpr uint32_t MAX_DIGITS = 9;

/* f: the two tag bytes of a field */
FPL_BAMTAG_HD inline bool mm_tag(const uint8_t* f) { return f[0] == 'M' && (f[1] == 'M' || f[1] == 'm'); }
FPL_BAMTAG_HD inline bool ml_tag(const uint8_t* f) { return f[0] == 'M' && (f[1] == 'L' || f[1] == 'l'); }
FPL_BAMTAG_HD inline bool mn_tag(const uint8_t* f) { return f[0] == 'M' && (f[1] == 'N' || f[1] == 'n'); }

/* the modification fields of a parsed prefix: how many carry each tag, and where the last of each lies in the region */
struct Found {
    uint32_t n_mm, n_ml, n_mn;
    uint64_t mm_at, mm_len, ml_at, ml_len, mn_at, mn_len; /* a field's first tag byte, its bytes */
};
FPL_BAMTAG_HD inline Found nothing_found() { return Found{0, 0, 0, 0, 0, 0, 0, 0, 0}; }
/* the walk's step: the field of n bytes at p + at */
FPL_BAMTAG_HD inline void note(Found& fd, const uint8_t* p, uint64_t at, uint64_t n) {
    if (mm_tag(p + at)) fd.n_mm++, fd.mm_at = at, fd.mm_len = n;
    else if (ml_tag(p + at)) fd.n_ml++, fd.ml_at = at, fd.ml_len = n;
    else if (mn_tag(p + at)) fd.n_mn++, fd.mn_at = at, fd.mn_len = n;
}
FPL_BAMTAG_HD inline bool any_found(const Found& fd) { return fd.n_mm + fd.n_ml + fd.n_mn != 0; }
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
/* the "fields" condition */
FPL_BAMTAG_HD inline bool fields_ok(const Found& fd, const uint8_t* p, uint64_t l_seq) {
    if (fd.n_mm != 1 || fd.n_ml != 1 || fd.n_mn > 1) return false;
    if (p[fd.mm_at + 2] != 'Z' || p[fd.ml_at + 2] != 'B' || p[fd.ml_at + 3] != 'C') return false;
    if (fd.n_mn && (!integer_type(p[fd.mn_at + 2]) || integer_value(p + fd.mn_at) != (int64_t)l_seq)) return false;
    return true;
}

/* ---- the grammar ---- */
FPL_BAMTAG_HD inline bool digit(uint32_t c) { return c - '0' < 10u; }
FPL_BAMTAG_HD inline bool lower(uint32_t c) { return c - 'a' < 26u; }
/* the 4-bit code a group's base counts: A 1, C 2, G 4, T 8; N 0 (every base); 0xFF: not a base of the grammar */
FPL_BAMTAG_HD inline uint32_t base_code(uint32_t c) {
    return c == 'A' ? 1u : c == 'C' ? 2u : c == 'G' ? 4u : c == 'T' ? 8u : c == 'N' ? 0u : 0xFFu;
}
struct Group {
    uint32_t at;      /* its first byte in the MM value */
    uint32_t hdr_len; /* base, strand, codes, the optional . or ? */
    uint32_t code;    /* base_code of its base */
    uint32_t k;       /* ML bytes per delta */
    uint32_t n_delta;
    uint32_t end;     /* its ';' in the MM value */
    uint64_t sum;     /* of (delta + 1) */
    uint64_t ml_at;   /* its share of the ML values starts here */
};
/* the decimal of the 1 to 9 digits v[a, b) */
FPL_BAMTAG_HD inline uint32_t number(const uint8_t* v, uint32_t a, uint32_t b) {
    uint32_t x = 0;
    for (; a < b; a++) x = 10 * x + (v[a] - '0');
    return x;
}
/* the delta behind the comma at v[at] (at < len) -> the byte behind its last digit, 0: not a delta */
FPL_BAMTAG_HD inline uint32_t delta_end(const uint8_t* v, uint32_t len, uint32_t at) {
    uint32_t e = at + 1;
    while (e < len && e - at - 1 <= MAX_DIGITS && digit(v[e])) e++;
    const uint32_t digits = e - at - 1;
    return digits >= 1 && digits <= MAX_DIGITS ? e : 0;
}
/* the header of the group at v[at] -> its bytes, 0: not one */
FPL_BAMTAG_HD inline uint32_t header_len(const uint8_t* v, uint32_t len, uint32_t at, uint32_t& code, uint32_t& k) {
    if (len - at < 3) return 0;
    code = base_code(v[at]);
    if (code == 0xFFu || (v[at + 1] != '+' && v[at + 1] != '-')) return 0;
    uint32_t e = at + 2;
    if (lower(v[e])) {
        while (e < len && lower(v[e])) e++;
        k = e - at - 2;
    } else if (digit(v[e])) {
        while (e < len && digit(v[e])) e++;
        k = 1;
    } else
        return 0;
    if (e < len && (v[e] == '.' || v[e] == '?')) e++;
    return e - at;
}
/* the MM value v[0, len) (without its NUL) -> its groups; false: it is not of the grammar */
FPL_BAMTAG_HD inline bool parse(const uint8_t* v, uint32_t len, Group* g, uint32_t& n_groups) {
    n_groups = 0;
    uint64_t ml = 0;
    for (uint32_t at = 0; at < len;) {
        if (n_groups == MAX_GROUPS) return false;
        Group& x = g[n_groups];
        x.at = at;
        x.hdr_len = header_len(v, len, at, x.code, x.k);
        if (!x.hdr_len) return false;
        x.n_delta = 0, x.sum = 0, x.ml_at = ml;
        uint32_t e = at + x.hdr_len;
        while (e < len && v[e] == ',') {
            const uint32_t de = delta_end(v, len, e);
            if (!de) return false;
            x.sum += (uint64_t)number(v, e + 1, de) + 1;
            x.n_delta++;
            e = de;
        }
        if (e >= len || v[e] != ';') return false;
        x.end = e;
        ml += (uint64_t)x.n_delta * x.k;
        at = e + 1;
        n_groups++;
    }
    return true;
}
/* bases of code `code` (0: all) among the first `to` of the 4-bit codes at pk (high nibble first; to <= l_seq, so the zero low
   nibble behind an odd l_seq is never looked at) */
FPL_BAMTAG_HD inline uint64_t count_bases(const uint8_t* pk, uint64_t to, uint32_t code) {
    if (code == 0) return to;
    uint64_t c = 0;
    for (uint64_t i = 0; i < to; i++) c += ((pk[i >> 1] >> ((i & 1) ? 0 : 4)) & 15u) == code;
    return c;
}

/* everything a re-indexable record's fragments are cut from */
struct Record {
    Found fd;
    uint32_t n_groups;
    Group g[MAX_GROUPS];
    uint64_t total[5]; /* bases of code 1, 2, 4, 8 (at [0..4)) and all of them */
};
FPL_BAMTAG_HD inline uint32_t code_slot(uint32_t code) { return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u; }
/* rec: the input record (its block_size field), p: its aux region, fd: what find() found in the parsed prefix.  true: the record is
   re-indexable, and R says how */
FPL_BAMTAG_HD inline bool reindexable(const uint8_t* rec, const uint8_t* p, const Found& fd, bool fragment_mode, Record& R) {
    const bamrule::Fields f = bamrule::fields(rec);
    if ((f.flag & 0x10u) || fragment_mode || !fields_ok(fd, p, f.l_seq)) return false;
    if (fd.mm_len - 4 > 0xFFFFFFF0ull) return false;
    R.fd = fd;
    const uint8_t* v = p + fd.mm_at + 3;
    if (!parse(v, (uint32_t)(fd.mm_len - 4), R.g, R.n_groups)) return false;
    const uint8_t* pk = rec + bamrule::qual_offset(f) - ((uint64_t)f.l_seq + 1) / 2;
    uint32_t want = 0; /* which counts the groups ask for */
    for (uint32_t k = 0; k < R.n_groups; k++) want |= 1u << code_slot(R.g[k].code);
    for (uint32_t s = 0; s < 5; s++) R.total[s] = (want >> s & 1u) ? count_bases(pk, f.l_seq, s < 4 ? 1u << s : 0u) : 0;
    uint64_t ml = 0;
    for (uint32_t k = 0; k < R.n_groups; k++) {
        if (R.g[k].sum > R.total[code_slot(R.g[k].code)]) return false;
        ml += (uint64_t)R.g[k].n_delta * R.g[k].k;
    }
    return ml == (uint64_t)bamrule::rd32(p + fd.ml_at + 4);
}

/* what a fragment keeps of one group */
struct Cut {
    uint32_t j0, j1;   /* the kept modifications */
    uint32_t first;    /* the new first delta, o_j0 - c0 (j0 < j1) */
    uint32_t rest_at;  /* the verbatim delta bytes, in the MM value: from the comma in front of delta j0 + 1 ... */
    uint32_t rest_end; /* ... to behind the last digit of delta j1 - 1 */
};
/* v: the MM value; c0, c1: the counts of the group's base in front of the fragment and up to its end */
FPL_BAMTAG_HD inline Cut cut(const uint8_t* v, uint32_t len, const Group& g, uint64_t c0, uint64_t c1) {
    Cut c = {0, 0, 0, 0, 0};
    uint64_t o = 0; /* occurrences up to and including modification j */
    uint32_t e = g.at + g.hdr_len, j = 0;
    bool in = false;
    for (; j < g.n_delta; j++) {
        const uint32_t de = delta_end(v, len, e);
        o += (uint64_t)number(v, e + 1, de) + 1;
        if (o - 1 >= c1) break;
        if (!in && o - 1 >= c0) in = true, c.j0 = j, c.first = (uint32_t)(o - 1 - c0), c.rest_at = de;
        if (in) c.rest_end = de;
        e = de;
    }
    if (in) c.j1 = j;
    return c;
}
/* decimal digits of x */
FPL_BAMTAG_HD inline uint32_t digits_of(uint32_t x) {
    uint32_t n = 1;
    while (x >= 10) x /= 10, n++;
    return n;
}

}  // namespace bammod
}  // namespace fpl
#endif
