/*
 * bam_comment_rules.h -- a BAM record's auxiliary fields as the COMMENT of a FASTQ name line (README "Tags as FASTQ comments",
 * --comment_tags): one text for the host's form (host/bam_comments.cpp) and for device code, as bam_tag_rules.h and
 * bam_mod_rules.h are for the fields themselves.  Plain C++, no HIP header needed.
 *
 * WHICH FIELDS.  The comment of an output read is made from the auxiliary fields the same run's .bam record of that read would
 * carry under --keep_tags --keep_mods: an unchanged record the parsed prefix verbatim, a changed one its non-positional fields,
 * a changed record of a re-indexable input record also MM / ML / MN rewritten for its piece; in a --break / --mask run every
 * record is changed and nothing is re-indexed.  bam_tag_rules.h and bam_mod_rules.h alone say what survives; re-indexing is
 * always on here (a stale MM in a FASTQ comment is worse than none).  The fields come in the record's order, restricted to the
 * run's SELECTION: every field, or a list of at most 32 two-character tags matched exactly (MM is not Mm).
 *
 * TEXT OF A FIELD (the SAM text form), XX its tag:
 *   A        XX:A:<byte>
 *   c s i    XX:i:<signed decimal>            C S I    XX:i:<unsigned decimal>
 *   f        XX:f: and the bytes of C's printf("%g", (double)v), inf, -inf, nan, -nan included (fmt_float below)
 *   Z, H     XX:Z: / XX:H: and the value without its NUL
 *   B        XX:B:<subtype>, then ,<value> per element, formatted as the scalar of that subtype; a count of 0 gives XX:B:C alone
 *
 * WHERE.  At the end of the name line the formatter writes -- behind --failed_out's failure word, behind a split read's name with
 * its prefix --, every written field preceded by one tab.  No selected field: the line is byte for byte the formatter's.
 *
 * LEFT OUT.  A selected A, Z or H field whose value holds a byte below 0x20 or the byte 0x7F is not written and is counted: a tab
 * or a newline would break the FASTQ.
 *
 * BOUND.  A field's text, tab included, is never more than 5 times its bytes (field_text_bound): the worst case is B:c, ",-128"
 * per byte.  So a comment is at most 5 times the record's tag bytes, and those never exceed the input region (bam_mod_rules.h,
 * SIZE).
 */
#ifndef FPL_BAM_COMMENT_RULES_H
#define FPL_BAM_COMMENT_RULES_H

#include <stdint.h>

#include "bam_tag_rules.h"

namespace fpl {
namespace bamcomment {

constexpr int32_t MAX_TAGS = 32;
constexpr uint32_t FLOAT_TEXT_MAX = 12; /* "-3.40282e+38", "-0.000123456" */
constexpr uint32_t SCALAR_TEXT_MAX = 12;

/* ---- the selection ---- */
struct Selection {
    int32_t n;                 /* 0: off, -1: every field, else the tags of the list */
    uint8_t tag[2 * MAX_TAGS]; /* two bytes each */
};
FPL_BAMTAG_HD inline bool tag_bytes_ok(uint32_t a, uint32_t b) {
    const bool a_ok = (a - 'A' < 26u) || (a - 'a' < 26u);
    const bool b_ok = (b - 'A' < 26u) || (b - 'a' < 26u) || (b - '0' < 10u);
    return a_ok && b_ok;
}
/* tags: 2 * n_tags bytes; n_tags 0: off, -1: every field.  false: more than MAX_TAGS tags, or a byte outside [A-Za-z][A-Za-z0-9] */
FPL_BAMTAG_HD inline bool make_selection(const char* tags, int32_t n_tags, Selection& s) {
    s.n = 0;
    for (int32_t k = 0; k < 2 * MAX_TAGS; k++) s.tag[k] = 0;
    if (n_tags < -1 || n_tags > MAX_TAGS) return false;
    for (int32_t k = 0; k < n_tags; k++) {
        if (!tag_bytes_ok((uint8_t)tags[2 * k], (uint8_t)tags[2 * k + 1])) return false;
        s.tag[2 * k] = (uint8_t)tags[2 * k], s.tag[2 * k + 1] = (uint8_t)tags[2 * k + 1];
    }
    s.n = n_tags;
    return true;
}
/* f: the two tag bytes of a field */
FPL_BAMTAG_HD inline bool selected(const Selection& s, const uint8_t* f) {
    if (s.n < 0) return true;
    for (int32_t k = 0; k < s.n; k++)
        if (s.tag[2 * k] == f[0] && s.tag[2 * k + 1] == f[1]) return true;
    return false;
}

/* ---- the bound ---- */
/* the most text, tab included, a field of n bytes gives */
FPL_BAMTAG_HD constexpr uint64_t field_text_bound(uint64_t n) { return 5 * n; }
/* ... checked type by type: "\tXX:t:" is 6 bytes in front of a field's 3; a value of w bytes gives at most m bytes of text */
static_assert(6 + 1 <= 5 * (3 + 1), "A");
static_assert(6 + 4 <= 5 * (3 + 1) && 6 + 6 <= 5 * (3 + 2) && 6 + 11 <= 5 * (3 + 4), "c C s S i I: -128, -32768, -2147483648");
static_assert(6 + FLOAT_TEXT_MAX <= 5 * (3 + 4), "f");
/* Z, H: 6 + (z - 1) for 3 + z bytes.  B: "\tXX:B:s" is 7 bytes for the field's 8, an element of w bytes gives a comma and its text */
static_assert(1 + 4 <= 5 * 1 && 1 + 6 <= 5 * 2 && 1 + 11 <= 5 * 4 && 1 + FLOAT_TEXT_MAX <= 5 * 4, "B elements: ,-128 per byte is the worst");

/* ---- numbers ---- */
/* the decimal of v at out (at most 10 bytes) -> its length */
FPL_BAMTAG_HD inline uint32_t fmt_u32(uint32_t v, char* out) {
    char t[10];
    uint32_t n = 0;
    do t[n++] = (char)('0' + v % 10), v /= 10;
    while (v);
    for (uint32_t k = 0; k < n; k++) out[k] = t[n - 1 - k];
    return n;
}
/* ... of a signed value (at most 11 bytes) */
FPL_BAMTAG_HD inline uint32_t fmt_i32(int32_t v, char* out) {
    if (v >= 0) return fmt_u32((uint32_t)v, out);
    out[0] = '-';
    return 1 + fmt_u32(0u - (uint32_t)v, out + 1);
}

/* the text of printf("%g", (double)v) for the float of these bits, at out (at most FLOAT_TEXT_MAX bytes) -> its length.
   Integer arithmetic only.  The value is m 2^e with m below 2^24 and -149 <= e <= 104: it is laid into a fixed-point number of
   128 integer and 160 fraction bits, which holds it exactly; the integer part gives its decimal digits by divisions by 10^9, the
   fraction by multiplications by 10^9 (every one takes 9 of its at most 149 binary places away, so it ends).  The first seven
   significant digits and whether anything non-zero follows them decide the rounding to six, half to even; then %g's choice: with
   X the decimal exponent of the ROUNDED value, exponent notation when X < -4 or X >= 6, else fixed; trailing zeros stripped. */
FPL_BAMTAG_HD inline uint32_t fmt_float(uint32_t bits, char* out) {
    uint32_t n = 0;
    const uint32_t ex = (bits >> 23) & 0xFFu, man = bits & 0x7FFFFFu;
    if (bits >> 31) out[n++] = '-';
    if (ex == 0xFFu) {
        const char* w = man ? "nan" : "inf";
        out[n++] = w[0], out[n++] = w[1], out[n++] = w[2];
        return n;
    }
    if (ex == 0 && man == 0) {
        out[n++] = '0';
        return n;
    }
    const uint32_t m = ex ? (man | 0x800000u) : man;
    const uint32_t pos = (ex ? ex : 1u) + 10u; /* e + 160: where bit 0 of m lies, 11 .. 264 */
    uint32_t w[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; /* [0, 5): the fraction, [5, 9): the integer part, little end first */
    {
        const uint32_t k = pos >> 5, s = pos & 31u;
        w[k] = m << s;
        if (s > 8) w[k + 1] = m >> (32 - s); /* (k + 1 <= 8: pos 264 has s == 8) */
    }
    uint32_t dig[7] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t n_sig = 0, zeros = 0;
    int32_t X = 0;
    bool started = false, sticky = false;
    /* the nine digits of a chunk below 10^9, most significant first; int_chunk: its place among the integer part's chunks, -1:
       a chunk of the fraction */
    auto feed = [&](uint32_t chunk, int32_t int_chunk) {
        uint32_t p = 100000000u;
        for (int32_t i = 8; i >= 0; i--, p /= 10) {
            const uint32_t d = chunk / p % 10;
            if (!started) {
                if (d == 0) {
                    if (int_chunk < 0) zeros++;
                    continue;
                }
                started = true;
                X = int_chunk >= 0 ? 9 * int_chunk + i : -(int32_t)(zeros + 1);
            }
            if (n_sig < 7) dig[n_sig++] = d;
            else if (d) sticky = true;
        }
    };
    { /* the integer part: up to 39 digits, five chunks */
        uint32_t c[5];
        for (uint32_t j = 0; j < 5; j++) {
            uint64_t r = 0;
            for (int32_t k = 8; k >= 5; k--) {
                const uint64_t x = (r << 32) | w[k];
                w[k] = (uint32_t)(x / 1000000000u);
                r = x % 1000000000u;
            }
            c[j] = (uint32_t)r;
        }
        for (int32_t j = 4; j >= 0; j--)
            if (started || c[j]) feed(c[j], j);
    }
    /* the fraction: at most 17 chunks until it is used up */
    for (uint32_t step = 0; step < 17 && n_sig < 7 && (w[0] | w[1] | w[2] | w[3] | w[4]); step++) {
        uint64_t carry = 0;
        for (uint32_t k = 0; k < 5; k++) {
            const uint64_t x = (uint64_t)w[k] * 1000000000u + carry;
            w[k] = (uint32_t)x;
            carry = x >> 32;
        }
        feed((uint32_t)carry, -1);
    }
    if (w[0] | w[1] | w[2] | w[3] | w[4]) sticky = true;
    /* six digits, half to even */
    if (dig[6] > 5 || (dig[6] == 5 && (sticky || (dig[5] & 1u)))) {
        int32_t k = 5;
        while (k >= 0 && dig[k] == 9) dig[k--] = 0;
        if (k >= 0) dig[k]++;
        else dig[0] = 1, X++; /* 999999.5 -> 1e+06 */
    }
    uint32_t n_dig = 6;
    while (n_dig > 1 && dig[n_dig - 1] == 0) n_dig--;
    if (X < -4 || X >= 6) {
        out[n++] = (char)('0' + dig[0]);
        if (n_dig > 1) {
            out[n++] = '.';
            for (uint32_t k = 1; k < n_dig; k++) out[n++] = (char)('0' + dig[k]);
        }
        out[n++] = 'e';
        out[n++] = X < 0 ? '-' : '+';
        const uint32_t a = (uint32_t)(X < 0 ? -X : X);
        out[n++] = (char)('0' + a / 10);
        out[n++] = (char)('0' + a % 10);
    } else if (X >= 0) {
        for (uint32_t k = 0; k <= (uint32_t)X; k++) out[n++] = (char)('0' + (k < n_dig ? dig[k] : 0));
        if (n_dig > (uint32_t)X + 1) {
            out[n++] = '.';
            for (uint32_t k = (uint32_t)X + 1; k < n_dig; k++) out[n++] = (char)('0' + dig[k]);
        }
    } else {
        out[n++] = '0', out[n++] = '.';
        for (int32_t k = -1; k > X; k--) out[n++] = '0';
        for (uint32_t k = 0; k < n_dig; k++) out[n++] = (char)('0' + dig[k]);
    }
    return n;
}

/* the text of the value at v of type (or B subtype) t out of cCsSiIf, at out (at most SCALAR_TEXT_MAX bytes) -> its length */
FPL_BAMTAG_HD inline uint32_t scalar_text(uint32_t t, const uint8_t* v, char* out) {
    switch (t) {
        case 'c': return fmt_i32((int8_t)v[0], out);
        case 'C': return fmt_u32(v[0], out);
        case 's': return fmt_i32((int16_t)bamrule::rd16(v), out);
        case 'S': return fmt_u32(bamrule::rd16(v), out);
        case 'i': return fmt_i32((int32_t)bamrule::rd32(v), out);
        case 'I': return fmt_u32(bamrule::rd32(v), out);
        default: return fmt_float(bamrule::rd32(v), out);
    }
}
/* the letter behind the tag in the text: every integer type is written as i */
FPL_BAMTAG_HD inline char text_type(uint32_t t) { return (t == 'c' || t == 'C' || t == 's' || t == 'S' || t == 'i' || t == 'I') ? 'i' : (char)t; }
FPL_BAMTAG_HD inline bool control_byte(uint32_t c) { return c < 0x20u || c == 0x7Fu; }

/* The text of the field of n bytes at f (it parses: bamtag::field_len gave n), tab included, into `sink` --
   sink.put(const char*, uint32_t) takes bytes, sink.copy(const uint8_t*, uint64_t) a run of the field's own.  One thread's form:
   the host's, and what any other form must equal.  false: the field is left out (control bytes), nothing was put */
template <class Sink>
FPL_BAMTAG_HD inline bool field_text(const uint8_t* f, uint64_t n, Sink& sink) {
    const uint32_t t = f[2];
    if (t == 'A' || t == 'Z' || t == 'H') {
        const uint64_t len = t == 'A' ? 1 : n - 4; /* (without the NUL) */
        for (uint64_t k = 0; k < len; k++)
            if (control_byte(f[3 + k])) return false;
    }
    char head[8] = {'\t', (char)f[0], (char)f[1], ':', text_type(t), ':', 0, 0};
    if (t == 'B') {
        head[6] = (char)f[3];
        sink.put(head, 7);
        const uint32_t sub = f[3], sz = bamtag::scalar_size(sub), count = bamrule::rd32(f + 4);
        char e[1 + SCALAR_TEXT_MAX];
        e[0] = ',';
        for (uint32_t k = 0; k < count; k++) sink.put(e, 1 + scalar_text(sub, f + 8 + (uint64_t)k * sz, e + 1));
        return true;
    }
    sink.put(head, 6);
    if (t == 'A') sink.copy(f + 3, 1);
    else if (t == 'Z' || t == 'H') sink.copy(f + 3, n - 4);
    else {
        char e[SCALAR_TEXT_MAX];
        sink.put(e, scalar_text(t, f + 3, e));
    }
    return true;
}

/* what a record's comment amounts to: the four counts of the run's statistics, for one record */
struct Counts {
    uint64_t fields, bytes, left_out;
};
/* The comment of the tag bytes p[0, len) -- a record's, as the tag and modification rules built them: every field parses --
   under the selection, into `sink` */
template <class ZScan, class Sink>
FPL_BAMTAG_HD inline Counts comment_text(const uint8_t* p, uint64_t len, const Selection& sel, const ZScan& zscan, Sink& sink) {
    Counts c = {0, 0, 0};
    if (sel.n == 0) return c;
    for (uint64_t o = 0; o < len;) {
        const uint64_t n = bamtag::field_len(p + o, len - o, zscan);
        if (!n) break;
        if (selected(sel, p + o)) {
            const uint64_t before = sink.size();
            if (field_text(p + o, n, sink)) c.fields++, c.bytes += sink.size() - before;
            else c.left_out++;
        }
        o += n;
    }
    return c;
}

}  // namespace bamcomment
}  // namespace fpl
#endif
