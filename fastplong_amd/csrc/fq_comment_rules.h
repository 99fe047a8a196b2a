/*
 * fq_comment_rules.h -- how the COMMENT of a FASTQ input's name line -- SAM fields in their text form, tab-separated, as
 * `samtools fastq -T`, a basecaller's FASTQ output and this project's own --comment_tags write them -- follows an output read
 * that is a piece [s, s + n) of its read (README "Comments of a FASTQ input", --reindex_comments): one text for the host's form
 * (host/fq_comments.cpp) and for device code once there is some, as bam_comment_rules.h is for the way there.  Plain C++, no HIP
 * header needed.  The grammar of an MM value, Group, Cut, cut() and digits_of() are bam_mod_rules.h's: an MM value's bytes are the
 * same in a BAM field and in a comment.
 *
 * REGION.  The bytes of the input's name line (without its line end) behind its first TAB.  A line without a TAB -- or whose first
 * byte is one: no reader hands out a record that does not start with '@' -- has no region: every output read gets the formatter's
 * line, and nothing is counted.
 *
 * FIELDS.  The region is split at its TABs.  A field PARSES when it is [A-Za-z][A-Za-z0-9]:T: plus a value (which may be empty),
 * T out of A i f Z H B; for B the value begins with a subtype out of cCsSiIf followed by the field's end or a ','.  Nothing else
 * of a value is looked at.  One field that does not parse -- an empty one from a doubled or trailing TAB included -- and the
 * region IS NOT TAGS: every output read of that input read gets the formatter's line and is counted as left as it is.
 *
 * CHANGED.  An output read is unchanged when it is the only fragment of its read (n_frag 1, kind 0), starts at 0, has the input
 * read's length and the run uses neither --mask nor --break (bamtag::unchanged without a flag: text has no 0x10, the comment is
 * taken to describe the read as the text gives it).  Every other output read is changed.  For --failed_out's record the
 * fragment is the trimmed read.
 *
 * POSITIONAL is a field of type B or of tag MM Mm ML Ml MN Mn.
 *
 * RE-INDEXABLE is an input read of which all of this holds:
 *   run      neither --mask nor --break
 *   fields   exactly one MM|Mm of type Z; exactly one ML|Ml of type B, subtype C; at most one MN|Mn, of type i, its value 1 to 10
 *            decimal digits that give the read's length
 *   grammar  the MM value passes bammod::parse (at most 16 groups, deltas of 1 to 9 digits)
 *   sums     for every group the sum of (delta + 1) is at most the count of its base among the read's bases: a byte counts for
 *            A C G T when (byte & 0xDF) is that letter; N counts every byte
 *   ML       the value behind "B:C" is zero or more of ',' plus 1 to 3 digits, as many as the sum over the groups of deltas x k
 *
 * WHAT AN OUTPUT READ GETS.  Unchanged: the formatter's line.  Changed: the name part in front of the first TAB as the formatter
 * writes it (a split prefix behind the '@'), then the fields in their order, each behind one TAB: a non-positional field
 * verbatim, a positional one not at all -- save that for a re-indexable read the three modification fields stand in their places,
 * rewritten with c0, c1, o_j, j0, j1 as bam_mod_rules.h defines them:
 *   MM   its first 5 bytes, then per group the header, when something is kept ',' and the decimal of o_j0 - c0, the input's bytes
 *        from the comma in front of delta j0 + 1 through the last digit of delta j1 - 1, and ';'
 *   ML   its first 6 bytes, then of every group's share the elements [j0 k, j1 k) with their commas, verbatim
 *   MN   its first 5 bytes and the decimal of n
 * A line never ends in a TAB.
 *
 * --failed_out.  The formatter appends " <failure word>" to the whole line, which would land inside the last field.  For a region
 * that is tags the word goes behind the name part, in front of the first TAB -- where --comment_tags puts it --, for unchanged
 * records too.
 *
 * SIZE.  A rewritten line is never longer than the formatter's: a kept field is the input's; the new first delta of a group has no
 * more digits than the one it replaces (bam_mod_rules.h, SIZE) and every other MM byte is an input byte; the ML elements are a
 * subset of the input's with their own commas; MN's n is at most the read's length, whose decimal the input's value is (leading
 * zeros only make that longer).  The split prefix and the failure word are bytes the formatter's line has too.  So every bound
 * on formatted text -- the gzip output bound, the blocks per stripe of the device's layout -- stands with the switch on.
 */
#ifndef FPL_FQ_COMMENT_RULES_H
#define FPL_FQ_COMMENT_RULES_H

#include <stdint.h>

#include "bam_comment_rules.h"
#include "bam_mod_rules.h"

namespace fpl {
namespace fqcomment {

constexpr uint32_t MN_DIGITS = 10;
constexpr uint32_t ML_DIGITS = 3;

/* ---- fields ---- */
FPL_BAMTAG_HD inline bool type_ok(uint32_t t) { return t == 'A' || t == 'i' || t == 'f' || t == 'Z' || t == 'H' || t == 'B'; }
/* the field f[0, n) (between two TABs, or a TAB and the line's end) parses */
FPL_BAMTAG_HD inline bool field_parses(const uint8_t* f, uint64_t n) {
    if (n < 5 || !bamcomment::tag_bytes_ok(f[0], f[1]) || f[2] != ':' || !type_ok(f[3]) || f[4] != ':') return false;
    if (f[3] != 'B') return true;
    return n >= 6 && bamtag::scalar_size(f[5]) != 0 && (n == 6 || f[6] == ',');
}
/* f: a field that parses */
FPL_BAMTAG_HD inline bool positional(const uint8_t* f) { return f[3] == 'B' || bammod::mm_tag(f) || bammod::ml_tag(f) || bammod::mn_tag(f); }

/* what the walk of a name line finds */
struct Region {
    uint64_t tab;          /* the first TAB (has_tab) */
    bool has_tab;
    bool tags;             /* every field parses */
    bool other_positional; /* a positional field that is none of MM ML MN */
    uint64_t kept;         /* bytes of the non-positional fields, their TABs included */
    bammod::Found fd;      /* the modification fields: a field's first tag byte in the line, its bytes */
};
/* the end of the field that starts at line[at] */
FPL_BAMTAG_HD inline uint64_t field_end(const uint8_t* line, uint64_t len, uint64_t at) {
    while (at < len && line[at] != '\t') at++;
    return at;
}
FPL_BAMTAG_HD inline Region scan(const uint8_t* line, uint64_t len) {
    Region r = {0, false, false, false, 0, bammod::nothing_found()};
    while (r.tab < len && line[r.tab] != '\t') r.tab++;
    if (r.tab == len || r.tab == 0) return r;
    r.has_tab = r.tags = true;
    for (uint64_t a = r.tab + 1; a <= len;) { /* (a == len: the empty field behind a trailing TAB) */
        const uint64_t b = field_end(line, len, a);
        if (!field_parses(line + a, b - a)) {
            r.tags = false;
            return r;
        }
        if (!positional(line + a)) r.kept += b - a + 1;
        else if (!(bammod::mm_tag(line + a) || bammod::ml_tag(line + a) || bammod::mn_tag(line + a))) r.other_positional = true;
        bammod::note(r.fd, line, a, b - a);
        a = b + 1;
    }
    return r;
}
FPL_BAMTAG_HD inline bool unchanged(uint32_t n_frag, uint32_t kind, uint64_t start, uint64_t len, uint64_t l_seq, bool fragment_mode) {
    return bamtag::unchanged(n_frag, kind, start, len, l_seq, 0, fragment_mode);
}

/* ---- re-indexable ---- */
/* the letter a group's 4-bit code counts; 0: every base */
FPL_BAMTAG_HD inline uint32_t code_letter(uint32_t code) { return code == 1 ? 'A' : code == 2 ? 'C' : code == 4 ? 'G' : code == 8 ? 'T' : 0u; }
/* bases of code `code` among the first `to` of the text bases at s */
FPL_BAMTAG_HD inline uint64_t count_bases(const uint8_t* s, uint64_t to, uint32_t code) {
    const uint32_t letter = code_letter(code);
    if (!letter) return to;
    uint64_t c = 0;
    for (uint64_t i = 0; i < to; i++) c += (s[i] & 0xDFu) == letter;
    return c;
}
/* the ML value v[0, len) behind "XX:B:C": zero or more of ',' and 1 to 3 digits -> how many; false: it is not that */
FPL_BAMTAG_HD inline bool ml_elements(const uint8_t* v, uint64_t len, uint64_t& count) {
    count = 0;
    for (uint64_t at = 0; at < len;) {
        if (v[at] != ',') return false;
        uint64_t e = at + 1;
        while (e < len && bammod::digit(v[e])) e++;
        if (e - at - 1 < 1 || e - at - 1 > ML_DIGITS) return false;
        count++;
        at = e;
    }
    return true;
}
/* where element e of such a value starts (its comma); len for the element behind the last.  from, from_e: a place the walk has
   been before (an element's comma and its number), 0 and 0 to start */
FPL_BAMTAG_HD inline uint64_t ml_element_at(const uint8_t* v, uint64_t len, uint64_t e, uint64_t from, uint64_t from_e) {
    uint64_t at = from;
    for (; from_e < e && at < len; from_e++) {
        at++;
        while (at < len && v[at] != ',') at++;
    }
    return at;
}
/* the MN field f[0, n): type i and 1 to 10 digits that give l_seq */
FPL_BAMTAG_HD inline bool mn_ok(const uint8_t* f, uint64_t n, uint64_t l_seq) {
    if (f[3] != 'i' || n < 6 || n > 5 + MN_DIGITS) return false;
    uint64_t x = 0;
    for (uint64_t k = 5; k < n; k++) {
        if (!bammod::digit(f[k])) return false;
        x = 10 * x + (f[k] - '0');
    }
    return x == l_seq;
}
/* line: the input's name line, rg: its scan (tags), bases: the read's l_seq input bases.  true: the read is re-indexable, and R
   says how (R.fd: the fields in the line; a group's ml_at counts ML elements) */
FPL_BAMTAG_HD inline bool reindexable(const uint8_t* line, const Region& rg, const uint8_t* bases, uint64_t l_seq, bool fragment_mode,
                                      bammod::Record& R) {
    const bammod::Found& fd = rg.fd;
    if (fragment_mode || fd.n_mm != 1 || fd.n_ml != 1 || fd.n_mn > 1) return false;
    if (line[fd.mm_at + 3] != 'Z' || line[fd.ml_at + 3] != 'B' || line[fd.ml_at + 5] != 'C') return false;
    if (fd.n_mn && !mn_ok(line + fd.mn_at, fd.mn_len, l_seq)) return false;
    if (fd.mm_len - 5 > 0xFFFFFFF0ull) return false;
    R.fd = fd;
    if (!bammod::parse(line + fd.mm_at + 5, (uint32_t)(fd.mm_len - 5), R.g, R.n_groups)) return false;
    uint32_t want = 0; /* which counts the groups ask for */
    for (uint32_t k = 0; k < R.n_groups; k++) want |= 1u << bammod::code_slot(R.g[k].code);
    for (uint32_t s = 0; s < 5; s++) R.total[s] = (want >> s & 1u) ? count_bases(bases, l_seq, s < 4 ? 1u << s : 0u) : 0;
    uint64_t ml = 0, have = 0;
    for (uint32_t k = 0; k < R.n_groups; k++) {
        if (R.g[k].sum > R.total[bammod::code_slot(R.g[k].code)]) return false;
        ml += (uint64_t)R.g[k].n_delta * R.g[k].k;
    }
    return ml_elements(line + fd.ml_at + 6, fd.ml_len - 6, have) && have == ml;
}

/* ---- the text ---- */
/* the five counts of the run's statistics */
struct Counts {
    uint64_t reindexed; /* output reads re-indexed */
    uint64_t lost;      /* changed output reads of reads with modification fields that were not re-indexable and lost them */
    uint64_t kept, cut; /* modification positions kept, cut away */
    uint64_t left;      /* output reads whose line was left as it is: the region is not tags */
};
/* The fields of a CHANGED output read [s, s + n) of the read with this line, every one behind its TAB, into `sink` --
   sink.put(const char*, uint32_t) takes bytes, sink.copy(const uint8_t*, uint64_t) a run of the line's own.  R: the read is
   re-indexable (nullptr: it is not, the positional fields go) */
template <class Sink>
FPL_BAMTAG_HD inline void fields_text(const uint8_t* line, uint64_t len, const Region& rg, const bammod::Record* R, const uint8_t* bases, uint64_t s,
                                      uint64_t n, Sink& sink, Counts& c) {
    bammod::Cut cuts[bammod::MAX_GROUPS];
    const uint8_t* v = nullptr;
    if (R) {
        v = line + R->fd.mm_at + 5;
        const uint32_t v_len = (uint32_t)(R->fd.mm_len - 5);
        uint64_t c0[5], c1[5];
        bool have[5] = {false, false, false, false, false};
        for (uint32_t k = 0; k < R->n_groups; k++) {
            const bammod::Group& g = R->g[k];
            const uint32_t slot = bammod::code_slot(g.code);
            if (!have[slot]) /* (one walk of [0, s + n) a slot) */
                c0[slot] = count_bases(bases, s, g.code), c1[slot] = c0[slot] + count_bases(bases + s, n, g.code), have[slot] = true;
            cuts[k] = bammod::cut(v, v_len, g, c0[slot], c1[slot]);
            c.kept += cuts[k].j1 - cuts[k].j0, c.cut += g.n_delta - (cuts[k].j1 - cuts[k].j0);
        }
    }
    for (uint64_t a = rg.tab + 1; a <= len;) {
        const uint64_t b = field_end(line, len, a);
        const uint8_t* f = line + a;
        if (R && a == R->fd.mm_at) {
            sink.copy(f - 1, 6);
            for (uint32_t k = 0; k < R->n_groups; k++) {
                sink.copy(v + R->g[k].at, R->g[k].hdr_len);
                if (cuts[k].j1 > cuts[k].j0) {
                    char e[11];
                    e[0] = ',';
                    sink.put(e, 1 + bamcomment::fmt_u32(cuts[k].first, e + 1));
                    sink.copy(v + cuts[k].rest_at, cuts[k].rest_end - cuts[k].rest_at);
                }
                sink.put(";", 1);
            }
        } else if (R && a == R->fd.ml_at) {
            sink.copy(f - 1, 7);
            const uint8_t* m = f + 6;
            const uint64_t m_len = b - a - 6;
            uint64_t at = 0, at_e = 0; /* the walk only goes forward: the groups' shares follow one another */
            for (uint32_t k = 0; k < R->n_groups; k++) {
                const uint64_t e0 = R->g[k].ml_at + (uint64_t)cuts[k].j0 * R->g[k].k, e1 = R->g[k].ml_at + (uint64_t)cuts[k].j1 * R->g[k].k;
                if (e1 == e0) continue;
                const uint64_t p0 = ml_element_at(m, m_len, e0, at, at_e), p1 = ml_element_at(m, m_len, e1, p0, e0);
                sink.copy(m + p0, p1 - p0);
                at = p1, at_e = e1;
            }
        } else if (R && R->fd.n_mn && a == R->fd.mn_at) {
            sink.copy(f - 1, 6);
            char e[10];
            sink.put(e, bamcomment::fmt_u32((uint32_t)n, e));
        } else if (!positional(f))
            sink.copy(f - 1, b - a + 1);
        a = b + 1;
    }
}
/* The name line of one output read into `sink`.  fmt[0, fmt_len): the line the formatter wrote for it -- the input's line with a
   split prefix behind its first byte, or, failed, with " <failure word>" behind it --; line[0, len): the input's line; bases: the
   read's l_seq input bases; [s, s + n): the output read's range, changed: the rule's verdict on it.  One thread's form: the
   host's, and what any other form must equal */
template <class Sink>
FPL_BAMTAG_HD inline void line_text(const uint8_t* fmt, uint64_t fmt_len, const uint8_t* line, uint64_t len, const uint8_t* bases, uint64_t l_seq,
                                    uint64_t s, uint64_t n, bool changed, bool failed, bool fragment_mode, Sink& sink, Counts& c) {
    const Region rg = fmt_len >= len ? scan(line, len) : Region{0, false, false, false, 0, bammod::nothing_found()};
    if (!rg.has_tab || !rg.tags) {
        if (rg.has_tab) c.left++;
        sink.copy(fmt, fmt_len);
        return;
    }
    if (failed) sink.copy(fmt, rg.tab), sink.copy(fmt + len, fmt_len - len);
    else sink.copy(fmt, rg.tab + (fmt_len - len));
    if (!changed) {
        sink.copy(line + rg.tab, len - rg.tab);
        return;
    }
    bammod::Record R;
    bool mods = false;
    if (bammod::any_found(rg.fd)) {
        mods = reindexable(line, rg, bases, l_seq, fragment_mode, R);
        if (mods) c.reindexed++;
        else c.lost++;
    }
    fields_text(line, len, rg, mods ? &R : nullptr, bases, s, n, sink, c);
}

}  // namespace fqcomment
}  // namespace fpl
#endif
