/*
 * bam_tag_rules.h -- which auxiliary fields of an INPUT BAM record an OUTPUT record keeps (README "BAM output", --keep_tags), for
 * the host's reader and converter (host/bam.cpp, host/bam_out.cpp) and the device's kernels (csrc/bam_tags.h): one text for all,
 * as bam_rules.h and bam_out_rules.h are for the records themselves.  Plain C++, no HIP header needed.
 *
 * The aux region of a record is what lies between its qualities and its end.  A field is two tag bytes, a type byte and a value:
 * A c C one byte, s S two, i I f four, Z H up to and including the first NUL, B a subtype out of cCsSiIf, a little-endian u32
 * count and count values.  The walk takes fields from the front and stops at the first that does not parse (fewer than 3 bytes
 * left, an unknown type or subtype, no NUL before the region's end, a value that runs past it): the PARSED PREFIX is what lies in
 * front of that point.  A field is POSITIONAL when its type is B or its tag is one of MM Mm ML Ml MN: it indexes bases, signal or
 * strand and is wrong as soon as the read is not the read that was sequenced.  An UNCHANGED output record gets the parsed prefix
 * verbatim, a CHANGED one its non-positional fields, in their order, verbatim.
 */
#ifndef FPL_BAM_TAG_RULES_H
#define FPL_BAM_TAG_RULES_H

#include <stdint.h>

#include "bam_rules.h"

#if defined(__HIP__) && !defined(FPL_EMU)
#define FPL_BAMTAG_HD __host__ __device__
#else
#define FPL_BAMTAG_HD
#endif

namespace fpl {
namespace bamtag {

/* bytes of a value of this type or B subtype; 0: not one of cCsSiIf (A is asked for beside it) */
FPL_BAMTAG_HD inline uint32_t scalar_size(uint32_t t) {
    return (t == 'c' || t == 'C') ? 1u : (t == 's' || t == 'S') ? 2u : (t == 'i' || t == 'I' || t == 'f') ? 4u : 0u;
}
/* f: the three bytes in front of a field's value */
FPL_BAMTAG_HD inline bool positional(const uint8_t* f) {
    if (f[2] == 'B') return true;
    return f[0] == 'M' && (f[1] == 'M' || f[1] == 'm' || f[1] == 'L' || f[1] == 'l' || f[1] == 'N');
}
/* the aux region of the record at r (r[0..4) is block_size; the record's fields have passed bamrule::fields_ok): where it
   starts, counted from r, and its bytes */
FPL_BAMTAG_HD inline void region(const uint8_t* r, uint64_t& at, uint64_t& len) {
    const bamrule::Fields f = bamrule::fields(r);
    at = bamrule::qual_offset(f) + f.l_seq;
    const uint64_t end = 4 + (uint64_t)f.bs;
    len = end > at ? end - at : 0;
}
/* the plain scan of a Z / H value: bytes up to and including the first NUL among v[0..left), 0 when there is none */
struct ByteScan {
    FPL_BAMTAG_HD uint64_t operator()(const uint8_t* v, uint64_t left) const {
        for (uint64_t k = 0; k < left; k++)
            if (v[k] == 0) return k + 1;
        return 0;
    }
};
/* bytes of the field at p, of which `left` belong to the region; 0: it does not parse.  zscan: ByteScan, or a faster scan with
   the same answer (it alone may look behind p + left, where its caller knows of padding) */
template <class ZScan>
FPL_BAMTAG_HD inline uint64_t field_len(const uint8_t* p, uint64_t left, const ZScan& zscan) {
    if (left < 3) return 0;
    const uint32_t t = p[2];
    uint64_t n;
    if (t == 'A') n = 4;
    else if (t == 'Z' || t == 'H') {
        const uint64_t z = zscan(p + 3, left - 3);
        if (!z) return 0;
        n = 3 + z;
    } else if (t == 'B') {
        if (left < 8) return 0;
        const uint32_t sz = scalar_size(p[3]);
        if (!sz) return 0;
        n = 8 + (uint64_t)bamrule::rd32(p + 4) * sz;
    } else {
        const uint32_t sz = scalar_size(t);
        if (!sz) return 0;
        n = 3 + sz;
    }
    return n <= left ? n : 0;
}
/* what the walk of a region finds */
struct Walk {
    uint64_t prefix;   /* bytes of the parsed prefix */
    uint64_t kept;     /* ... of its non-positional fields */
    bool positional;   /* it holds a positional field */
    bool whole;        /* the prefix is the whole region: the record parses */
};
template <class ZScan>
FPL_BAMTAG_HD inline Walk walk(const uint8_t* p, uint64_t len, const ZScan& zscan) {
    Walk w = {0, 0, false, false};
    while (w.prefix < len) {
        const uint64_t n = field_len(p + w.prefix, len - w.prefix, zscan);
        if (!n) break;
        if (positional(p + w.prefix)) w.positional = true;
        else w.kept += n;
        w.prefix += n;
    }
    w.whole = w.prefix == len;
    return w;
}
/* an output record is unchanged: the only fragment of its read, all of it, never reverse-complemented, in a run without --mask /
   --break (n_frag, kind, start, len: the fragment's; for --failed_out's record 1, 0 and the trimmed read's) */
FPL_BAMTAG_HD inline bool unchanged(uint32_t n_frag, uint32_t kind, uint64_t start, uint64_t len, uint64_t l_seq, uint32_t flag,
                                    bool fragment_mode) {
    return n_frag == 1 && kind == 0 && start == 0 && len == l_seq && !(flag & 0x10u) && !fragment_mode;
}

}  // namespace bamtag
}  // namespace fpl
#endif
