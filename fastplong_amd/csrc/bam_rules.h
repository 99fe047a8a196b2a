/*
 * bam_rules.h -- the checks of ONE BAM record, for the host's walk (host/bam.cpp, BamReader::walk) and the device's
 * (csrc/bam_walk.h): one text for both, as adapter_pick.h is for the adapter detection.  Plain C++, no HIP header needed.
 *
 * A record is block_size (4 bytes) and block_size bytes behind it; 32 of those are fixed fields: l_read_name at +12,
 * n_cigar_op at +16, flag at +18, l_seq at +20 (offsets from the block_size field), the name at +36.
 */
#ifndef FPL_BAM_RULES_H
#define FPL_BAM_RULES_H

#include <stdint.h>
#include <string.h>

#if defined(__HIP__) && !defined(FPL_EMU)
#define FPL_BAMRULE_HD __host__ __device__
#else
#define FPL_BAMRULE_HD
#endif

namespace fpl {
namespace bamrule {

constexpr uint64_t MAX_TAG_BYTES = 256u << 20; /* tags may follow the fields, but not more than this + 16 bytes for every byte of them */
constexpr uint32_t HEAD = 36;                  /* block_size and the fixed fields: what a walk reads of a record before it trusts it */
constexpr uint32_t MIN_BLOCK_SIZE = 32;

struct Fields {
    uint32_t bs, l_name, n_cigar, flag, l_seq;
};

FPL_BAMRULE_HD inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
FPL_BAMRULE_HD inline uint32_t rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

/* r: HEAD readable bytes */
FPL_BAMRULE_HD inline Fields fields(const uint8_t* r) {
    Fields f;
    f.bs = rd32(r);
    f.l_name = r[12];
    f.n_cigar = rd16(r + 16);
    f.flag = rd16(r + 18);
    f.l_seq = rd32(r + 20);
    return f;
}
/* bytes of block_size the fields account for */
FPL_BAMRULE_HD inline uint64_t fixed_len(const Fields& f) {
    return 32 + (uint64_t)f.l_name + 4 * (uint64_t)f.n_cigar + ((uint64_t)f.l_seq + 1) / 2 + f.l_seq;
}
FPL_BAMRULE_HD inline bool block_size_ok(uint32_t bs) { return bs >= MIN_BLOCK_SIZE; }
/* block_size agrees with the fields (block_size_ok asked before) */
FPL_BAMRULE_HD inline bool fields_ok(const Fields& f) {
    const uint64_t fixed = fixed_len(f);
    return f.l_name >= 1 && f.l_seq <= 0x7FFFFFFFu && fixed <= (uint64_t)f.bs && (uint64_t)f.bs - fixed <= MAX_TAG_BYTES + 16 * fixed;
}
FPL_BAMRULE_HD inline bool skipped(uint32_t flag) { return (flag & 0x900u) != 0; } /* secondary / supplementary: not part of the twin */
FPL_BAMRULE_HD inline bool paired(uint32_t flag) { return (flag & 0x1u) != 0; }
/* where the qualities start, from the block_size field */
FPL_BAMRULE_HD inline uint64_t qual_offset(const Fields& f) {
    return HEAD + (uint64_t)f.l_name + 4 * (uint64_t)f.n_cigar + ((uint64_t)f.l_seq + 1) / 2;
}
FPL_BAMRULE_HD inline bool no_qualities(const Fields& f, uint8_t first_qual) { return f.l_seq > 0 && first_qual == 0xFF; }

}  // namespace bamrule
}  // namespace fpl
#endif
