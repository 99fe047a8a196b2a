/*
 * bam_out_rules.h -- the rules of ONE unaligned BAM record on the OUTPUT side (README "BAM output"), for the host's converter
 * (host/bam_out.cpp) and the device's compose kernels (csrc/bam_emit.h): one text for both, as bam_rules.h is for the input side.
 * Plain C++, no HIP header needed.
 *
 * A record is the 36 fixed bytes (block_size, refID -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag 4, l_seq,
 * next_refID -1, next_pos -1, tlen 0), the name with its NUL, (l_seq + 1) / 2 bytes of packed bases (high nibble first, the last
 * low nibble 0 when l_seq is odd) and l_seq quality bytes.  No tags -- unless the run keeps the input BAM's (--keep_tags): then the
 * bytes csrc/bam_tag_rules.h picks follow the qualities and block_size counts them.
 */
#ifndef FPL_BAM_OUT_RULES_H
#define FPL_BAM_OUT_RULES_H

#include <stdint.h>

#if defined(__HIP__) && !defined(FPL_EMU)
#define FPL_BAMOUT_HD __host__ __device__
#else
#define FPL_BAMOUT_HD
#endif

namespace fpl {
namespace bamout {

constexpr uint32_t FIXED = 36;     /* block_size and the fixed fields */
constexpr uint32_t NAME_BYTES = 254; /* bytes of a name: l_read_name is one byte and counts the NUL */
constexpr uint32_t BIN = 4680;     /* reg2bin(-1, 0): what every unmapped record carries */
constexpr uint32_t FLAG = 4;       /* unmapped */
/* the file's header, uncompressed: magic, l_text, the text, n_ref = 0.  Fixed, so that a file is a function of its reads alone */
#define FPL_BAMOUT_HEADER_HD "@HD\tVN:1.6\tSO:unknown\n"
#define FPL_BAMOUT_HEADER_PG "@PG\tID:fastplong_amd\tPN:fastplong_amd\n"
#define FPL_BAMOUT_HEADER_TEXT FPL_BAMOUT_HEADER_HD FPL_BAMOUT_HEADER_PG /* (--keep_tags: the input's @RG lines between the two) */

/* htslib's seq_nt16_table: '=' -> 0, the letters of "=ACMGRSVTWYHKDBN" in either case -> their code, every other byte -> 15.
   A letter's code is nibble (c & 31) of the two constants (letters outside the alphabet hold 15 there, and so do the five
   places around the letters: '@', '[' .. '_', '`', '{' .. DEL). */
FPL_BAMOUT_HD inline uint32_t base_code(uint32_t c) {
    c &= 0xFFu;
    if (c == (uint32_t)'=') return 0u;
    if ((c & 0xC0u) != 0x40u) return 15u;
    const uint64_t nib = (c & 16u) ? 0xFFFFFFAF97F865FFull : 0xFF3FCFFB4FFD2E1Full;
    return (uint32_t)(nib >> (4u * (c & 15u))) & 15u;
}
/* the 256-entry table of base_code: what the host's converter and the device's LDS copy hold */
inline void base_table(uint8_t t[256]) {
    for (uint32_t c = 0; c < 256; c++) t[c] = (uint8_t)base_code(c);
}
/* a quality byte of the FASTQ text -> the phred value of the record */
FPL_BAMOUT_HD inline uint32_t qual_code(uint32_t q) { return (q > 33u ? q : 33u) - 33u; }

/* The name: `prefix` bytes the formatter puts in front ("split-by-adapter-left-": never a space or tab in them) and the name line's
   bytes behind its '@' (rest, rest_len).  It is cut at the first space or tab, then truncated to NAME_BYTES bytes.
   name_cut: how many bytes of rest stay; name_len: the bytes of the record's name -- what is left empty becomes "*". */
FPL_BAMOUT_HD inline bool name_ends(uint32_t c) { return c == (uint32_t)' ' || c == (uint32_t)'\t'; }
FPL_BAMOUT_HD inline uint32_t name_room(uint32_t prefix) { return prefix < NAME_BYTES ? NAME_BYTES - prefix : 0u; }
FPL_BAMOUT_HD inline uint32_t name_cut(const uint8_t* rest, uint32_t rest_len, uint32_t prefix) {
    const uint32_t room = name_room(prefix), cap = rest_len < room ? rest_len : room;
    uint32_t n = 0;
    while (n < cap && !name_ends(rest[n])) n++;
    return n;
}
FPL_BAMOUT_HD inline uint32_t name_len(uint32_t prefix, uint32_t cut) {
    const uint32_t n = (prefix < NAME_BYTES ? prefix : NAME_BYTES) + cut;
    return n ? n : 1u;
}
/* a record's bytes from (name length, bases); block_size is this minus 4 */
FPL_BAMOUT_HD inline uint64_t record_len(uint32_t name_len, uint64_t l_seq) {
    return (uint64_t)FIXED + name_len + 1u + (l_seq + 1u) / 2u + l_seq;
}
/* word k (0..8) of the 36 fixed bytes, little-endian */
FPL_BAMOUT_HD inline uint32_t fixed_word(uint32_t k, uint32_t name_len, uint32_t l_seq) {
    return k == 0 ? (uint32_t)(record_len(name_len, l_seq) - 4u)
         : k == 3 ? (name_len + 1u) | (BIN << 16) /* l_read_name, mapq 0, bin */
         : k == 4 ? FLAG << 16                     /* n_cigar_op 0, flag */
         : k == 5 ? l_seq
         : k == 8 ? 0u                             /* tlen */
                  : 0xFFFFFFFFu;                   /* refID, pos, next_refID, next_pos */
}

}  // namespace bamout
}  // namespace fpl
#endif
