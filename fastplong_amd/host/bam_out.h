/*
 * bam_out.h -- unaligned BAM output (README "BAM output"): the file's fixed header and the record form of formatted FASTQ text.
 * The rules of a record are csrc/bam_out_rules.h's, shared with the device's compose kernels (csrc/bam_emit.h).  What comes out
 * of here is uncompressed; bgzf_into (gzip.h) frames it.
 *
 * --keep_tags: the header also carries the input's @RG lines, and a record the auxiliary fields of the input record its read
 * came from, picked by csrc/bam_tag_rules.h.  Which input record that is the text does not say: the caller names it, record by
 * record in the text's order (host/bam_tags.h derives the list from a batch's results).
 *
 * --keep_mods: a changed record of a re-indexable input record (csrc/bam_mod_rules.h) gets its MM / ML / MN fields rewritten for
 * its piece of the read in place of losing them.
 *
 * --keep_moves: the same for the move table mv and its ts (csrc/bam_move_rules.h); either switch decides its own fields.
 */
#ifndef FPLH_BAM_OUT_H
#define FPLH_BAM_OUT_H

#include <stddef.h>
#include <stdint.h>

#include <string>

namespace fplh {

/* magic, l_text, the fixed text, n_ref = 0: the bytes of a BAM file in front of its first record */
const std::string& bam_header_bytes();
/* the same with `read_groups` -- whole "@RG\t...\n" lines, as bam_read_group_lines gives them -- between the @HD and the @PG line */
std::string bam_header_bytes(const std::string& read_groups);
/* every line of a BAM header's text (taken to end at its first NUL, if it has one) that starts with "@RG\t", verbatim and in
   order, a '\n' added where the last one lacks it */
std::string bam_read_group_lines(const std::string& header_text);
/* Formatted FASTQ text (whole records of four lines, as format_batch writes them) -> the records of the rule, appended to out in
   the text's order.  The '+' line's contents are dropped.  out may NOT be text itself. */
void fastq_to_bam_records(const std::string& text, std::string& out);

/* where record k of a text takes its auxiliary fields from: the input record (its block_size field; the record has passed the
   reader's checks and all of it is readable), or nullptr for none; changed: csrc/bam_tag_rules.h's verdict on the output record */
struct BamTagSrc {
    const uint8_t* rec;
    bool changed;
    /* --keep_mods (csrc/bam_mod_rules.h): the record is the bases [start, start + len) of its read; mods: the switch is on;
       fragment_mode: a --break / --mask run, in which no record is re-indexable */
    uint32_t start = 0, len = 0;
    bool mods = false, fragment_mode = false;
    bool moves = false; /* --keep_moves (csrc/bam_move_rules.h): the switch is on */
    BamTagSrc(const uint8_t* r, bool c) : rec(r), changed(c) {}
    BamTagSrc(const uint8_t* r, bool c, uint32_t s, uint32_t n, bool m, bool fm, bool mv = false)
        : rec(r), changed(c), start(s), len(n), mods(m), fragment_mode(fm), moves(mv) {}
};
/* the same with tags: record k of the text gets what the rule picks of src[k] (k >= n_src: nothing).  stats (4 counts, added to):
   records that kept every field of their parsed prefix, records that lost positional fields, tag bytes written, records whose
   region did not parse to its end.  mod_stats (4 counts, added to; only sources with `mods` move them): records re-indexed, changed
   records whose modification fields were not re-indexable and went the old way, modification positions kept, positions cut away.
   move_stats (the same for sources with `moves`): records re-indexed, changed records with a table that was not re-indexable, table
   entries kept, entries cut away */
void fastq_to_bam_records(const std::string& text, const BamTagSrc* src, size_t n_src, std::string& out, uint64_t* stats,
                          uint64_t* mod_stats = nullptr, uint64_t* move_stats = nullptr);
/* what the rules pick of the input record of s (s.rec is not nullptr) -- the tag bytes of its output record --, appended to out
   -> the bytes appended; stats, mod_stats, move_stats: as above, nullptr for not wanted */
uint64_t bam_record_tags(const BamTagSrc& s, std::string& out, uint64_t* stats, uint64_t* mod_stats, uint64_t* move_stats = nullptr);
/* records of a formatted text: a quarter of its line ends */
size_t fastq_record_count(const std::string& text);

}  // namespace fplh
#endif
