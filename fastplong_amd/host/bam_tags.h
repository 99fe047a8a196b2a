/*
 * bam_tags.h -- --keep_tags on the host: for every record the formatter writes for a BAM-backed batch, in the order it writes
 * them, the input record its read came from and whether the rule (csrc/bam_tag_rules.h) calls the output record changed.  The
 * formatter (format.cpp) stays as it is: the list is derived from the same results by the same order -- passing fragments in
 * input order for --out, the one failed read for --failed_out -- and bam_out.h's converter takes it beside the text.
 */
#ifndef FPLH_BAM_TAGS_H
#define FPLH_BAM_TAGS_H

#include <vector>

#include "bam_out.h"
#include "fastq.h"

namespace fplh {

/* The sources of the records format_range(b, res, first, last, ..., fl) appends to its `out` (failed == false) or to its `failed`
   (true), appended to `src`.  A batch that is not BAM-backed gives records without a source.  fl: the fragment list of a --break /
   --mask run, in which every record counts as changed.  mods: --keep_mods, the sources say so and carry their fragment's range;
   moves: --keep_moves, the same. */
void bam_tag_sources(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, const FragmentList* fl, bool failed,
                     std::vector<BamTagSrc>& src, bool mods = false, bool moves = false);
/* Every piece's formatted text -> its records with their tags, in place and side by side on the worker pool: `src` holds the
   sources of the records of ALL pieces together, in their order (a piece's share is found by counting its records).  stats: the
   four counts of bam_out.h, added to; mod_stats, move_stats: its four counts of --keep_mods and of --keep_moves, added to (nullptr: not wanted). */
void pieces_to_bam_records(std::vector<std::string>& pieces, const std::vector<BamTagSrc>& src, uint64_t stats[4], uint64_t* mod_stats = nullptr,
                           uint64_t* move_stats = nullptr);

}  // namespace fplh
#endif
