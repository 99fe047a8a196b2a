/*
 * fq_comments.h -- --reindex_comments on the host (README "Comments of a FASTQ input"): the SAM fields a FASTQ input carries as
 * comments of its name lines follow every trim and split into the formatted FASTQ text, by csrc/fq_comment_rules.h.  The sibling
 * of bam_comments.h: the formatter stays as it is, the list of where every record of the text came from is derived from the same
 * results by the same order (as bam_tags.h derives BamTagSrc), and the name lines are rewritten in front of the deflate / BGZF
 * framing.
 */
#ifndef FPLH_FQ_COMMENTS_H
#define FPLH_FQ_COMMENTS_H

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "fastq.h"

namespace fplh {

/* where record k of a formatted text came from: the input read's name line (without its line end) and bases, the output read's
   range in them, the rule's verdict on it, and whether it is --failed_out's record (the formatter put a failure word behind the
   line) */
struct FqCommentSrc {
    const char* name;
    uint32_t name_len;
    const uint8_t* seq;
    uint32_t l_seq;
    uint32_t start, len;
    bool changed, failed, fragment_mode;
};
/* The sources of the records format_range(b, res, first, last, ..., fl) appends to its `out` (failed == false) or to its `failed`
   (true), appended to `src`; they point into the batch.  fl: the fragment list of a --break / --mask run, in which every record is
   changed and nothing is re-indexed */
void fq_comment_sources(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, const FragmentList* fl, bool failed,
                        std::vector<FqCommentSrc>& src);
/* One formatted text (whole records of four lines): record k's name line becomes the rule's line for src[k] (k >= n_src: the text
   is kept).  stats (5 counts, added to): output reads re-indexed, changed output reads whose modification fields were not
   re-indexable and went, modification positions kept, positions cut away, output reads left as they are (the region is not tags) */
void reindex_comments(std::string& text, const FqCommentSrc* src, size_t n_src, uint64_t stats[5]);
/* the same for every piece of a batch's formatted text, in place and side by side on the worker pool: `src` holds the sources of
   the records of ALL pieces together, in their order (a piece's share is found by counting its records) */
void pieces_reindex_comments(std::vector<std::string>& pieces, const std::vector<FqCommentSrc>& src, uint64_t stats[5]);

}  // namespace fplh
#endif
