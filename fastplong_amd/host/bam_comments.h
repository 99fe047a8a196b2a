/*
 * bam_comments.h -- --comment_tags on the host (README "Tags as FASTQ comments"): the auxiliary fields of the input record behind
 * every name line of a BAM-backed batch's formatted FASTQ text, by csrc/bam_comment_rules.h.  The sibling of bam_tags.h's
 * pieces_to_bam_records: the same source lists (bam_tag_sources with mods on), the same tag bytes (bam_out.h's
 * bam_record_tags), written as SAM text in place of BAM bytes.  The formatter (format.cpp) stays as it is; this runs behind it
 * and in front of the deflate.
 */
#ifndef FPLH_BAM_COMMENTS_H
#define FPLH_BAM_COMMENTS_H

#include <string>
#include <vector>

#include "../csrc/bam_comment_rules.h"
#include "bam_out.h"

namespace fplh {

using BamCommentSelection = fpl::bamcomment::Selection;

/* --comment_tags LIST: "*" or "MM,ML,..." -> the selection; false: a malformed list (empty, an item that is not two bytes out of
   [A-Za-z][A-Za-z0-9], more than 32 items) */
bool parse_comment_tags(const std::string& list, BamCommentSelection& sel);
/* One formatted text (whole records of four lines): record k's name line gets the comment of src[k] (k >= n_src, or a source
   without a record: nothing), in place.  stats (4 counts, added to): output records that got at least one field, fields written,
   comment bytes (tabs included), fields left out for control bytes */
void add_tag_comments(std::string& text, const BamTagSrc* src, size_t n_src, const BamCommentSelection& sel, uint64_t stats[4]);
/* Every piece's text, in place and side by side on the worker pool: `src` holds the sources of the records of ALL pieces together,
   in their order (bam_tag_sources(..., mods = true)); a piece's share is found by counting its records */
void pieces_add_tag_comments(std::vector<std::string>& pieces, const std::vector<BamTagSrc>& src, const BamCommentSelection& sel, uint64_t stats[4]);

}  // namespace fplh
#endif
