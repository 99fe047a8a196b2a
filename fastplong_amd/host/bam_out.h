/*
 * bam_out.h -- unaligned BAM output (README "BAM output"): the file's fixed header and the record form of formatted FASTQ text.
 * The rules of a record are csrc/bam_out_rules.h's, shared with the device's compose kernels (csrc/bam_emit.h).  What comes out
 * of here is uncompressed; bgzf_into (gzip.h) frames it.
 */
#ifndef FPLH_BAM_OUT_H
#define FPLH_BAM_OUT_H

#include <string>

namespace fplh {

/* magic, l_text, the fixed text, n_ref = 0: the bytes of a BAM file in front of its first record */
const std::string& bam_header_bytes();
/* Formatted FASTQ text (whole records of four lines, as format_batch writes them) -> the records of the rule, appended to out in
   the text's order.  The '+' line's contents are dropped.  out may NOT be text itself. */
void fastq_to_bam_records(const std::string& text, std::string& out);

}  // namespace fplh
#endif
