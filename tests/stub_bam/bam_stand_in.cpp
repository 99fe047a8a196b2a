/*
 * bam_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_bam/libfastplong_amd.so, built by tests/stub_bam/build.py).
 *
 * The two BAM entry points of ABI v8 for the CPU stand-in of tests/stub (fpl_stub.cpp, unchanged, linked beside this file):
 * fpl_process_bam_async decodes the records into the caller's arrays at submission -- the twin rule of README "BAM input",
 * written out plainly here, independent of the device kernel -- and hands the decoded batch to fpl_process_batch_async, so
 * the CLI's BAM path (reader, submission, formatting from the decoded arrays) runs on a box without GPUs.
 */
#include <string.h>

#include "../../include/fastplong_amd.h"

static void decode(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, uint32_t n, uint8_t* seq, uint8_t* qual) {
    static const char codes[] = "=ACMGRSVTWYHKDBN", comp[] = "=TGKCYSBAWRDMHVN";
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* r = bam + rec_start[i];
        const uint32_t l_name = r[12], n_cigar = r[16] | (r[17] << 8), flag = r[18] | (r[19] << 8);
        const uint64_t l = off[i + 1] - off[i];
        const uint8_t* sq = r + 36 + l_name + 4 * n_cigar;
        const uint8_t* ql = sq + (l + 1) / 2;
        for (uint64_t j = 0; j < l; j++) {
            const uint64_t k = (flag & 0x10) ? l - 1 - j : j;
            const int c = (k & 1) ? (sq[k >> 1] & 15) : (sq[k >> 1] >> 4);
            seq[off[i] + j] = (uint8_t)((flag & 0x10) ? comp[c] : codes[c]);
            qual[off[i] + j] = (uint8_t)((ql[k] > 93 ? 93 : ql[k]) + 33);
        }
    }
}

extern "C" int fpl_process_bam_async(fpl_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                                     uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out, fpl_read_result* results) {
    (void)n_bytes;
    if (n_reads) decode(bam, rec_start, off, n_reads, seq_out, qual_out);
    return fpl_process_batch_async(ctx, seq_out, qual_out, off, n_reads, results);
}

extern "C" int fpl_decode_bam(int32_t device, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                              uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out) {
    (void)device;
    (void)n_bytes;
    if (n_reads) decode(bam, rec_start, off, n_reads, seq_out, qual_out);
    return FPL_OK;
}
