/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bam/libfpl_emu_bam.so, built by tests/emu_bam/build.py).
 *
 * The BAM decode kernel (fastplong_amd/csrc/bam_decode.h) compiled for the host on the lock-step emulator of tests/emu/hip_emu.h,
 * launched the way fpl_process_bam_async / fpl_decode_bam launch it.  The caller's record buffer must hold fpl::BAM_PAD bytes
 * behind its n_bytes, as the library's device buffer does.
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/bam_decode.h"

using namespace fpl;

extern "C" int emu_bam_decode(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, uint32_t n_reads, uint8_t* seq,
                              uint8_t* qual) {
    if (n_reads == 0) return 0;
    u64 word0, n_words;
    bam_words(off[0], off[n_reads], word0, n_words);
    if (!n_words) return 0;
    const u64 blocks = (n_words + BAM_THREADS - 1) / BAM_THREADS;
    emu_launch(k_bam_decode, dim3((unsigned)blocks), dim3(BAM_THREADS), bam, rec_start, off, n_reads, word0, n_words, seq, qual);
    return 0;
}
