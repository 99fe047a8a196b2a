/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bamgz/libfpl_emu_bamgz.so, built by tests/emu_bamgz/build.py).
 *
 * The BAM forms of the gzip layout and compose kernels (fastplong_amd/csrc/gz_emit.h) behind the decode kernel
 * (fastplong_amd/csrc/bam_decode.h), and the unchanged block kernels behind them, compiled for the host on the lock-step emulator
 * of tests/emu/hip_emu.h and launched in the order fpl_process_bam_async / fpl_wait_bam_gz launch them.  The caller's record buffer
 * must hold fpl::BAM_PAD bytes behind its n_bytes, as the library's device buffer does.
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/gz_emit.h"
#include "../../fastplong_amd/csrc/bam_decode.h"

#include <vector>

using namespace fpl;

extern "C" {
/* the decode kernel alone, as fpl_decode_bam launches it (seq / qual: off[n_rec] bytes rounded up to 16, and 16 more) */
int emu_bamgz_decode(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, uint32_t n_rec, uint8_t* seq, uint8_t* qual) {
    if (n_rec == 0) return 0;
    u64 word0, n_words;
    bam_words(off[0], off[n_rec], word0, n_words);
    if (n_words)
        emu_launch(k_bam_decode, dim3((unsigned)((n_words + BAM_THREADS - 1) / BAM_THREADS)), dim3(BAM_THREADS), bam, rec_start, off, n_rec, word0,
                   n_words, seq, qual);
    return 0;
}
/* info: total, gz_len, n_blocks, crc.  blk_out (optional): n_blocks + 1 block starts, at most blk_out_cap of them are written.
   returns 0, -2 when out is too small, -3 when the kernels report a status */
int emu_bamgz_emit(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, const fpl_read_result* res, uint32_t n_rec,
                   uint8_t* out, uint64_t out_cap, uint64_t* info, uint8_t* comp_out, uint64_t* blk_out, uint64_t blk_out_cap) {
    const u64 n_bases = n_rec ? off[n_rec] : 0;
    std::vector<u8> seq((size_t)n_bases + 32), qual((size_t)n_bases + 32);
    emu_bamgz_decode(bam, rec_start, off, n_rec, seq.data(), qual.data());
    const u32 blk_cap = (u32)gz_bam_blocks_bound(n_bases, n_rec);
    std::vector<u64> rec_off((size_t)n_rec + 1), blk_start((size_t)blk_cap + 1);
    GzHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    emu_launch(k_gz_layout_bam, dim3(1), dim3(1024), bam, rec_start, (const u8*)seq.data(), (const u8*)qual.data(), off, res, n_rec,
               rec_off.data(), blk_start.data(), blk_cap, &hdr);
    if (hdr.status) return -3;
    std::vector<u8> comp((size_t)hdr.total + 16);
    if (n_rec)
        emu_launch(k_gz_compose_bam, dim3(2), dim3(256), bam, rec_start, (const u8*)seq.data(), (const u8*)qual.data(), off, res, n_rec,
                   (const u64*)rec_off.data(), comp.data(), (u64)hdr.total);
    if (comp_out) memcpy(comp_out, comp.data(), (size_t)hdr.total);
    info[0] = hdr.total;
    info[1] = 0;
    info[2] = hdr.n_blocks;
    info[3] = 0;
    if (blk_out)
        for (u64 k = 0; k <= hdr.n_blocks && k < blk_out_cap; k++) blk_out[k] = blk_start[(size_t)k];
    if (GZ_MEMBER_EXTRA + hdr.total + (u64)GZ_SLACK * hdr.n_blocks > out_cap) return -2;
    const u32 nb = hdr.n_blocks;
    std::vector<u8> tmp((size_t)(hdr.total + (u64)GZ_SLACK * nb + 16));
    std::vector<u32> blk_size(nb + 1), blk_crc(nb + 1);
    std::vector<u64> blk_off(nb + 1);
    if (nb)
        emu_launch(k_gz_block, dim3(std::min<u32>(nb, 3)), dim3(GZ_THREADS), (const u8*)comp.data(), (const u64*)blk_start.data(),
                   (const GzHeader*)&hdr, tmp.data(), blk_size.data(), blk_crc.data());
    emu_launch(k_gz_finish, dim3(1), dim3(1024), (const u32*)blk_size.data(), (const u32*)blk_crc.data(), blk_off.data(), &hdr, out, out_cap);
    if (nb)
        emu_launch(k_gz_compact, dim3(std::min<u32>(nb, 3)), dim3(GZ_THREADS), (const u8*)tmp.data(), (const u64*)blk_start.data(),
                   (const u32*)blk_size.data(), (const u64*)blk_off.data(), (const GzHeader*)&hdr, out, out_cap);
    info[1] = hdr.gz_len;
    info[3] = hdr.crc;
    return hdr.status ? -3 : 0;
}
uint32_t emu_bamgz_block_bytes(void) { return GZ_B; }
uint32_t emu_bamgz_long_line(void) { return GZ_L; }
uint32_t emu_bamgz_pad(void) { return BAM_PAD; }
}
