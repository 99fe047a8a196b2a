/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_emit/libfpl_emu_emit.so, built by tests/emu_emit/build.py).
 *
 * The emit kernels (fastplong_amd/csrc/emit.h) compiled for the host on the lock-step emulator of tests/emu/hip_emu.h and
 * launched in the order fpl_emit_batch_device launches them, over the caller's arrays as they are: the workspace is the
 * only thing made here.
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/emit.h"

#include <vector>

using namespace fpl;

extern "C" {
/* the arguments of fpl_emit_batch_device without the context and the stream; gather_blocks: the gather's grid (0: as the library
   sizes it for 256 CUs).  returns 0, or -1 for arguments the library refuses */
int emu_emit(const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint32_t n_reads, const fpl_read_result* res, uint8_t* seq_out,
             uint8_t* qual_out, uint64_t out_cap_bytes, uint64_t* off_out, uint32_t out_cap_reads, uint32_t* src, uint8_t* kind,
             fpl_emit_info* info, uint32_t gather_blocks) {
    if (!info) return -1;
    if (n_reads && (!seq || !qual || !off || !res || !seq_out || !qual_out || !off_out)) return -1;
    if (!n_reads) {
        memset(info, 0, sizeof(*info));
        if (off_out) off_out[0] = 0;
        return 0;
    }
    const u32 nblk = (n_reads + EM_LAYOUT_READS - 1) / EM_LAYOUT_READS;
    std::vector<u32> blk_cnt(nblk), blk_max(nblk);
    std::vector<u64> blk_bytes(nblk);
    std::vector<EmitFrom> from(std::min<uint64_t>(2ull * n_reads, out_cap_reads) + 1);
    emu_launch(k_emit_count, dim3(nblk), dim3(EM_LAYOUT_READS), off, res, n_reads, blk_cnt.data(), blk_bytes.data(), blk_max.data());
    emu_launch(k_emit_scan, dim3(1), dim3(EM_SCAN_BLOCKS), blk_cnt.data(), blk_bytes.data(), (const u32*)blk_max.data(), nblk,
               (u64)out_cap_bytes, out_cap_reads, off_out, info);
    emu_launch(k_emit_fill, dim3(nblk), dim3(EM_LAYOUT_READS), off, res, n_reads, (const u32*)blk_cnt.data(), (const u64*)blk_bytes.data(),
               (const fpl_emit_info*)info, off_out, src, kind, from.data());
    const u32 grid = gather_blocks ? gather_blocks : emit_gather_blocks(out_cap_bytes, 256);
    emu_launch(k_emit_gather, dim3(grid), dim3(EM_GATHER_THREADS), seq, qual, (const uint64_t*)off_out, (const EmitFrom*)from.data(),
               (const fpl_emit_info*)info, seq_out, qual_out);
    return 0;
}
uint32_t emu_emit_layout_reads(void) { return EM_LAYOUT_READS; }
uint32_t emu_emit_scan_blocks(void) { return EM_SCAN_BLOCKS; }
uint32_t emu_emit_tile(void) { return EM_TILE; }
uint32_t emu_emit_step(void) { return EM_STEP; }
}
