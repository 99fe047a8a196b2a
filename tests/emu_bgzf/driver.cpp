/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bgzf/emu_bgzf_run and the object tests/stub_bgzf links; tests/emu_bgzf/build.py).
 *
 * k_bgzf_inflate (fastplong_amd/csrc/bgzf_inflate.h) compiled for the host on the lock-step emulator of tests/emu/hip_emu.h.
 * emu_bgzf_inflate is what fpl_inflate_bgzf does behind its range checks: one launch over the descriptors.
 * With EMU_BGZF_MAIN the file is a program, built with -fsanitize=address,undefined: it reads a job (see build.py), POISONS every
 * byte of comp and out that no descriptor covers, runs the kernel and writes the descriptors and out back -- so a read outside a
 * block's payload or a write outside its output range ends the program with a sanitizer report instead of going unseen.
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/bgzf_inflate.h"

#include <vector>

using namespace fpl;

extern "C" int emu_bgzf_inflate(const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                                uint64_t out_bytes, uint32_t grid) {
    for (uint32_t i = 0; i < n_blocks; i++) {
        const fpl_bgzf_block& d = blocks[i];
        if (d.comp_len > BGZF_MAX_COMP || d.isize > BGZF_MAX_ISIZE || d.comp_off > comp_bytes || comp_bytes - d.comp_off < d.comp_len ||
            d.out_off > out_bytes || out_bytes - d.out_off < d.isize)
            return -1;
    }
    if (n_blocks == 0) return 0;
    u32 next = 0;
    if (grid == 0) grid = std::min<u32>((n_blocks + 3) / 4, 2);
    emu_launch(k_bgzf_inflate, dim3(grid), dim3(BGZF_THREADS), comp, blocks, n_blocks, out, &next);
    return 0;
}
extern "C" uint32_t emu_bgzf_lds_per_wave(void) { return BGZF_LDS_PER_WAVE; }

#ifdef EMU_BGZF_MAIN
#include <sanitizer/asan_interface.h>

/* poison the bytes of [base, base + n) outside the given (offset, length) ranges */
static void poison_gaps(const uint8_t* base, uint64_t n, std::vector<std::pair<uint64_t, uint64_t>> r) {
    std::sort(r.begin(), r.end());
    uint64_t at = 0;
    for (auto& x : r) {
        if (x.first > at) ASAN_POISON_MEMORY_REGION(base + at, x.first - at);
        at = std::max(at, x.first + x.second);
    }
    if (n > at) ASAN_POISON_MEMORY_REGION(base + at, n - at);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hdr[4]; /* comp_bytes, out_bytes, n_blocks, grid */
    if (fread(hdr, 8, 4, f) != 4) return 2;
    std::vector<fpl_bgzf_block> blocks((size_t)hdr[2]);
    uint8_t* comp = (uint8_t*)malloc((size_t)hdr[0] + 1);
    uint8_t* out = (uint8_t*)malloc((size_t)hdr[1] + 1);
    if (hdr[2] && fread(blocks.data(), 32, blocks.size(), f) != blocks.size()) return 2;
    if (hdr[0] && fread(comp, 1, (size_t)hdr[0], f) != hdr[0]) return 2;
    if (hdr[1] && fread(out, 1, (size_t)hdr[1], f) != hdr[1]) return 2;
    fclose(f);
    std::vector<std::pair<uint64_t, uint64_t>> rc, ro;
    for (auto& d : blocks) {
        rc.emplace_back(d.comp_off, d.comp_len);
        ro.emplace_back(d.out_off, d.isize);
    }
    poison_gaps(comp, hdr[0] + 1, rc);
    poison_gaps(out, hdr[1] + 1, ro);
    const int rcode = emu_bgzf_inflate(comp, hdr[0], blocks.data(), (uint32_t)blocks.size(), out, hdr[1], (uint32_t)hdr[3]);
    ASAN_UNPOISON_MEMORY_REGION(comp, hdr[0] + 1);
    ASAN_UNPOISON_MEMORY_REGION(out, hdr[1] + 1);
    if (rcode != 0) return 3;
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(blocks.data(), 32, blocks.size(), f);
    fwrite(out, 1, (size_t)hdr[1], f);
    fclose(f);
    free(comp);
    free(out);
    return 0;
}
#endif
