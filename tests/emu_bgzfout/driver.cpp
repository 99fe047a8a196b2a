/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bgzfout/emu_bgzfout_run, built by tests/emu_bgzfout/build.py).
 *
 * The gzip kernels (fastplong_amd/csrc/gz_emit.h) in BOTH framings, compiled for the host on the lock-step emulator of
 * tests/emu/hip_emu.h and launched in the order gz_emit (csrc/rt_slots.h) launches them -- as a program of its own, built with
 * -fsanitize=address,undefined.  Every buffer is a heap allocation of exactly the size the library gives it (the output: the
 * bound of gz_out_bound and not a byte more), so a store past a bound ends the program with a report.
 *   in:  u64 n_bytes, n_rec, framing (0 member, 1 BGZF); the text (regular: four lines a record, every line ended by "\n" or
 *        "\r\n"); n_rec x fpl_read_result
 *   out: u64 total, gz_len, n_blocks, crc, out_cap; the bytes
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/gz_emit.h"

#include <vector>

using namespace fpl;

template <class T>
struct Heap { /* exactly n items, so the sanitizer sees the first byte behind them */
    T* p;
    explicit Heap(size_t n) : p((T*)calloc(n ? n : 1, sizeof(T))) {}
    ~Heap() { free(p); }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hd[3];
    if (fread(hd, 8, 3, f) != 3) return 2;
    const u64 n_bytes = hd[0];
    const u32 n_rec = (u32)hd[1];
    const bool bgzf = hd[2] != 0;
    Heap<u8> text((size_t)n_bytes + 16);
    Heap<fpl_read_result> res(n_rec);
    if (n_bytes && fread(text.p, 1, (size_t)n_bytes, f) != n_bytes) return 2;
    if (n_rec && fread(res.p, sizeof(fpl_read_result), n_rec, f) != n_rec) return 2;
    fclose(f);
    std::vector<u32> nl, line;
    for (u64 i = 0; i < n_bytes; i++)
        if (text.p[i] == '\n') nl.push_back((u32)i);
    if (nl.size() != 4 * (size_t)n_rec || (n_bytes && text.p[n_bytes - 1] != '\n')) return 3;
    line.resize(nl.size() + 1);
    for (size_t k = 0; k < nl.size(); k++) line[k] = k ? nl[k - 1] + 1 : 0;
    nl.push_back(0);
    const u32 blk_cap = (u32)gz_blocks_bound(n_bytes, n_rec);
    Heap<u64> rec_off((size_t)n_rec + 1), blk_start((size_t)blk_cap + 1);
    GzHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    emu_launch(k_gz_layout, dim3(1), dim3(1024), (const u8*)text.p, (const u32*)line.data(), (const u32*)nl.data(),
               (const fpl_read_result*)res.p, n_rec, rec_off.p, blk_start.p, blk_cap, &hdr);
    if (hdr.status) return 4;
    const u32 nb = hdr.n_blocks;
    const u64 out_cap = hdr.total ? gz_out_bound(hdr.total, nb, bgzf) : 0;
    Heap<u8> comp((size_t)hdr.total + 16), tmp((size_t)(hdr.total + (u64)GZ_SLACK * nb + 16)), out((size_t)out_cap);
    Heap<u32> blk_size(nb + 1), blk_crc(nb + 1);
    Heap<u64> blk_off(nb + 1);
    if (hdr.total) {
        emu_launch(k_gz_compose, dim3(2), dim3(256), (const u8*)text.p, (const u32*)line.data(), (const u32*)nl.data(),
                   (const fpl_read_result*)res.p, n_rec, (const u64*)rec_off.p, comp.p, (u64)hdr.total);
        const dim3 grid(std::min<u32>(nb, 3));
        if (bgzf) {
            const u32 n_stripes = (u32)gz_bgzf_blocks(hdr.total);
            emu_launch(k_gz_block_bgzf, grid, dim3(GZ_THREADS), (const u8*)comp.p, (const u64*)blk_start.p, (const GzHeader*)&hdr, tmp.p,
                       blk_size.p, blk_crc.p);
            emu_launch(k_gz_finish_bgzf, dim3(1), dim3(1024), (const u64*)blk_start.p, (const u32*)blk_size.p, (const u32*)blk_crc.p,
                       blk_off.p, &hdr, out_cap);
            emu_launch(k_gz_frame, dim3((n_stripes + 255) / 256), dim3(256), (const u64*)blk_start.p, (const u32*)blk_size.p,
                       (const u32*)blk_crc.p, (const u64*)blk_off.p, &hdr, out.p, out_cap);
        } else {
            emu_launch(k_gz_block, grid, dim3(GZ_THREADS), (const u8*)comp.p, (const u64*)blk_start.p, (const GzHeader*)&hdr, tmp.p,
                       blk_size.p, blk_crc.p);
            emu_launch(k_gz_finish, dim3(1), dim3(1024), (const u32*)blk_size.p, (const u32*)blk_crc.p, blk_off.p, &hdr, out.p, out_cap);
        }
        emu_launch(k_gz_compact, grid, dim3(GZ_THREADS), (const u8*)tmp.p, (const u64*)blk_start.p, (const u32*)blk_size.p,
                   (const u64*)blk_off.p, (const GzHeader*)&hdr, out.p, out_cap);
        if (hdr.status || hdr.gz_len == 0 || hdr.gz_len > out_cap) return 5;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const uint64_t info[5] = {hdr.total, hdr.gz_len, nb, hdr.crc, out_cap};
    fwrite(info, 8, 5, f);
    fwrite(out.p, 1, (size_t)hdr.gz_len, f);
    fclose(f);
    return 0;
}
