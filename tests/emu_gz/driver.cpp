/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_gz/libfpl_emu_gz.so, built by tests/emu_gz/build.py).
 *
 * The gzip kernels (fastplong_amd/csrc/gz_emit.h) compiled for the host on the lock-step emulator of tests/emu/hip_emu.h and
 * launched in the order fpl_wait_text_gz launches them.  The line starts and line ends are found here the plain way: the text must
 * be regular (four lines a record, every line ended by "\n" or "\r\n").
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/gz_emit.h"

#include <vector>

using namespace fpl;

/* blocks -> member: k_gz_block, k_gz_finish, k_gz_compact over a composed text whose block starts are known */
static int run_blocks(const u8* comp, const std::vector<u64>& blk_start, GzHeader* hdr, u8* out, u64 out_cap) {
    const u32 nb = hdr->n_blocks;
    std::vector<u8> tmp((size_t)(hdr->total + (u64)GZ_SLACK * nb + 16));
    std::vector<u32> blk_size(nb + 1), blk_crc(nb + 1);
    std::vector<u64> blk_off(nb + 1);
    if (nb) emu_launch(k_gz_block, dim3(std::min<u32>(nb, 3)), dim3(GZ_THREADS), comp, blk_start.data(), (const GzHeader*)hdr, tmp.data(),
                       blk_size.data(), blk_crc.data());
    emu_launch(k_gz_finish, dim3(1), dim3(1024), (const u32*)blk_size.data(), (const u32*)blk_crc.data(), blk_off.data(), hdr, out, out_cap);
    if (nb) emu_launch(k_gz_compact, dim3(std::min<u32>(nb, 3)), dim3(GZ_THREADS), (const u8*)tmp.data(), blk_start.data(),
                       (const u32*)blk_size.data(), (const u64*)blk_off.data(), (const GzHeader*)hdr, out, out_cap);
    return (int)hdr->status;
}

extern "C" {
/* info: total, gz_len, n_blocks, crc.  returns 0, or -1 for text that is not regular, -2 when out is too small */
int emu_gz_emit(const uint8_t* text, uint64_t n_bytes, const fpl_read_result* res, uint32_t n_rec, uint8_t* out, uint64_t out_cap,
                uint64_t* info, uint8_t* comp_out) {
    std::vector<u32> nl, line;
    for (u64 i = 0; i < n_bytes; i++)
        if (text[i] == '\n') nl.push_back((u32)i);
    if (nl.size() != 4 * (size_t)n_rec || (n_bytes && text[n_bytes - 1] != '\n')) return -1;
    line.resize(nl.size() + 1);
    for (size_t k = 0; k < nl.size(); k++) line[k] = k ? nl[k - 1] + 1 : 0;
    nl.push_back(0);
    std::vector<u8> padded(n_bytes + 16);
    memcpy(padded.data(), text, n_bytes);
    const u32 blk_cap = (u32)gz_blocks_bound(n_bytes, n_rec);
    std::vector<u64> rec_off((size_t)n_rec + 1), blk_start((size_t)blk_cap + 1);
    GzHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    emu_launch(k_gz_layout, dim3(1), dim3(1024), (const u8*)padded.data(), (const u32*)line.data(), (const u32*)nl.data(), res, n_rec,
               rec_off.data(), blk_start.data(), blk_cap, &hdr);
    if (hdr.status) return -3;
    std::vector<u8> comp((size_t)hdr.total + 16);
    if (n_rec) emu_launch(k_gz_compose, dim3(2), dim3(256), (const u8*)padded.data(), (const u32*)line.data(), (const u32*)nl.data(), res, n_rec,
                          (const u64*)rec_off.data(), comp.data(), (u64)hdr.total);
    if (comp_out) memcpy(comp_out, comp.data(), (size_t)hdr.total);
    info[0] = hdr.total;
    info[2] = hdr.n_blocks;
    if (GZ_MEMBER_EXTRA + hdr.total + (u64)GZ_SLACK * hdr.n_blocks > out_cap) return -2;
    const int st = run_blocks(comp.data(), blk_start, &hdr, out, out_cap);
    info[1] = hdr.gz_len;
    info[3] = hdr.crc;
    return st ? -3 : 0;
}

/* the block / CRC / member stages alone over any bytes, blocks cut at every multiple of GZ_B */
int emu_gz_deflate(const uint8_t* data, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* info) {
    GzHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.total = n;
    hdr.n_blocks = (u32)((n + GZ_B - 1) / GZ_B);
    std::vector<u64> blk_start;
    for (u32 b = 0; b < hdr.n_blocks; b++) blk_start.push_back((u64)b * GZ_B);
    blk_start.push_back(n);
    std::vector<u8> comp(data, data + n);
    comp.resize(n + 16);
    if (GZ_MEMBER_EXTRA + n + (u64)GZ_SLACK * hdr.n_blocks > out_cap) return -2;
    const int st = run_blocks(comp.data(), blk_start, &hdr, out, out_cap);
    info[0] = hdr.total, info[1] = hdr.gz_len, info[2] = hdr.n_blocks, info[3] = hdr.crc;
    return st ? -3 : 0;
}
uint32_t emu_gz_block_bytes(void) { return GZ_B; }
uint32_t emu_gz_long_line(void) { return GZ_L; }
uint32_t emu_gz_stretch(void) { return GZ_STRETCH; }
}
