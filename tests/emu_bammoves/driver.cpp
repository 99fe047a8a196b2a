/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bammoves/emu_bammoves_run, built by tests/emu_bammoves/build.py).
 *
 * k_bam_tags_moves, k_bam_moves_plan and k_bamout_compose_bam_moves (fastplong_amd/csrc/bam_moves.h), with k_bam_mods_plan
 * (fastplong_amd/csrc/bam_mods.h) between the first two where the job asks for --keep_mods beside the switch, around the tagged
 * layout kernel (fastplong_amd/csrc/bam_tags.h), in front of the unchanged BGZF
 * block kernels (fastplong_amd/csrc/gz_emit.h), compiled for the host on the lock-step emulator of tests/emu/hip_emu.h and launched
 * in the order gz_layout / gz_emit (csrc/rt_slots.h) launch them -- as a program of its own, built with -fsanitize=address,undefined.
 * Every buffer is a heap allocation of exactly the size the library gives it (the record stream: its bytes + BAM_PAD; the composed
 * bytes: hdr.total + 16; the output: the bound of gz_out_bound and not a byte more; the plans: one per record; without --keep_mods the
 * buffers of its walk are null pointers, as in the library), so an access past a bound ends the program with
 * a report.
 *   in:  u64 n_bytes, n_rec, fragment_mode, mods; the uncompressed record stream; n_rec x u64 record starts; (n_rec + 1) x u64 CSR
 *        offsets; n_rec x fpl_read_result
 *   out: u64 total, gz_len, n_blocks, crc, out_cap, the four tag counters, the four modification counters, the four move counters; the composed record bytes; the BGZF blocks
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/bam_moves.h"
#include "../../fastplong_amd/csrc/bam_decode.h"

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
    uint64_t hd[4];
    if (fread(hd, 8, 4, f) != 4) return 2;
    const u64 n_bytes = hd[0];
    const u32 n_rec = (u32)hd[1];
    const u32 fragment_mode = (u32)hd[2];
    const bool mods = hd[3] != 0;
    Heap<u8> in((size_t)n_bytes + BAM_PAD);
    Heap<u64> rec_start(n_rec), off((size_t)n_rec + 1);
    Heap<fpl_read_result> res(n_rec);
    if (n_bytes && fread(in.p, 1, (size_t)n_bytes, f) != n_bytes) return 2;
    if (n_rec && fread(rec_start.p, 8, n_rec, f) != n_rec) return 2;
    if (fread(off.p, 8, (size_t)n_rec + 1, f) != (size_t)n_rec + 1) return 2;
    if (n_rec && fread(res.p, sizeof(fpl_read_result), n_rec, f) != n_rec) return 2;
    fclose(f);

    GzHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    Heap<u64> rec_off((size_t)n_rec + 1);
    Heap<BamTagInfo> info(n_rec);
    Heap<unsigned long long> counters(4), mod_counters(BAMMOD_COUNTERS);
    Heap<BamModInfo> minfo(n_rec);
    Heap<u32> cand(n_rec);
    Heap<BamModPlan> plans(n_rec);
    Heap<unsigned long long> move_counters(BAMMOVE_COUNTERS);
    Heap<BamMoveInfo> vinfo(n_rec);
    Heap<u32> vcand(n_rec);
    Heap<BamMovePlan> vplans(n_rec);
    const u64 n_bases = off.p[n_rec];
    Heap<u8> seq((size_t)n_bases + 32), qual((size_t)n_bases + 32);
    const u32 blk_cap = (u32)(bamout_bam_blocks_bound(n_bases, n_rec) + bamtag_extra_bound(n_bytes) / GZ_B + 1);
    Heap<u64> blk_start((size_t)blk_cap + 1);
    u64 word0, n_words;
    bam_words(off.p[0], off.p[n_rec], word0, n_words);
    if (n_rec && n_words)
        emu_launch(k_bam_decode, dim3((unsigned)((n_words + BAM_THREADS - 1) / BAM_THREADS)), dim3(BAM_THREADS), (const u8*)in.p,
                   (const uint64_t*)rec_start.p, (const uint64_t*)off.p, n_rec, word0, n_words, seq.p, qual.p);
    emu_launch(k_bam_tags_moves, dim3(2), dim3(256), (const u8*)in.p, n_bytes, (const uint64_t*)rec_start.p, (const fpl_read_result*)res.p, n_rec,
               fragment_mode, info.p, counters.p, mods ? minfo.p : (BamModInfo*)nullptr, mods ? cand.p : (u32*)nullptr,
               mods ? mod_counters.p : (unsigned long long*)nullptr, vinfo.p, vcand.p, move_counters.p);
    if (mods)
        emu_launch(k_bam_mods_plan, dim3(2), dim3(256), (const u8*)in.p, n_bytes, (const uint64_t*)rec_start.p, (const fpl_read_result*)res.p, n_rec,
                   fragment_mode, info.p, (const BamModInfo*)minfo.p, (const u32*)cand.p, plans.p, counters.p, mod_counters.p);
    emu_launch(k_bam_moves_plan, dim3(2), dim3(256), (const u8*)in.p, n_bytes, (const uint64_t*)rec_start.p, (const fpl_read_result*)res.p, n_rec,
               fragment_mode, info.p, (const BamMoveInfo*)vinfo.p, (const u32*)vcand.p, vplans.p, counters.p, move_counters.p);
    emu_launch(k_bamout_layout_bam_tags, dim3(1), dim3(1024), (const u8*)in.p, (const uint64_t*)rec_start.p, (const u8*)seq.p, (const u8*)qual.p,
               (const uint64_t*)off.p, (const fpl_read_result*)res.p, n_rec, (const BamTagInfo*)info.p, rec_off.p, blk_start.p, blk_cap, &hdr);
    if (hdr.status) return 4;
    const u32 nb = hdr.n_blocks;
    const u64 out_cap = hdr.total ? gz_out_bound(hdr.total, nb, true) : 0;
    Heap<u8> comp((size_t)hdr.total + 16), tmp((size_t)(hdr.total + (u64)GZ_SLACK * nb + 16)), out((size_t)out_cap);
    memset(comp.p, 0xEE, (size_t)hdr.total + 16); /* (a byte nobody writes shows up in the comparison) */
    Heap<u32> blk_size(nb + 1), blk_crc(nb + 1);
    Heap<u64> blk_off(nb + 1);
    if (hdr.total) {
        emu_launch(k_bamout_compose_bam_moves, dim3(2), dim3(256), (const u8*)in.p, (const uint64_t*)rec_start.p, (const u8*)seq.p, (const u8*)qual.p,
                   (const uint64_t*)off.p, (const fpl_read_result*)res.p, n_rec, (const BamTagInfo*)info.p,
                   mods ? (const BamModInfo*)minfo.p : (const BamModInfo*)nullptr, mods ? (const BamModPlan*)plans.p : (const BamModPlan*)nullptr,
                   (const BamMoveInfo*)vinfo.p, (const BamMovePlan*)vplans.p, (const u64*)rec_off.p, comp.p, (u64)hdr.total);
        for (int k = 0; k < 16; k++)
            if (comp.p[hdr.total + k] != 0xEE) return 6; /* a store behind the last record */
        const dim3 grid(std::min<u32>(nb, 3));
        const u32 n_stripes = (u32)gz_bgzf_blocks(hdr.total);
        emu_launch(k_gz_block_bgzf, grid, dim3(GZ_THREADS), (const u8*)comp.p, (const u64*)blk_start.p, (const GzHeader*)&hdr, tmp.p, blk_size.p,
                   blk_crc.p);
        emu_launch(k_gz_finish_bgzf, dim3(1), dim3(1024), (const u64*)blk_start.p, (const u32*)blk_size.p, (const u32*)blk_crc.p, blk_off.p, &hdr,
                   out_cap);
        emu_launch(k_gz_frame, dim3((n_stripes + 255) / 256), dim3(256), (const u64*)blk_start.p, (const u32*)blk_size.p, (const u32*)blk_crc.p,
                   (const u64*)blk_off.p, &hdr, out.p, out_cap);
        emu_launch(k_gz_compact, grid, dim3(GZ_THREADS), (const u8*)tmp.p, (const u64*)blk_start.p, (const u32*)blk_size.p, (const u64*)blk_off.p,
                   (const GzHeader*)&hdr, out.p, out_cap);
        if (hdr.status || hdr.gz_len == 0 || hdr.gz_len > out_cap) return 5;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const uint64_t head[17] = {hdr.total,          hdr.gz_len,         nb,                 hdr.crc,           out_cap,           counters.p[0],
                               counters.p[1],      counters.p[2],      counters.p[3],      mod_counters.p[0], mod_counters.p[1], mod_counters.p[2],
                               mod_counters.p[3],  move_counters.p[0], move_counters.p[1], move_counters.p[2], move_counters.p[3]};
    fwrite(head, 8, 17, f);
    fwrite(comp.p, 1, (size_t)hdr.total, f);
    fwrite(out.p, 1, (size_t)hdr.gz_len, f);
    fclose(f);
    return 0;
}
