/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_frag/emu_frag_run; tests/emu_frag/build.py).
 *
 * The fragment forms of the device output -- fastplong_amd/csrc/frag_index.h, the k_gz_*_frag kernels of gz_emit.h and the
 * k_emit_*_frag / k_emit_mask kernels of emit.h -- compiled for the host on the lock-step emulator of tests/emu/hip_emu.h and
 * launched in the order the library launches them (rt_batch.h: frag_index, emit_fragments; rt_slots.h: gz_layout_frag, gz_emit),
 * with the library's capacities.  Every buffer is a heap block of exactly the size the kernels are promised, filled with 0xA5:
 * under AddressSanitizer a read or a store outside one ends the program with a report, and nothing can rely on an initial value.
 * The program takes one job: a file in, a file out (build.py says what they hold).
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/gz_emit.h"
#include "../../fastplong_amd/csrc/emit.h"

#include <stdio.h>

#include <algorithm>
#include <vector>

using namespace fpl;

namespace {
template <class T>
T* fresh(size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset((void*)p, 0xA5, n ? n * sizeof(T) : 1);
    return p;
}
struct In {
    std::vector<u8> raw;
    size_t at = 0;
    template <class T>
    T one() {
        T v;
        memcpy(&v, raw.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    template <class T>
    T* block(size_t n) { /* a heap block of its own, exactly n items */
        T* p = (T*)malloc(n ? n * sizeof(T) : 1);
        if (n) memcpy((void*)p, raw.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return p;
    }
};
struct Out {
    FILE* f;
    template <class T>
    void put(const T* p, size_t n) {
        if (n) fwrite(p, sizeof(T), n, f);
    }
    void u64v(u64 v) { put(&v, 1); }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    In in;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        in.raw.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (!in.raw.empty() && fread(in.raw.data(), 1, in.raw.size(), f) != in.raw.size()) return 2;
        fclose(f);
    }
    const u64 n_bytes = in.one<u64>(), n_rec64 = in.one<u64>(), n_frag = in.one<u64>(), n_reg = in.one<u64>(), frag_cap = in.one<u64>(),
              bgzf = in.one<u64>(), cap_reads = in.one<u64>(), cap_bytes = in.one<u64>();
    const u32 n_rec = (u32)n_rec64;
    u32 counts_in[4];
    for (u32& c : counts_in) c = in.one<u32>();
    u8* text = fresh<u8>(n_bytes + 16); /* (the chunk and 16 bytes of padding, as the slot's d_text) */
    memcpy(text, in.raw.data() + in.at, n_bytes);
    in.at += n_bytes;
    fpl_read_result* res = in.block<fpl_read_result>(n_rec);
    fpl_fragment* frags = fresh<fpl_fragment>(frag_cap); /* (the list has its capacity; the entries behind the count are nobody's) */
    memcpy((void*)frags, in.raw.data() + in.at, std::min<u64>(n_frag, frag_cap) * sizeof(fpl_fragment));
    in.at += n_frag * sizeof(fpl_fragment);
    fpl_region* regs = in.block<fpl_region>(n_reg);
    u32* counts = fresh<u32>(4);
    memcpy(counts, counts_in, sizeof(counts_in));

    /* the text's lines, found the plain way: four a record, every one ended by "\n" */
    std::vector<u32> nl;
    for (u64 i = 0; i < n_bytes; i++)
        if (text[i] == '\n') nl.push_back((u32)i);
    if (nl.size() != 4 * (size_t)n_rec) return 3;
    u32* line = fresh<u32>(4 * (size_t)n_rec);
    u32* nl_pos = fresh<u32>(4 * (size_t)n_rec);
    for (size_t k = 0; k < nl.size(); k++) line[k] = k ? nl[k - 1] + 1 : 0, nl_pos[k] = nl[k];
    /* the batch as CSR arrays: what the parse makes of it */
    uint64_t* off = fresh<uint64_t>((size_t)n_rec + 1);
    off[0] = 0;
    for (u32 r = 0; r < n_rec; r++) off[r + 1] = off[r] + (nl[4 * r + 1] - line[4 * r + 1]);
    const u64 n_bases = off[n_rec];
    u8* seq = fresh<u8>(n_bases);
    u8* qual = fresh<u8>(n_bases);
    for (u32 r = 0; r < n_rec; r++) {
        memcpy(seq + off[r], text + line[4 * r + 1], off[r + 1] - off[r]);
        memcpy(qual + off[r], text + line[4 * r + 3], off[r + 1] - off[r]);
    }

    Out out{fopen(argv[2], "wb")};
    if (!out.f) return 2;

    /* ---- the index (rt_batch.h: frag_index) ---- */
    FragIndex* fi = fresh<FragIndex>(1);
    memset(fi, 0, sizeof(FragIndex));
    u32* cnt = fresh<u32>((size_t)n_rec + 1);
    memset(cnt, 0, sizeof(u32) * ((size_t)n_rec + 1));
    u32* first = fresh<u32>((size_t)n_rec + 1);
    u32* order = fresh<u32>(frag_cap);
    memset(order, 0xFF, sizeof(u32) * frag_cap);
    const dim3 fgrid(std::min<u32>(frag_index_blocks(frag_cap, 2), 3)); /* (a few blocks: the lanes walk the list in strides) */
    emu_launch(k_frag_count, fgrid, dim3(FI_THREADS), (const fpl_fragment*)frags, (const u32*)counts, (u32)frag_cap, n_rec, cnt, fi);
    emu_launch(k_frag_first, dim3(1), dim3(FI_SCAN), (const u32*)cnt, n_rec, (const u32*)counts, first, fi);
    emu_launch(k_frag_place, fgrid, dim3(FI_THREADS), (const fpl_fragment*)frags, (const u32*)cnt, (const u32*)first, n_rec, order, fi);
    out.put(fi, 1);
    out.put(first, (size_t)n_rec + 1);
    out.put(order, fi->status ? 0 : fi->n);

    /* ---- gzip (rt_slots.h: gz_layout_frag, gz_emit) ---- */
    const GzFragList fl{frags, regs, order, fi};
    const u64 blk_want = gz_frag_blocks_bound(n_bytes / 2, frag_cap) + 1;
    u64* rec_off = fresh<u64>(frag_cap + 1);
    u64* blk_start = fresh<u64>(blk_want);
    GzHeader* hdr = fresh<GzHeader>(1);
    emu_launch(k_gz_layout_frag, dim3(1), dim3(1024), (const u8*)text, (const u32*)line, (const u32*)nl_pos, (const fpl_read_result*)res, n_rec, fl,
               rec_off, blk_start, (u32)blk_want - 1, hdr);
    out.put(hdr, 1);
    if (!hdr->status) {
        const u32 n = fi->n, nb = hdr->n_blocks;
        const u64 total = hdr->total;
        out.put(rec_off, (size_t)n + 1);
        out.put(blk_start, (size_t)nb + 1);
        u8* comp = fresh<u8>(total + 16);
        emu_launch(k_gz_compose_frag, dim3(2), dim3(256), (const u8*)text, (const u32*)line, (const u32*)nl_pos, (const fpl_read_result*)res, n_rec,
                   fl, (const u64*)rec_off, comp, total);
        out.put(comp, total);
        /* the kernels behind the compose, unchanged: the member, or the BGZF blocks */
        const u64 out_want = gz_out_bound(total, nb, bgzf != 0);
        u8* tmp = fresh<u8>(out_want + 16);
        u8* gz = fresh<u8>(out_want + 16);
        u32* blk_size = fresh<u32>((size_t)nb + 1);
        u32* blk_crc = fresh<u32>((size_t)nb + 1);
        u64* blk_off = fresh<u64>((size_t)nb + 1);
        if (total) {
            const dim3 grid(std::max<u32>(1, std::min<u32>(nb, 3)));
            if (bgzf) {
                emu_launch(k_gz_block_bgzf, grid, dim3(GZ_THREADS), (const u8*)comp, (const u64*)blk_start, (const GzHeader*)hdr, tmp, blk_size, blk_crc);
                emu_launch(k_gz_finish_bgzf, dim3(1), dim3(1024), (const u64*)blk_start, (const u32*)blk_size, (const u32*)blk_crc, blk_off, hdr, out_want);
                emu_launch(k_gz_frame, dim3(1), dim3(256), (const u64*)blk_start, (const u32*)blk_size, (const u32*)blk_crc, (const u64*)blk_off, hdr,
                           gz, out_want);
            } else {
                emu_launch(k_gz_block, grid, dim3(GZ_THREADS), (const u8*)comp, (const u64*)blk_start, (const GzHeader*)hdr, tmp, blk_size, blk_crc);
                emu_launch(k_gz_finish, dim3(1), dim3(1024), (const u32*)blk_size, (const u32*)blk_crc, blk_off, hdr, gz, out_want);
            }
            emu_launch(k_gz_compact, grid, dim3(GZ_THREADS), (const u8*)tmp, (const u64*)blk_start, (const u32*)blk_size, (const u64*)blk_off,
                       (const GzHeader*)hdr, gz, out_want);
        }
        out.put(hdr, 1);
        out.put(gz, total && !hdr->status ? hdr->gz_len : 0);
        free(comp), free(tmp), free(gz), free(blk_size), free(blk_crc), free(blk_off);
    }

    /* ---- CSR (rt_batch.h: emit_fragments) ---- */
    {
        const u32 nblk = (u32)((frag_cap + EM_LAYOUT_READS - 1) / EM_LAYOUT_READS);
        const size_t n_from = (size_t)std::min<u64>(frag_cap, cap_reads);
        u32* blk_cnt = fresh<u32>(nblk);
        u32* blk_max = fresh<u32>(nblk);
        u64* blk_bytes = fresh<u64>(nblk);
        EmitFrom* from = fresh<EmitFrom>(n_from ? n_from : 1);
        u32* ent = fresh<u32>(n_from ? n_from : 1);
        fpl_emit_info* info = fresh<fpl_emit_info>(1);
        uint64_t* off_out = fresh<uint64_t>(cap_reads + 1);
        u32* src = fresh<u32>(cap_reads);
        u8* kind = fresh<u8>(cap_reads);
        uint16_t* break_no = fresh<uint16_t>(cap_reads);
        u8* seq_out = fresh<u8>(cap_bytes);
        u8* qual_out = fresh<u8>(cap_bytes);
        emu_launch(k_emit_count_frag, dim3(nblk), dim3(EM_LAYOUT_READS), (const uint64_t*)off, (const fpl_read_result*)res, n_rec,
                   (const fpl_fragment*)frags, (const u32*)order, (const FragIndex*)fi, blk_cnt, blk_bytes, blk_max);
        emu_launch(k_emit_scan, dim3(1), dim3(EM_SCAN_BLOCKS), blk_cnt, blk_bytes, (const u32*)blk_max, nblk, cap_bytes, (u32)cap_reads, off_out,
                   info);
        emu_launch(k_emit_fill_frag, dim3(nblk), dim3(EM_LAYOUT_READS), (const uint64_t*)off, (const fpl_read_result*)res, n_rec,
                   (const fpl_fragment*)frags, (const u32*)order, (const FragIndex*)fi, (const u32*)blk_cnt, (const u64*)blk_bytes, info, off_out,
                   src, kind, break_no, from, ent);
        emu_launch(k_emit_gather, dim3(emit_gather_blocks(cap_bytes, 2)), dim3(EM_GATHER_THREADS), (const u8*)seq, (const u8*)qual,
                   (const uint64_t*)off_out, (const EmitFrom*)from, (const fpl_emit_info*)info, seq_out, qual_out);
        emu_launch(k_emit_mask, dim3(2), dim3(EM_GATHER_THREADS), (const fpl_fragment*)frags, (const fpl_region*)regs, (const u32*)ent,
                   (const uint64_t*)off_out, (const fpl_emit_info*)info, seq_out);
        out.put(info, 1);
        out.put(off_out, 1);
        if (!info->status) {
            out.put(off_out + 1, info->n_out);
            out.put(src, info->n_out);
            out.put(kind, info->n_out);
            out.put(break_no, info->n_out);
            out.put(seq_out, info->n_bytes);
            out.put(qual_out, info->n_bytes);
        }
    }
    fclose(out.f);
    return 0;
}
