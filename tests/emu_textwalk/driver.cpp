/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_textwalk/emu_textwalk_run; tests/emu_textwalk/build.py).
 *
 * The kernels of fastplong_amd/csrc/text_walk.h and text_parse.h compiled for the host on the lock-step emulator of
 * tests/emu/hip_emu.h.  A Ctx is what fpl_ctx keeps for fpl_process_bgzf_text_async -- the tail buffer and the walk's state --
 * and submit() is that call without the device and without the inflate: the same plan (text_walk_plan), the same launches
 * (text_walk_enqueue), the library's capacities, over inflated bytes given as they are.  whole() is fpl_process_text_async's six
 * launches over a whole chunk.  Every buffer is a heap block of exactly the size the kernels are promised and filled with 0xA5,
 * so under AddressSanitizer a read outside the text or a store outside a list, an array, the names or the tail ends the program
 * with a report, and nothing can rely on an initial value.
 * With EMU_TEXTWALK_MAIN the file is that program: a script of operations in, results out (build.py says how).
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/text_walk.h"

#include <vector>

using namespace fpl;

namespace {
struct Ctx {
    uint64_t tail_cap;
    u8* tail;
    BamWalkState* st;
};
template <class T>
T* fresh(size_t n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset((void*)p, 0xA5, n ? n * sizeof(T) : 1);
    return p;
}
Ctx* ctx_new(uint64_t tail_cap) {
    Ctx* c = new Ctx;
    c->tail_cap = tail_cap;
    c->tail = fresh<u8>(tail_cap);
    c->st = (BamWalkState*)calloc(1, sizeof(BamWalkState));
    return c;
}
void ctx_free(Ctx* c) {
    if (!c) return;
    free(c->tail), free(c->st);
    delete c;
}
/* rt_bam.h's rule for the names of a submission */
uint64_t names_cap_of(uint64_t hi) { return std::min<uint64_t>(hi, hi / 4 + (1u << 20)); }

struct Out {
    fpl_text_window hdr;
    uint64_t lo;
    std::vector<u32> line, len;
    std::vector<uint64_t> off, name_off;
    std::vector<u8> names, seq, qual;
};
/* -1: the arguments are refused */
int submit(Ctx* c, const u8* bytes, uint64_t n, const uint32_t* block_status, uint32_t n_blocks, Out& o) {
    TextWalkJob j;
    if (!text_walk_plan(j, c->tail_cap, n)) return -1;
    const uint64_t hi = c->tail_cap + n;
    u8* buf = fresh<u8>(hi);
    if (n) memcpy(buf + c->tail_cap, bytes, n);
    std::vector<fpl_bgzf_block> blocks(n_blocks);
    for (uint32_t i = 0; i < n_blocks; i++) blocks[i] = fpl_bgzf_block{0, 0, 0, 0, 0, block_status[i]};
    o.lo = c->tail_cap - std::min<uint64_t>(c->st->tail_len, c->tail_cap);
    j.buf = buf;
    j.st = c->st;
    j.tail_buf = c->tail;
    j.blocks = blocks.data();
    j.n_blocks = n_blocks;
    j.blk = fresh<u32>((size_t)j.nblk + 1);
    j.nl_pos = fresh<u32>(4 * (size_t)j.rec_cap);
    j.line = fresh<u32>(4 * (size_t)j.rec_cap);
    j.len = fresh<u32>(j.rec_cap);
    j.nlen = fresh<u32>(j.rec_cap);
    j.ws = fresh<TextWalkScratch>(1);
    j.hdr = fresh<fpl_text_window>(1);
    j.off = fresh<uint64_t>((size_t)j.rec_cap + 1);
    j.name_off = fresh<uint64_t>((size_t)j.rec_cap + 1);
    j.names_cap = names_cap_of(hi);
    j.names = fresh<u8>(j.names_cap);
    j.seq_cap = hi / 2 + 64;
    j.seq = fresh<u8>(j.seq_cap);
    j.qual = fresh<u8>(j.seq_cap);
    text_walk_enqueue(j, 2, nullptr);
    o.hdr = *j.hdr;
    if (o.hdr.status == FPL_TXTW_OK) {
        const size_t k = o.hdr.n_reads;
        o.line.assign(j.line, j.line + 4 * k);
        o.len.assign(j.len, j.len + k);
        o.off.assign(j.off, j.off + k + 1);
        o.name_off.assign(j.name_off, j.name_off + k + 1);
        o.names.assign(j.names, j.names + o.hdr.name_bytes);
        o.seq.assign(j.seq, j.seq + o.hdr.n_bases);
        o.qual.assign(j.qual, j.qual + o.hdr.n_bases);
    }
    free(buf), free(j.blk), free(j.nl_pos), free(j.line), free(j.len), free(j.nlen), free(j.ws), free(j.hdr), free(j.off), free(j.name_off);
    free(j.names), free(j.seq), free(j.qual);
    return 0;
}

struct Whole {
    TextHeader hdr;
    std::vector<u32> line, len;
    std::vector<uint64_t> off;
    std::vector<u8> seq, qual;
};
/* the six launches of fpl_process_text_async (rt_text.h) over a chunk of n > 0 bytes, with its sizes */
void whole(const u8* bytes, uint64_t n, Whole& o) {
    const u32 nblk = (u32)((n + TP_BLOCK_BYTES - 1) / TP_BLOCK_BYTES);
    const u32 rec_cap = (u32)(n / 64 + 16);
    u8* text = fresh<u8>(n);
    memcpy(text, bytes, n);
    u32* blk = fresh<u32>(nblk);
    u32* nl = fresh<u32>(4 * (size_t)rec_cap);
    u32* line = fresh<u32>(4 * (size_t)rec_cap);
    u32* len = fresh<u32>(rec_cap);
    uint64_t* off = fresh<uint64_t>((size_t)rec_cap + 1);
    const uint64_t cap = n / 2 + 64;
    u8 *seq = fresh<u8>(cap), *qual = fresh<u8>(cap);
    TextHeader* hdr = (TextHeader*)calloc(1, sizeof(TextHeader));
    hdr->bad_record = ~0ull;
    emu_launch(k_text_count, dim3(nblk), dim3(TP_THREADS), (const u8*)text, (u64)n, blk, hdr);
    emu_launch(k_text_scan, dim3(1), dim3(1024), blk, nblk, hdr);
    emu_launch(k_text_fill, dim3(nblk), dim3(TP_THREADS), (const u8*)text, (u64)n, (const u32*)blk, nl, 4 * rec_cap);
    emu_launch(k_text_records, dim3(std::min<u32>(std::max<u32>(1u, (rec_cap + 255u) / 256u), 2u)), dim3(256), (const u8*)text, (u64)n, (const u32*)nl,
               rec_cap, hdr, line, len);
    emu_launch(k_text_offsets, dim3(1), dim3(1024), (const u32*)len, rec_cap, hdr, off);
    emu_launch(k_text_gather, dim3(2), dim3(256), (const u8*)text, (const u32*)line, (const u32*)len, (const uint64_t*)off, (const TextHeader*)hdr,
               rec_cap, seq, qual);
    o.hdr = *hdr;
    if (hdr->status == 0) {
        const size_t k = hdr->n_records;
        o.line.assign(line, line + 4 * k);
        o.len.assign(len, len + k);
        o.off.assign(off, off + k + 1);
        o.seq.assign(seq, seq + hdr->n_bases);
        o.qual.assign(qual, qual + hdr->n_bases);
    }
    free(text), free(blk), free(nl), free(line), free(len), free(off), free(seq), free(qual), free(hdr);
}
}  // namespace

#ifdef EMU_TEXTWALK_MAIN
static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static void put(FILE* g, const void* p, size_t n) {
    if (n) fwrite(p, 1, n, g);
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint64_t n_ops;
    if (!get(f, &n_ops, 8)) return 2;
    Ctx* c = nullptr;
    for (uint64_t k = 0; k < n_ops; k++) {
        uint64_t op;
        if (!get(f, &op, 8)) return 2;
        if (op == 0) { /* a new context: tail_cap */
            uint64_t cap;
            if (!get(f, &cap, 8)) return 2;
            ctx_free(c);
            c = ctx_new(cap);
        } else if (op == 1 && c) { /* a submission: n, n_blocks; the bytes; the blocks' statuses */
            uint64_t h[2];
            if (!get(f, h, 16)) return 2;
            std::vector<uint32_t> bst(h[1]);
            u8* exact = (u8*)malloc(h[0] ? h[0] : 1); /* (a block of its own: reading past the input is a report) */
            if (!get(f, exact, h[0]) || !get(f, bst.data(), 4 * h[1])) return 2;
            Out o;
            memset(&o.hdr, 0, sizeof(o.hdr));
            o.lo = 0;
            const int64_t rc = submit(c, exact, h[0], bst.data(), (uint32_t)h[1], o);
            free(exact);
            fwrite(&rc, 8, 1, g);
            fwrite(&o.hdr, sizeof(o.hdr), 1, g);
            fwrite(&o.lo, 8, 1, g);
            if (rc == 0 && o.hdr.status == FPL_TXTW_OK) {
                put(g, o.line.data(), 4 * o.line.size());
                put(g, o.len.data(), 4 * o.len.size());
                put(g, o.off.data(), 8 * o.off.size());
                put(g, o.name_off.data(), 8 * o.name_off.size());
                put(g, o.names.data(), o.names.size());
                put(g, o.seq.data(), o.seq.size());
                put(g, o.qual.data(), o.qual.size());
            }
        } else if (op == 2 && c) { /* the tail */
            const uint64_t n = c->st->tail_len;
            if (n > c->tail_cap) return 3; /* must not happen */
            fwrite(&n, 8, 1, g);
            put(g, c->tail, n);
        } else if (op == 3 && c) { /* set the tail: len; bytes */
            uint64_t n;
            if (!get(f, &n, 8) || n > c->tail_cap) return 2;
            if (!get(f, c->tail, n)) return 2;
            c->st->tail_len = (u32)n;
            c->st->refused = 0;
            if (!n) c->st->rec_base = 0;
        } else if (op == 4 && c) { /* resume */
            c->st->refused = 0;
        } else if (op == 5 && c) { /* a larger tail capacity */
            uint64_t cap;
            if (!get(f, &cap, 8) || cap < c->tail_cap) return 2;
            u8* nw = fresh<u8>(cap);
            memcpy(nw, c->tail, c->tail_cap);
            free(c->tail);
            c->tail = nw;
            c->tail_cap = cap;
        } else if (op == 6) { /* a whole chunk through the kernels of text_parse.h: n (> 0); the bytes */
            uint64_t n;
            if (!get(f, &n, 8) || n == 0) return 2;
            u8* exact = (u8*)malloc(n);
            if (!get(f, exact, n)) return 2;
            Whole o;
            whole(exact, n, o);
            free(exact);
            fwrite(&o.hdr, sizeof(o.hdr), 1, g);
            if (o.hdr.status == 0) {
                put(g, o.line.data(), 4 * o.line.size());
                put(g, o.len.data(), 4 * o.len.size());
                put(g, o.off.data(), 8 * o.off.size());
                put(g, o.seq.data(), o.seq.size());
                put(g, o.qual.data(), o.qual.size());
            }
        } else {
            return 2;
        }
    }
    ctx_free(c);
    fclose(f);
    fclose(g);
    return 0;
}
#endif
