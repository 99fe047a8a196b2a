/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_bamwalk/emu_bamwalk_run; tests/emu_bamwalk/build.py).
 *
 * The kernels of fastplong_amd/csrc/bam_walk.h compiled for the host on the lock-step emulator of tests/emu/hip_emu.h.  A Ctx is
 * what fpl_ctx keeps for fpl_process_bgzf_bam_async -- the tail buffer and the walk's state -- and emu_bw_submit is that call
 * without the device and without the inflate: the same plan (bam_walk_plan), the same launches (bam_walk_enqueue), over inflated
 * bytes given as they are.  Every buffer is a heap block of exactly the size the kernels are promised and filled with 0xA5, so
 * under AddressSanitizer a read outside [0, tail_cap + total) or a store outside a list, a dense array, the names or the tail ends
 * the program with a report, and nothing can rely on an initial value.
 * With EMU_BAMWALK_MAIN the file is that program: a script of operations in, results out (build.py says how).
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/bam_walk.h"

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
struct Out {
    fpl_bam_window hdr;
    std::vector<u64> cand, rec, off, name_off;
    std::vector<u8> names;
};
/* -1: the arguments are refused */
int submit(Ctx* c, const u8* bytes, uint64_t n, uint64_t skip, uint32_t seg_bytes, uint32_t rec_cap, const uint32_t* block_status,
           uint32_t n_blocks, Out& o) {
    BamWalkJob j;
    if (!bam_walk_plan(j, c->tail_cap, n, skip, seg_bytes)) return -1;
    const uint64_t hi = c->tail_cap + n;
    u8* buf = fresh<u8>(hi);
    if (n) memcpy(buf + c->tail_cap, bytes, n);
    std::vector<fpl_bgzf_block> blocks(n_blocks);
    for (uint32_t i = 0; i < n_blocks; i++) blocks[i] = fpl_bgzf_block{0, 0, 0, 0, 0, block_status[i]};
    j.buf = buf;
    j.rec_cap = rec_cap ? rec_cap : bam_walk_rec_cap(n);
    j.st = c->st;
    j.tail_buf = c->tail;
    j.blocks = blocks.data();
    j.n_blocks = n_blocks;
    j.cand = fresh<u64>(j.n_seg);
    j.segs = fresh<BamSeg>(j.n_seg);
    j.lists = fresh<u32>((size_t)j.n_seg * j.per_seg);
    j.bases = fresh<BamSegBase>(j.n_seg);
    j.hdr = fresh<fpl_bam_window>(1);
    j.rec_start = fresh<uint64_t>((size_t)j.rec_cap + 1);
    j.off = fresh<uint64_t>((size_t)j.rec_cap + 1);
    j.name_off = fresh<uint64_t>((size_t)j.rec_cap + 1);
    j.names = fresh<u8>(hi);
    j.names_cap = hi;
    bam_walk_enqueue(j, nullptr);
    o.hdr = *j.hdr;
    o.cand.assign(j.cand, j.cand + j.n_seg);
    if (o.hdr.status == FPL_BAMW_OK) {
        const size_t k = o.hdr.n_reads;
        o.rec.assign(j.rec_start, j.rec_start + k);
        o.off.assign(j.off, j.off + k + 1);
        o.name_off.assign(j.name_off, j.name_off + k + 1);
        o.names.assign(j.names, j.names + o.hdr.name_bytes);
    }
    free(buf), free(j.cand), free(j.segs), free(j.lists), free(j.bases), free(j.hdr), free(j.rec_start), free(j.off), free(j.name_off), free(j.names);
    return 0;
}
}  // namespace

#ifdef EMU_BAMWALK_MAIN
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
        } else if (op == 1 && c) { /* a submission: n, skip, seg_bytes, rec_cap, n_blocks; the bytes; the blocks' statuses */
            uint64_t h[5];
            if (!get(f, h, 40)) return 2;
            std::vector<u8> bytes(h[0]);
            std::vector<uint32_t> bst(h[4]);
            if (!get(f, bytes.data(), h[0]) || !get(f, bst.data(), 4 * h[4])) return 2;
            u8* exact = (u8*)malloc(h[0] ? h[0] : 1); /* (a block of its own: reading past the input is a report) */
            if (h[0]) memcpy(exact, bytes.data(), h[0]);
            Out o;
            memset(&o.hdr, 0, sizeof(o.hdr));
            const int64_t rc = submit(c, exact, h[0], h[1], (uint32_t)h[2], (uint32_t)h[3], bst.data(), (uint32_t)h[4], o);
            free(exact);
            fwrite(&rc, 8, 1, g);
            fwrite(&o.hdr, sizeof(o.hdr), 1, g);
            const uint64_t ns = o.cand.size();
            fwrite(&ns, 8, 1, g);
            put(g, o.cand.data(), 8 * ns);
            if (rc == 0 && o.hdr.status == FPL_BAMW_OK) {
                put(g, o.rec.data(), 8 * o.rec.size());
                put(g, o.off.data(), 8 * o.off.size());
                put(g, o.name_off.data(), 8 * o.name_off.size());
                put(g, o.names.data(), o.names.size());
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
