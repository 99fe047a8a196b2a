#include "batch.h"

#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <mutex>

#include "timing.h"

using namespace std;

namespace fplh {

static ByteBuf::AllocFn g_alloc = nullptr;
static ByteBuf::FreeFn g_free = nullptr;
void ByteBuf::set_allocator(AllocFn a, FreeFn f) {
    g_alloc = a;
    g_free = f;
}
namespace {
struct Arena {
    uint8_t* base = nullptr;
    size_t block = 0, n = 0;
    vector<uint8_t*> free_blocks;
    mutex mu;
    bool released = false;
    bool owns(const uint8_t* p) const { return base && p >= base && p < base + block * n; }
} g_arena;
}  // namespace
void ByteBuf::set_arena(size_t block_bytes, size_t n_blocks) {
    if (!g_alloc || g_arena.base || block_bytes == 0 || n_blocks == 0) return;
    block_bytes = (block_bytes + 4095) & ~(size_t)4095;
    const double t0 = now_s();
    g_arena.base = (uint8_t*)g_alloc(block_bytes * n_blocks);
    g_alloc_seconds_x1000.fetch_add((uint64_t)((now_s() - t0) * 1e6));
    if (!g_arena.base) return; /* (buffers then come from the allocator one by one) */
    g_alloc_bytes.fetch_add(block_bytes * n_blocks);
    g_arena.block = block_bytes;
    g_arena.n = n_blocks;
    for (size_t i = n_blocks; i-- > 0;) g_arena.free_blocks.push_back(g_arena.base + i * block_bytes);
}
void ByteBuf::release_arena() {
    lock_guard<mutex> g(g_arena.mu);
    if (g_arena.base && g_free && !g_arena.released) g_free(g_arena.base);
    g_arena.released = true; /* (owns() stays true: a buffer of the arena that is destroyed later is simply dropped) */
    g_arena.free_blocks.clear();
}
static void buf_release(uint8_t* p) {
    if (g_arena.owns(p)) {
        lock_guard<mutex> g(g_arena.mu);
        if (!g_arena.released) g_arena.free_blocks.push_back(p); /* (a released arena hands nothing out again) */
    } else if (g_free) {
        g_free(p);
    } else {
        free(p);
    }
}
ByteBuf::~ByteBuf() {
    if (p_) buf_release(p_);
}
void ByteBuf::reserve(size_t c) {
    if (c <= cap_) return;
    uint8_t* np = nullptr;
    size_t nc = 0;
    if (g_arena.base && !g_arena.released && c <= g_arena.block) {
        lock_guard<mutex> g(g_arena.mu);
        if (!g_arena.free_blocks.empty()) {
            np = g_arena.free_blocks.back();
            g_arena.free_blocks.pop_back();
            nc = g_arena.block;
        }
    }
    if (!np) {
        nc = cap_ ? cap_ : 4096;
        while (nc < c) nc += nc / 2 + 4096; /* (page-locked memory is not cheap: grow by halves, not by doubling) */
        if (g_alloc) {
            const double t0 = now_s();
            np = (uint8_t*)g_alloc(nc);
            g_alloc_seconds_x1000.fetch_add((uint64_t)((now_s() - t0) * 1e6));
            g_alloc_bytes.fetch_add(nc);
            if (!np) {
                cerr << "ERROR: cannot allocate " << nc << " bytes of page-locked host memory" << endl;
                exit(-1);
            }
        } else {
            np = (uint8_t*)malloc(nc);
            if (!np) {
                cerr << "ERROR: out of memory" << endl;
                exit(-1);
            }
        }
    }
    if (n_) memcpy(np, p_, n_);
    if (p_) buf_release(p_);
    p_ = np;
    cap_ = nc;
}

void Batch::clear() {
    seq.clear();
    qual.clear();
    off.clear();
    text.clear();
    name_off.clear();
    name_len.clear();
    strand_len.clear();
    raw.clear();
    raw_begin = raw_len = 0;
    line.clear();
    text_backed = false;
    bam.clear();
    rec_start.clear();
    bam_backed = false;
}

void Batch::adopt_lines(const uint32_t* ls, uint32_t n_records) {
    const uint8_t* t = raw.data();
    const uint32_t base = (uint32_t)raw_begin;
    line.resize(4 * (size_t)n_records);
    off.resize((size_t)n_records + 1);
    name_len.resize(n_records);
    strand_len.resize(n_records);
    uint64_t run = 0;
    for (uint32_t i = 0; i < n_records; i++) {
        uint32_t L[5];
        for (int j = 0; j < 4; j++) L[j] = line[4 * (size_t)i + j] = ls[4 * (size_t)i + j] + base;
        L[4] = i + 1 < n_records ? ls[4 * (size_t)i + 4] + base : base + (uint32_t)raw_len;
        uint32_t ll[4];
        for (int j = 0; j < 4; j++) { /* a line ends with "\n" or "\r\n" (regular text: the device checked) */
            uint32_t e = L[j + 1] - 1;
            if (e > L[j] && t[e - 1] == '\r') e--;
            ll[j] = e - L[j];
        }
        name_len[i] = ll[0];
        strand_len[i] = ll[2];
        off[i] = run;
        run += ll[1];
    }
    off[n_records] = run;
}

}  // namespace fplh
