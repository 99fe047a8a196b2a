/*
 * text_walk.h -- FASTQ text that k_bgzf_inflate left in device memory -> CSR batch, names and the tail, ON THE DEVICE
 * (fpl_process_bgzf_text_async, include/fastplong_amd.h): the resident forms of text_parse.h's kernels, and the stage between
 * inflate and parse that fpl_process_text_async leaves to its caller -- the cut at a record's end.
 *
 * The buffer of a slot is bam_walk.h's: [room for the tail | the inflated bytes of this submission].  The inflated part starts
 * at the fixed offset tail_cap, the tail of the submission before (the bytes behind its last whole record) is placed so that
 * it ends there.  The text is [lo, hi): lo = tail_cap - tail_len is known on the device only, hi = tail_cap + total.  Every
 * position -- line breaks, line starts -- is a byte offset into the BUFFER, so the buffer stays 16-byte aligned for tp_load16
 * whatever lo is, and GzTextSrc{buf, line, nl_pos} reads a slot of this kind as it reads a text slot.
 *
 * The bytes start at a record (the file's start, or the previous tail), so in regular text record k is lines 4k .. 4k + 3 and
 * with L line breaks the submission holds L / 4 whole records; the new tail starts behind line break 4 (L / 4) - 1 -- at lo
 * when there is no whole record: zero reads, status OK, and the tail grows.
 *
 *   k_tw_place_tail  the context's tail, right-aligned in front of the inflated bytes; the scratch record at its start values.
 *   k_tw_count       '\n' per 4 KiB block of the buffer (a block in front of lo returns at once), and the POSITION of the first
 *                    '\r' that is not followed by '\n' -- the buffer's last byte is never one: its line has not ended, it is
 *                    judged with the next submission, when the byte behind it is there.
 *   k_text_scan      (text_parse.h, as it is) the block counts' prefix sums, the number of lines.
 *   k_tw_fill        the position of every '\n', in order.
 *   k_tw_records     lane = record: line starts, the read's and the name's length, the checks of k_text_records; the first
 *                    record that fails one, and the first whose third line is longer than "+".
 *   k_text_offsets   (as it is, twice) read lengths -> CSR offsets, name lengths -> 64-bit name offsets.
 *   k_tw_verdict     ONE wave, the only serial point: the blocks' statuses, the counts against the capacities, the lone '\r'
 *                    against the cut, the header, and -- for status OK only -- the context's new state.
 *   k_text_gather    (as it is) bases and qualities into the CSR arrays; it reads the scratch record's TextHeader, whose status
 *                    the verdict sets for a refused submission.
 *   k_tw_names       a wave per record: its first line to the names; all blocks together save the new tail.
 *
 * A submission is taken whole or refused by status; a refused one counts nothing, leaves the tail as it was and sets
 * BamWalkState::refused, which every submission queued behind it reads (status CHAIN): bam_walk.h's rules.
 *
 * Bounds hold by construction, whatever the bytes: nothing in front of lo or behind hi is read; the line-break list takes at
 * most 4 * rec_cap positions and a record is looked at only when all four of its breaks are in it; line starts, lengths and
 * offsets are written below rec_cap (+ 1); more records than that, names beyond names_cap, bases beyond seq_cap and a tail
 * beyond tail_cap are a status, not a store.
 */
#ifndef FPL_TEXT_WALK_H
#define FPL_TEXT_WALK_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"
#include "text_parse.h"
#include "bam_walk.h" /* BamWalkState: the context's tail is one, whichever kind submitted last */

#include <algorithm>

namespace fpl {

constexpr u64 TW_NONE = ~0ull;

/* what the kernels of one submission hand each other */
struct TextWalkScratch {
    TextHeader reads; /* n_lines (k_text_scan), n_records, n_bases, max_len (k_text_offsets), status (k_text_gather reads it) */
    TextHeader names; /* n_records in, n_bases out: the bytes of all names */
    u64 cr_pos;       /* the first '\r' that is not followed by '\n' */
    u64 bad_rec;      /* the first record that fails a check of k_text_records */
    u64 strand_rec;   /* the first record that passes them with a third line longer than "+" */
    u64 cut;          /* k_tw_verdict -> k_tw_names: where the new tail starts */
};

struct TextWalkJob {
    u8* buf;
    u64 tail_cap, total;
    u32 rec_cap, nblk; /* records the arrays hold; 4 KiB blocks of [0, hi) */
    BamWalkState* st;
    u8* tail_buf; /* tail_cap bytes */
    const fpl_bgzf_block* blocks;
    u32 n_blocks;
    u32* blk;    /* nblk + 1 */
    u32* nl_pos; /* 4 * rec_cap */
    u32* line;   /* 4 * rec_cap */
    u32 *len, *nlen; /* rec_cap */
    TextWalkScratch* ws;
    fpl_text_window* hdr;
    uint64_t *off, *name_off; /* rec_cap + 1 */
    u8* names;
    u64 names_cap;
    u8 *seq, *qual;
    u64 seq_cap;
};

__device__ __forceinline__ u64 tw_lo(const TextWalkJob& j) { return j.tail_cap - min((u64)j.st->tail_len, j.tail_cap); }

/* the 16 bytes at `at` (a multiple of 16): bit i of nl / cr says that byte at + i lies in [lo, hi) and is '\n' / '\r' */
__device__ __forceinline__ void tw_masks(const u8* buf, u64 lo, u64 hi, u64 at, u32& nl, u32& cr) {
    nl = cr = 0;
    if (at >= hi || at + 16 <= lo) return;
    u32 w[4];
    tp_load16(buf, hi, at, w); /* (zeros behind hi) */
    const u32 keep = at < lo ? (0xFFFFu << (u32)(lo - at)) & 0xFFFFu : 0xFFFFu;
    nl = tp_eq_mask16(w, '\n') & keep;
    cr = tp_eq_mask16(w, '\r') & keep;
}
/* block b of the buffer holds none of the text (block-uniform) */
__device__ __forceinline__ bool tw_block_empty(u64 lo, u64 hi) {
    const u64 b0 = (u64)blockIdx.x * TP_BLOCK_BYTES;
    return b0 >= hi || b0 + TP_BLOCK_BYTES <= lo;
}

__global__ void __launch_bounds__(TP_THREADS) k_tw_place_tail(TextWalkJob j) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        TextWalkScratch s;
        s.reads.n_lines = s.reads.n_records = s.reads.status = s.reads.max_len = 0;
        s.reads.n_bases = 0;
        s.reads.bad_record = TW_NONE;
        s.names = s.reads;
        s.cr_pos = s.bad_rec = s.strand_rec = TW_NONE;
        s.cut = 0;
        *j.ws = s;
    }
    if (j.st->refused) return;
    const u32 tl = (u32)min((u64)j.st->tail_len, j.tail_cap);
    u8* dst = j.buf + (j.tail_cap - tl);
    for (u64 i = (u64)blockIdx.x * TP_THREADS + threadIdx.x; i < tl; i += (u64)gridDim.x * TP_THREADS) dst[i] = j.tail_buf[i];
}

__global__ void __launch_bounds__(TP_THREADS) k_tw_count(TextWalkJob j) {
    __shared__ u32 wsum[TP_THREADS / 64];
    const u64 hi = j.tail_cap + j.total, lo = tw_lo(j);
    if (j.st->refused || tw_block_empty(lo, hi)) { /* block-uniform */
        if (threadIdx.x == 0) j.blk[blockIdx.x] = 0;
        return;
    }
    const u64 at = (u64)blockIdx.x * TP_BLOCK_BYTES + 16ull * threadIdx.x;
    u32 nl, cr;
    tw_masks(j.buf, lo, hi, at, nl, cr);
    u64 odd = TW_NONE;
    if (cr) {
        /* every '\r' must have a '\n' behind it (byte 16 of this thread is the next thread's byte 0); the buffer's last byte has
           nothing behind it yet */
        u32 next_nl = nl >> 1;
        if (at + 16 < hi) {
            if (j.buf[at + 16] == '\n') next_nl |= 1u << 15;
        } else {
            next_nl |= 1u << (u32)(hi - 1 - at);
        }
        const u32 m = cr & ~next_nl;
        if (m) odd = at + (u64)(__ffs((int)m) - 1);
    }
    const u32 ws = wave_sum_u32((u32)__popc(nl));
    const u64 first = wave_min_u64(odd);
    if (lane_id() == 0) {
        wsum[wave_in_block()] = ws;
        if (first != TW_NONE) atomicMin((unsigned long long*)&j.ws->cr_pos, (unsigned long long)first);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 t = 0;
        for (int i = 0; i < TP_THREADS / 64; i++) t += wsum[i];
        j.blk[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(TP_THREADS) k_tw_fill(TextWalkJob j) {
    __shared__ u32 wsum[TP_THREADS / 64];
    const u64 hi = j.tail_cap + j.total, lo = tw_lo(j);
    if (j.st->refused || tw_block_empty(lo, hi)) return; /* block-uniform */
    const u64 at = (u64)blockIdx.x * TP_BLOCK_BYTES + 16ull * threadIdx.x;
    u32 nl, cr;
    tw_masks(j.buf, lo, hi, at, nl, cr);
    const u32 cnt = (u32)__popc(nl);
    const u32 incl = wave_scan_incl_u32(cnt);
    if (lane_id() == 63) wsum[wave_in_block()] = incl;
    __syncthreads();
    u32 k = j.blk[blockIdx.x] + incl - cnt;
    for (int i = 0; i < wave_in_block(); i++) k += wsum[i];
    const u32 nl_cap = 4u * j.rec_cap;
    while (nl) {
        const int b = __ffs((int)nl) - 1;
        nl &= nl - 1;
        if (k < nl_cap) j.nl_pos[k] = (u32)(at + (u64)b);
        k++;
    }
}

/* lane = record.  line[4 r + i] = where line i of record r starts; len[r] = its bases; nlen[r] = the bytes of its first line */
__global__ void __launch_bounds__(256) k_tw_records(TextWalkJob j) {
    if (j.st->refused) return;
    const u32 n_rec = min(j.ws->reads.n_lines / 4, j.rec_cap); /* (more than rec_cap: the verdict refuses) */
    const u32 lo = (u32)tw_lo(j);
    const u8* text = j.buf;
    if (blockIdx.x == 0 && threadIdx.x == 0) j.ws->reads.n_records = j.ws->names.n_records = n_rec;
    for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        u32 L[5];
        L[0] = r ? j.nl_pos[4 * r - 1] + 1u : lo;
#pragma unroll
        for (int i = 0; i < 4; i++) L[i + 1] = j.nl_pos[4 * r + i] + 1u;
        u32 ll[4]; /* line lengths without the line break */
#pragma unroll
        for (int i = 0; i < 4; i++) {
            u32 e = L[i + 1] - 1u; /* the '\n' */
            if (e > L[i] && text[e - 1] == '\r') e--;
            ll[i] = e - L[i];
            j.line[4 * (size_t)r + i] = L[i];
        }
        const bool good = ll[0] > 0 && text[L[0]] == '@' && ll[2] > 0 && text[L[2]] == '+' && ll[1] == ll[3];
        j.len[r] = ll[1];
        j.nlen[r] = ll[0];
        if (!good)
            atomicMin((unsigned long long*)&j.ws->bad_rec, (unsigned long long)r);
        else if (ll[2] > 1)
            atomicMin((unsigned long long*)&j.ws->strand_rec, (unsigned long long)r);
    }
}

__global__ void __launch_bounds__(WAVE) k_tw_verdict(TextWalkJob j) {
    const u32 lane = (u32)lane_id();
    const u64 hi = j.tail_cap + j.total, lo = tw_lo(j);
    fpl_text_window h;
    h.status = FPL_TXTW_OK;
    h.n_reads = 0;
    h.n_bases = 0;
    h.max_read_len = 0;
    h.n_lines = 0;
    h.name_bytes = 0;
    h.records_seen = j.st->rec_base;
    h.tail_bytes = 0;
    h.reserved = 0;
    h.bad_index = 0;
    h.bad_pos = 0;
    auto finish = [&](u32 status) {
        h.status = status;
        if (lane == 0) {
            *j.hdr = h;
            if (status != FPL_TXTW_OK) j.ws->reads.status = 1u; /* (k_text_gather, k_tw_names: nothing of it is used) */
            if (status != FPL_TXTW_OK && status != FPL_TXTW_CHAIN) j.st->refused = 1;
        }
    };
    if (uniform_u32(j.st->refused)) {
        finish(FPL_TXTW_CHAIN);
        return;
    }
    { /* a block k_bgzf_inflate did not vouch for: its bytes are undefined */
        u32 bad = ~0u;
        for (u32 i = lane; i < j.n_blocks; i += WAVE)
            if (j.blocks[i].status != FPL_BGZF_OK) {
                bad = i;
                break;
            }
        bad = wave_min_u32(bad);
        if (bad != ~0u) {
            h.bad_index = bad;
            finish(FPL_TXTW_BLOCK);
            return;
        }
    }
    const u32 n_lines = j.ws->reads.n_lines;
    const u32 n_rec = n_lines / 4;
    h.n_lines = n_lines;
    if (n_rec > j.rec_cap) {
        finish(FPL_TXTW_TOO_MANY);
        return;
    }
    const u64 cut = n_rec ? (u64)j.nl_pos[4 * (size_t)n_rec - 1] + 1 : lo;
    const u64 cr = j.ws->cr_pos, bad = j.ws->bad_rec, strand = j.ws->strand_rec;
    const bool lone_cr = cr < cut;
    if (lone_cr || (bad != TW_NONE && bad < strand)) {
        u64 pos = lone_cr ? cr : TW_NONE;
        if (bad != TW_NONE) pos = min(pos, (u64)j.line[4 * (size_t)bad]);
        h.bad_index = bad != TW_NONE ? j.st->rec_base + bad : TW_NONE;
        h.bad_pos = pos - lo;
        finish(FPL_TXTW_IRREGULAR);
        return;
    }
    if (strand != TW_NONE) {
        h.bad_index = j.st->rec_base + strand;
        h.bad_pos = (u64)j.line[4 * (size_t)strand] - lo;
        finish(FPL_TXTW_STRAND);
        return;
    }
    const u64 name_bytes = j.ws->names.n_bases, n_bases = j.ws->reads.n_bases;
    if (name_bytes > j.names_cap || n_bases > j.seq_cap) {
        finish(FPL_TXTW_TOO_MANY);
        return;
    }
    const u64 tail = hi - cut;
    h.tail_bytes = (u32)min(tail, (u64)0xFFFFFFFFu);
    if (tail > j.tail_cap) {
        finish(FPL_TXTW_TAIL_ROOM);
        return;
    }
    h.n_reads = n_rec;
    h.n_bases = n_bases;
    h.max_read_len = j.ws->reads.max_len;
    h.name_bytes = name_bytes;
    h.records_seen = j.st->rec_base + n_rec;
    if (lane == 0) {
        j.st->tail_len = (u32)tail;
        j.st->rec_base += n_rec;
        j.st->tail_src = cut;
        j.ws->cut = cut;
    }
    finish(FPL_TXTW_OK);
}

/* a wave per record: its first line, '@' included, to the names (16 bytes a lane and step; neither side is aligned); all
   blocks together: [cut, hi) into the context's tail buffer */
__global__ void __launch_bounds__(256) k_tw_names(TextWalkJob j) {
    if (j.hdr->status != FPL_TXTW_OK) return;
    const u64 hi = j.tail_cap + j.total;
    {
        const u64 tail = j.hdr->tail_bytes, src = j.ws->cut;
        if (tail <= j.tail_cap && src <= hi && hi - src >= tail)
            for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < tail; i += (u64)gridDim.x * blockDim.x) j.tail_buf[i] = j.buf[src + i];
    }
    const u32 n_rec = min(j.hdr->n_reads, j.rec_cap);
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    for (u32 r = wave; r < n_rec; r += n_waves) { /* wave-uniform */
        const u32 l = j.nlen[r];
        const uint64_t o = j.name_off[r];
        if (o + l > j.names_cap) continue; /* (cannot be: the verdict compared the sum) */
        const u8* src = j.buf + j.line[4 * (size_t)r];
        u8* dst = j.names + o;
        const u32 whole = l & ~15u;
        for (u32 i = 16 * lane; i < whole; i += 16 * 64) {
            u32x4 v;
            __builtin_memcpy(&v, src + i, 16);
            __builtin_memcpy(dst + i, &v, 16);
        }
        if (lane < (l & 15u)) dst[whole + lane] = src[whole + lane];
    }
}

#ifdef FPL_EMU
#define TW_LAUNCH(kernel, grid, block, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
typedef void* tw_stream_t;
#else
#define TW_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__)
typedef hipStream_t tw_stream_t;
#endif

/* records the arrays of a submission hold: one per 64 bytes of [tail room | inflated bytes] and 16, as for text; more is
   FPL_TXTW_TOO_MANY */
inline uint32_t text_walk_rec_cap(uint64_t hi) { return (uint32_t)(hi / 64 + 16); }
/* the sizes of a submission of `total` inflated bytes; false: the arguments are refused (line positions are 32 bits) */
inline bool text_walk_plan(TextWalkJob& j, uint64_t tail_cap, uint64_t total) {
    if (tail_cap > 0xFFFFFFF0ull || total > 0xFFFFFFF0ull || tail_cap + total > 0xFFFFFFF0ull) return false;
    const uint64_t hi = tail_cap + total;
    j.tail_cap = tail_cap;
    j.total = total;
    j.rec_cap = text_walk_rec_cap(hi);
    j.nblk = (u32)std::max<uint64_t>(1, (hi + TP_BLOCK_BYTES - 1) / TP_BLOCK_BYTES);
    return true;
}

/* the ten launches of one submission, in stream order (behind k_bgzf_inflate); wide: blocks of the record and gather kernels */
inline void text_walk_enqueue(const TextWalkJob& j, u32 wide, tw_stream_t s) {
    const u32 rblk = std::min<u32>(std::max<u32>(1u, (j.rec_cap + 255u) / 256u), std::max<u32>(1u, wide / 2));
    TW_LAUNCH(k_tw_place_tail, dim3(std::max<u32>(1, std::min<u32>(64, (u32)(j.tail_cap / TP_THREADS + 1)))), dim3(TP_THREADS), s, j);
    TW_LAUNCH(k_tw_count, dim3(j.nblk), dim3(TP_THREADS), s, j);
    TW_LAUNCH(k_text_scan, dim3(1), dim3(1024), s, j.blk, j.nblk, &j.ws->reads);
    TW_LAUNCH(k_tw_fill, dim3(j.nblk), dim3(TP_THREADS), s, j);
    TW_LAUNCH(k_tw_records, dim3(rblk), dim3(256), s, j);
    TW_LAUNCH(k_text_offsets, dim3(1), dim3(1024), s, (const u32*)j.len, j.rec_cap, &j.ws->reads, j.off);
    TW_LAUNCH(k_text_offsets, dim3(1), dim3(1024), s, (const u32*)j.nlen, j.rec_cap, &j.ws->names, j.name_off);
    TW_LAUNCH(k_tw_verdict, dim3(1), dim3(WAVE), s, j);
    TW_LAUNCH(k_text_gather, dim3(std::max<u32>(1u, wide)), dim3(256), s, (const u8*)j.buf, (const u32*)j.line, (const u32*)j.len,
              (const uint64_t*)j.off, (const TextHeader*)&j.ws->reads, j.rec_cap, j.seq, j.qual);
    TW_LAUNCH(k_tw_names, dim3(std::max<u32>(1u, wide)), dim3(256), s, j);
}

}  // namespace fpl
#endif
