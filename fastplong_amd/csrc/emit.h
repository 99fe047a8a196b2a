/*
 * emit.h -- the passing, trimmed reads of a CSR batch as a CSR batch, ON THE DEVICE (fpl_emit_batch_device,
 * include/fastplong_amd.h).
 *
 * fpl_process_batch_device leaves one record per read; what a writer makes of the records -- every fragment with code
 * FPL_PASS_FILTER of every read that was not dropped, in input order, fragment 0 before fragment 1 (format_range,
 * host/format.cpp) -- these kernels make where the bases are, so that a second device-side consumer never meets the host:
 *
 *   k_emit_count   lane = read: its passing fragments and their bytes; per block of EM_LAYOUT_READS reads the sums, the
 *                  longest fragment and whether a window reaches outside its read
 *   k_emit_scan    one block: exclusive prefix sums of the block sums (EM_SCAN_BLOCKS of them per step), the totals, the
 *                  verdict: the info record, d_off_out[0]
 *   k_emit_fill    lane = read again: d_off_out, d_src, d_kind, and per output read where its bytes come from (EmitFrom)
 *   k_emit_gather  the copy.  Cut by OUTPUT BYTES: a wave owns tiles of EM_TILE bytes of the output (the same range of the
 *                  bases and of the qualities), a lane 16 destination bytes per step.
 *
 * The records are the caller's memory and may hold anything.  k_emit_count vouches for every window it counts
 * (frag_start + frag_len inside the read), k_emit_scan for the totals against the capacities; the fill and the gather run
 * only behind a zero status and then cannot read outside a read or write outside the capacities.
 *
 * With fpl_set_fragment_output on a --break / --mask context the output reads are the ordered fragments of the context's last
 * batch (frag_index.h): k_emit_count_frag / k_emit_fill_frag in place of the count and the fill, k_emit_mask behind the gather
 * (at the end of this file).
 */
#ifndef FPL_EMIT_H
#define FPL_EMIT_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"
#include "frag_index.h"

namespace fpl {

constexpr int EM_LAYOUT_READS = 256; /* reads per block of k_emit_count / k_emit_fill: a thread each */
constexpr int EM_SCAN_BLOCKS = 1024; /* block sums k_emit_scan takes per step: a thread each */
constexpr u32 EM_STEP = 16 * 64;     /* output bytes a wave copies per step */
constexpr u32 EM_TILE = 32 * EM_STEP; /* output bytes per tile: one search of d_off_out pays for 32 steps */
constexpr int EM_GATHER_THREADS = 256;
constexpr u32 EM_BAD = 0x80000000u; /* in a block's count word: one of its windows reaches outside its read */

/* where output read j comes from: source byte offset minus destination byte offset, the same for bases and qualities */
typedef u64 EmitFrom;

struct EmitRead {
    bool take[2]; /* fragment f is put out */
    u32 len[2];   /* 0 where it is not */
    u32 start[2];
    u8 kind[2];
    bool bad;
    __device__ __forceinline__ u32 n() const { return (take[0] ? 1u : 0u) + (take[1] ? 1u : 0u); }
    __device__ __forceinline__ u64 bytes() const { return (u64)len[0] + len[1]; }
};

/* what read i puts out: the record is not trusted, the offsets are the caller's promise (non-decreasing) */
__device__ __forceinline__ EmitRead em_read(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 i) {
    EmitRead e = {};
    const fpl_read_result r = res[i];
    if (r.dropped) return e;
    const u64 o0 = off[i], o1 = off[i + 1];
    const u64 rlen = o1 >= o0 ? o1 - o0 : 0;
#pragma unroll
    for (int f = 0; f < 2; f++) {
        if (f >= r.n_frag || r.code[f] != FPL_PASS_FILTER) continue;
        if ((u64)r.frag_start[f] + r.frag_len[f] > rlen) e.bad = true;
        e.take[f] = true;
        e.len[f] = r.frag_len[f];
        e.start[f] = r.frag_start[f];
        e.kind[f] = r.kind[f];
    }
    return e;
}

/* inclusive prefix sum across the lanes of 64-bit values */
__device__ __forceinline__ u64 em_wave_scan_incl_u64(u64 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = shfl_u64(v, lane_id() - d < 0 ? lane_id() : lane_id() - d);
        if (lane_id() >= d) v += up;
    }
    return v;
}

__global__ void __launch_bounds__(EM_LAYOUT_READS)
k_emit_count(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_reads, u32* __restrict__ blk_cnt,
             u64* __restrict__ blk_bytes, u32* __restrict__ blk_max) {
    __shared__ u32 w_cnt[EM_LAYOUT_READS / 64], w_max[EM_LAYOUT_READS / 64];
    __shared__ u64 w_bytes[EM_LAYOUT_READS / 64];
    const u64 i = (u64)blockIdx.x * EM_LAYOUT_READS + threadIdx.x;
    EmitRead e = {};
    if (i < n_reads) e = em_read(off, res, (u32)i);
    const u32 cnt = wave_sum_u32(e.n() | (e.bad ? 1u << 16 : 0u)); /* (at most 128 fragments a wave: the flags add up above them) */
    const u32 mx = wave_max_u32(max(e.len[0], e.len[1]));
    const u64 by = em_wave_scan_incl_u64(e.bytes());
    if (lane_id() == 63) {
        w_cnt[wave_in_block()] = cnt;
        w_max[wave_in_block()] = mx;
        w_bytes[wave_in_block()] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0, m = 0;
        u64 b = 0;
        for (int k = 0; k < EM_LAYOUT_READS / 64; k++) {
            c += w_cnt[k];
            m = max(m, w_max[k]);
            b += w_bytes[k];
        }
        blk_cnt[blockIdx.x] = (c & 0xFFFFu) | (c >> 16 ? EM_BAD : 0u);
        blk_max[blockIdx.x] = m;
        blk_bytes[blockIdx.x] = b;
    }
}

/* one block: blk_cnt[b] / blk_bytes[b] -> the output reads / bytes in front of block b; the info record */
__global__ void __launch_bounds__(EM_SCAN_BLOCKS)
k_emit_scan(u32* __restrict__ blk_cnt, u64* __restrict__ blk_bytes, const u32* __restrict__ blk_max, u32 nblk, u64 out_cap_bytes,
            u32 out_cap_reads, uint64_t* __restrict__ off_out, fpl_emit_info* __restrict__ info) {
    __shared__ u32 w_cnt[EM_SCAN_BLOCKS / 64], w_max[EM_SCAN_BLOCKS / 64], w_bad[EM_SCAN_BLOCKS / 64];
    __shared__ u64 w_bytes[EM_SCAN_BLOCKS / 64];
    __shared__ u64 carry_cnt, carry_bytes; /* (the reads are counted in 64 bits: 2^31 fits a u32, the test against the capacity is simpler so) */
    if (threadIdx.x == 0) carry_cnt = 0, carry_bytes = 0;
    u32 mx = 0, bad = 0;
    __syncthreads();
    for (u32 base = 0; base < nblk; base += EM_SCAN_BLOCKS) { /* block-uniform */
        const u32 b = base + threadIdx.x;
        const u32 raw = b < nblk ? blk_cnt[b] : 0u;
        const u32 c = raw & ~EM_BAD;
        const u64 y = b < nblk ? blk_bytes[b] : 0ull;
        bad |= raw & EM_BAD;
        mx = max(mx, b < nblk ? blk_max[b] : 0u);
        const u32 ci = wave_scan_incl_u32(c);
        const u64 yi = em_wave_scan_incl_u64(y);
        if (lane_id() == 63) {
            w_cnt[wave_in_block()] = ci;
            w_bytes[wave_in_block()] = yi;
        }
        __syncthreads();
        u64 rc = carry_cnt + ci - c, ry = carry_bytes + yi - y;
        for (int k = 0; k < wave_in_block(); k++) {
            rc += w_cnt[k];
            ry += w_bytes[k];
        }
        if (b < nblk) {
            blk_cnt[b] = (u32)rc; /* (below 2^31 for n_reads <= 2^30) */
            blk_bytes[b] = ry;
        }
        __syncthreads();
        if (threadIdx.x == EM_SCAN_BLOCKS - 1) carry_cnt = rc + c, carry_bytes = ry + y;
        __syncthreads();
    }
    const u32 wm = wave_max_u32(mx);
    const u64 wb = wave_ballot(bad != 0);
    if (lane_id() == 0) {
        w_max[wave_in_block()] = wm;
        w_bad[wave_in_block()] = wb ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 m = 0, st = 0;
        for (int k = 0; k < EM_SCAN_BLOCKS / 64; k++) {
            m = max(m, w_max[k]);
            if (w_bad[k]) st |= 1u;
        }
        if (carry_cnt > out_cap_reads || carry_bytes > out_cap_bytes) st |= 2u;
        fpl_emit_info o = {};
        o.status = st;
        if (!st) {
            o.n_bytes = carry_bytes;
            o.n_out = (u32)carry_cnt;
            o.max_len = m;
        }
        *info = o;
        off_out[0] = 0;
    }
}

__global__ void __launch_bounds__(EM_LAYOUT_READS)
k_emit_fill(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_reads, const u32* __restrict__ blk_cnt,
            const u64* __restrict__ blk_bytes, const fpl_emit_info* __restrict__ info, uint64_t* __restrict__ off_out,
            u32* __restrict__ src, u8* __restrict__ kind, EmitFrom* __restrict__ from) {
    __shared__ u32 w_cnt[EM_LAYOUT_READS / 64];
    __shared__ u64 w_bytes[EM_LAYOUT_READS / 64];
    if (info->status) return; /* block-uniform: nothing of a refused batch is written */
    const u64 i = (u64)blockIdx.x * EM_LAYOUT_READS + threadIdx.x;
    EmitRead e = {};
    if (i < n_reads) e = em_read(off, res, (u32)i);
    const u64 y = e.bytes();
    const u32 n = e.n();
    const u32 ci = wave_scan_incl_u32(n);
    const u64 yi = em_wave_scan_incl_u64(y);
    if (lane_id() == 63) {
        w_cnt[wave_in_block()] = ci;
        w_bytes[wave_in_block()] = yi;
    }
    __syncthreads();
    u64 j = (u64)blk_cnt[blockIdx.x] + ci - n;
    u64 at = blk_bytes[blockIdx.x] + yi - y;
    for (int k = 0; k < wave_in_block(); k++) {
        j += w_cnt[k];
        at += w_bytes[k];
    }
#pragma unroll
    for (int f = 0; f < 2; f++) {
        if (!e.take[f]) continue;
        from[j] = off[i] + e.start[f] - at;
        at += e.len[f];
        off_out[j + 1] = at;
        if (src) src[j] = (u32)i;
        if (kind) kind[j] = e.kind[f];
        j++;
    }
}

/* 64 values of a wave that every lane reads at wave-uniform indices (v_readlane on the device; the emulator takes one
   snapshot instead of a rendezvous per read) */
struct EmWave32 {
#ifdef FPL_EMU
    u64 vals[64];
    u32 get(int t) const { return (u32)vals[t]; }
#else
    u32 v;
    __device__ __forceinline__ u32 get(int t) const { return readlane_u32(v, t); }
#endif
};
__device__ __forceinline__ EmWave32 em_publish(u32 v) {
    EmWave32 w;
#ifdef FPL_EMU
    emu_gather_u64(v, w.vals);
#else
    w.v = v;
#endif
    return w;
}

/* the largest j in [0, n_out) with off_out[j] <= t (t < off_out[n_out]): the read that holds output byte t.  Every lane
   probes one of 64 evenly spread entries per round: four rounds for two million reads */
__device__ __forceinline__ u32 em_search(const uint64_t* __restrict__ off_out, u32 n_out, u64 t) {
    u32 lo = 0, hi = n_out; /* off_out[lo] <= t < off_out[hi] */
    for (;;) {              /* wave-uniform */
        const u32 span = hi - lo;
        const u32 step = span > 64 ? (span + 63) / 64 : 1u;
        const u64 want = (u64)lo + (u64)step * (u32)lane_id();
        const u32 idx = want < hi ? (u32)want : hi;
        const u32 k = (u32)__popcll(wave_ballot(off_out[idx] <= t)) - 1u; /* (lane 0 probes lo: at least one) */
        lo = uniform_u32(lo + step * k);
        if (step == 1) return lo;
        hi = (u64)lo + step < hi ? lo + step : hi;
    }
}

/* a lane's 16 destination bytes [p, p + 16) -- fewer at the end t1 of the output --, the first of which lies in output read r */
__device__ __forceinline__ void em_copy16(const u8* __restrict__ seq, const u8* __restrict__ qual, const uint64_t* __restrict__ off_out,
                                          const EmitFrom* __restrict__ from, u8* __restrict__ seq_out, u8* __restrict__ qual_out, u64 p,
                                          u64 t1, u32 r) {
    u64 end_r = off_out[(u64)r + 1];
    EmitFrom d = from[r];
    if (p + 16 <= end_r) { /* (then p + 16 <= t1 too: t1 is the output's end, or a tile's, a multiple of 16 from p) */
        const u32x4 a = load16(seq + (p + d)), b = load16(qual + (p + d));
        __builtin_memcpy(seq_out + p, &a, 16);
        __builtin_memcpy(qual_out + p, &b, 16);
        return;
    }
    /* over a boundary between reads, or the last bytes of the output: collected byte by byte, stored at once when whole */
    u32 a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    const u32 nb = p + 16 <= t1 ? 16u : (u32)(t1 - p);
#pragma unroll
    for (u32 k = 0; k < 16; k++) { /* (unrolled: the words stay in registers) */
        if (k < nb) {
            const u64 pos = p + k;
            while (pos >= end_r) { /* (stops at the last read at the latest: pos < t1 <= its end) */
                r++;
                end_r = off_out[(u64)r + 1];
                d = from[r];
            }
            a[k >> 2] |= (u32)seq[pos + d] << (8 * (k & 3));
            b[k >> 2] |= (u32)qual[pos + d] << (8 * (k & 3));
        }
    }
    if (nb == 16) {
        const u32x4 va = {a[0], a[1], a[2], a[3]}, vb = {b[0], b[1], b[2], b[3]};
        __builtin_memcpy(seq_out + p, &va, 16);
        __builtin_memcpy(qual_out + p, &vb, 16);
    } else {
#pragma unroll
        for (u32 k = 0; k < 16; k++)
            if (k < nb) {
                seq_out[p + k] = (u8)(a[k >> 2] >> (8 * (k & 3)));
                qual_out[p + k] = (u8)(b[k >> 2] >> (8 * (k & 3)));
            }
    }
}

/* Tiles of EM_TILE output bytes, dealt to the waves round-robin.  Per step of EM_STEP bytes a lane owns 16 destination bytes
   at p = base + 16 * lane; the read that holds byte p is `cur` (the one that holds the step's first byte) plus the number of
   reads that end at or in front of p: the ends of 64 reads at a time sit in the lanes, and every lane counts, at wave-uniform
   indices, those not behind its p -- the count stops at the first end behind the step, so a step inside one long read looks at
   one end and a step over 20-byte reads at fifty.  A lane whose 16 bytes lie in one read moves them with one 16-byte load and
   one 16-byte store per array (neither side need be aligned: gfx950 global accesses take any address; the stores are aligned
   when the caller's arrays are); a lane over a boundary between reads, or over the end of the output, collects byte by byte. */
__global__ void __launch_bounds__(EM_GATHER_THREADS)
k_emit_gather(const u8* __restrict__ seq, const u8* __restrict__ qual, const uint64_t* __restrict__ off_out,
              const EmitFrom* __restrict__ from, const fpl_emit_info* __restrict__ info, u8* __restrict__ seq_out,
              u8* __restrict__ qual_out) {
    if (info->status) return;
    const u64 n_bytes = info->n_bytes;
    const u32 n_out = info->n_out;
    const u64 n_tiles = (n_bytes + EM_TILE - 1) / EM_TILE;
    const u32 wave = (u32)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (u32)((gridDim.x * blockDim.x) >> 6);
    const u32 lane = (u32)lane_id();
    for (u64 tile = wave; tile < n_tiles; tile += n_waves) { /* wave-uniform */
        const u64 t0 = tile * EM_TILE, t1 = min(t0 + EM_TILE, n_bytes);
        u32 cur = em_search(off_out, n_out, t0);
        for (u64 base = t0; base < t1; base += EM_STEP) { /* wave-uniform */
            const u32 prel = 16 * lane;
            const u64 p = base + prel;
            u32 r = cur;
            for (u32 w = cur;; w += 64) { /* wave-uniform: windows of 64 ends */
                const u64 at = (u64)w + lane + 1;
                const u64 end = off_out[at < n_out ? at : n_out];
                const u32 rel = end <= base ? 0u : (end - base > EM_STEP ? EM_STEP : (u32)(end - base));
                const EmWave32 ends = em_publish(rel);
                bool more = true;
                for (int l = 0; l < 64; l++) {
                    const u32 s = ends.get(l);
                    /* an end behind the last lane's p, or the last read's: nothing further counts */
                    if (s > EM_STEP - 16 || (u64)w + l + 1 >= n_out) {
                        more = false;
                        break;
                    }
                    r += s <= prel ? 1u : 0u;
                }
                if (!more) break;
            }
            if (r >= n_out) r = n_out - 1; /* (lanes behind the end of the output) */
            cur = uniform_u32(shfl_u32(r, 63));
            if (p < t1) em_copy16(seq, qual, off_out, from, seq_out, qual_out, p, t1, r);
        }
    }
}

/* ---- the fragment forms (fpl_set_fragment_output): the output reads of a --break / --mask batch ----
   The reads are the batch's fragment list in the order frag_index.h makes: k_emit_count_frag and k_emit_fill_frag are the count
   and the fill with a lane per ordered fragment -- blocks of EM_LAYOUT_READS fragments, as many as the list's CAPACITY asks for
   (how many fragments there are only the device knows; the blocks behind them count nothing) --, k_emit_scan and k_emit_gather
   run unchanged on what they leave, and k_emit_mask writes N over the regions behind the gather.  The caller's records say which
   reads are dropped and nothing else. */
struct EmitFrag {
    bool take, bad;
    fpl_fragment f;
};
__device__ __forceinline__ EmitFrag em_frag(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_reads,
                                            const fpl_fragment* __restrict__ frags, const u32* __restrict__ order, u32 j, u32 n) {
    EmitFrag e = {};
    const u32 ent = frag_entry(order, j, n);
    if (ent == FI_NONE) return e;
    e.f = frags[ent];
    if (e.f.code != FPL_PASS_FILTER || e.f.read >= n_reads || res[e.f.read].dropped) return e;
    const u64 o0 = off[e.f.read], o1 = off[(u64)e.f.read + 1];
    e.take = true;
    e.bad = (u64)e.f.start + e.f.len > (o1 >= o0 ? o1 - o0 : 0);
    return e;
}
__global__ void __launch_bounds__(EM_LAYOUT_READS)
k_emit_count_frag(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_reads, const fpl_fragment* __restrict__ frags,
                  const u32* __restrict__ order, const FragIndex* __restrict__ fi, u32* __restrict__ blk_cnt, u64* __restrict__ blk_bytes,
                  u32* __restrict__ blk_max) {
    __shared__ u32 w_cnt[EM_LAYOUT_READS / 64], w_max[EM_LAYOUT_READS / 64];
    __shared__ u64 w_bytes[EM_LAYOUT_READS / 64];
    const u32 n = frag_index_len(fi);
    const u64 j = (u64)blockIdx.x * EM_LAYOUT_READS + threadIdx.x;
    EmitFrag e = {};
    if (j < n) e = em_frag(off, res, n_reads, frags, order, (u32)j, n);
    const u32 len = e.take ? e.f.len : 0u;
    const u32 cnt = wave_sum_u32((e.take ? 1u : 0u) | (e.bad ? 1u << 16 : 0u));
    const u32 mx = wave_max_u32(len);
    const u64 by = em_wave_scan_incl_u64(len);
    if (lane_id() == 63) {
        w_cnt[wave_in_block()] = cnt;
        w_max[wave_in_block()] = mx;
        w_bytes[wave_in_block()] = by;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0, m = 0;
        u64 b = 0;
        for (int k = 0; k < EM_LAYOUT_READS / 64; k++) {
            c += w_cnt[k];
            m = max(m, w_max[k]);
            b += w_bytes[k];
        }
        blk_cnt[blockIdx.x] = (c & 0xFFFFu) | (c >> 16 ? EM_BAD : 0u);
        blk_max[blockIdx.x] = m;
        blk_bytes[blockIdx.x] = b;
    }
}
/* ent[j]: the list entry of output read j (k_emit_mask finds its regions there); break_no may be nullptr.  A status of the index
   becomes bit 2 of the info record here: the count saw an empty list, so everything else in the record is zero already */
__global__ void __launch_bounds__(EM_LAYOUT_READS)
k_emit_fill_frag(const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_reads, const fpl_fragment* __restrict__ frags,
                 const u32* __restrict__ order, const FragIndex* __restrict__ fi, const u32* __restrict__ blk_cnt,
                 const u64* __restrict__ blk_bytes, fpl_emit_info* __restrict__ info, uint64_t* __restrict__ off_out, u32* __restrict__ src,
                 u8* __restrict__ kind, uint16_t* __restrict__ break_no, EmitFrom* __restrict__ from, u32* __restrict__ ent) {
    __shared__ u32 w_cnt[EM_LAYOUT_READS / 64];
    __shared__ u64 w_bytes[EM_LAYOUT_READS / 64];
    if (fi->status) { /* block-uniform */
        if (blockIdx.x == 0 && threadIdx.x == 0) info->status |= 4u;
        return;
    }
    if (info->status) return; /* block-uniform: nothing of a refused batch is written */
    const u32 n = fi->n;
    const u64 j0 = (u64)blockIdx.x * EM_LAYOUT_READS + threadIdx.x;
    EmitFrag e = {};
    if (j0 < n) e = em_frag(off, res, n_reads, frags, order, (u32)j0, n);
    const u64 y = e.take ? e.f.len : 0u;
    const u32 c = e.take ? 1u : 0u;
    const u32 ci = wave_scan_incl_u32(c);
    const u64 yi = em_wave_scan_incl_u64(y);
    if (lane_id() == 63) {
        w_cnt[wave_in_block()] = ci;
        w_bytes[wave_in_block()] = yi;
    }
    __syncthreads();
    u64 j = (u64)blk_cnt[blockIdx.x] + ci - c;
    u64 at = blk_bytes[blockIdx.x] + yi - y;
    for (int k = 0; k < wave_in_block(); k++) {
        j += w_cnt[k];
        at += w_bytes[k];
    }
    if (!e.take) return;
    from[j] = off[e.f.read] + e.f.start - at;
    off_out[j + 1] = at + e.f.len;
    ent[j] = order[j0];
    if (src) src[j] = e.f.read;
    if (kind) kind[j] = e.f.kind;
    if (break_no) break_no[j] = e.f.break_no;
}
/* behind the gather, on its stream: a wave per output read whose fragment has regions writes N over them in seq_out
   (frag_clip_region: the clipping of the host's append_masked).  The gather's stores are done -- a kernel boundary --, so the
   order of the two writes to a masked byte is not a question. */
__global__ void __launch_bounds__(EM_GATHER_THREADS)
k_emit_mask(const fpl_fragment* __restrict__ frags, const fpl_region* __restrict__ regs, const u32* __restrict__ ent,
            const uint64_t* __restrict__ off_out, const fpl_emit_info* __restrict__ info, u8* __restrict__ seq_out) {
    if (info->status) return;
    const u32 n_out = info->n_out;
    const u32 wave = (u32)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), n_waves = (u32)((gridDim.x * blockDim.x) >> 6);
    const u32 lane = (u32)lane_id();
    for (u32 j = wave; j < n_out; j += n_waves) { /* wave-uniform */
        const fpl_fragment f = frags[ent[j]];
        u8* const d = seq_out + off_out[j];
        for (u32 k = 0; k < f.region_count; k++) {
            u32 a, l;
            if (!frag_clip_region(regs[f.region_first + k], f.start, f.len, a, l)) continue;
            for (u32 i = lane; i < l; i += 64) d[a + i] = (u8)'N';
        }
    }
}

/* the grid of k_emit_gather for an output of at most cap_bytes: a wave per tile, no more blocks than keep every CU full */
inline u32 emit_gather_blocks(u64 cap_bytes, u32 n_cu) {
    const u64 tiles = (cap_bytes + EM_TILE - 1) / EM_TILE;
    const u64 blocks = (tiles + EM_GATHER_THREADS / 64 - 1) / (EM_GATHER_THREADS / 64);
    const u64 cap = 8ull * n_cu;
    return (u32)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

}  // namespace fpl
#endif
