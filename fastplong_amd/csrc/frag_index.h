/*
 * frag_index.h -- the order of a batch's fragment list, ON THE DEVICE (fpl_set_fragment_output, include/fastplong_amd.h).
 *
 * k_break_mask (kernels.h) appends a batch's fpl_fragment records with an atomic counter: entry e of the list is whichever
 * fragment got there e-th.  What a writer needs is the list by (read, seq_no) -- the order the reference writes the output
 * reads in, and the order fpl_get_fragments sorts into on the host.  A read's seq_no values are dense, 0 .. n_out - 1, so no
 * sort is needed: the place of an entry is first[read] + seq_no, where first[] is the exclusive prefix sum of the reads'
 * fragment counts -- exactly what fplh::FragmentList::index (host/format.cpp) builds.
 *
 *   k_frag_count   a lane per list entry: cnt[read]++ (cnt zeroed by the caller)
 *   k_frag_first   one block: first[r] = cnt[0] + .. + cnt[r - 1], first[n_reads] = the entries (the carry pattern of
 *                  k_emit_scan: EM_SCAN_BLOCKS values a step)
 *   k_frag_place   a lane per entry: order[first[read] + seq_no] = e (order filled with 0xFF bytes by the caller)
 *
 * Cost: two passes over 32-byte records, one over n_reads words.  fpl_read_result::n_frag is not used: it saturates at 255.
 *
 * The list is checked, not trusted: a list that overflowed (counts[2]), a count beyond the capacity, a read >= n_reads, a
 * seq_no >= its read's count or a sum that is not the list's length set FragIndex::status; whatever runs behind the index
 * asks frag_index_len(), which is 0 under a status, and writes nothing.  An entry of order[] that no fragment claimed (two fragments of one read
 * with one seq_no) stays 0xFFFFFFFF: frag_entry() says so, and the fragment counts as absent.
 */
#ifndef FPL_FRAG_INDEX_H
#define FPL_FRAG_INDEX_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"

namespace fpl {

constexpr int FI_THREADS = 256;
constexpr int FI_SCAN = 1024; /* counts k_frag_first takes per step: a thread each (EM_SCAN_BLOCKS) */
constexpr u32 FI_OVERFLOW = 1u;     /* status: a list of k_break_mask was too small for the batch */
constexpr u32 FI_INCONSISTENT = 2u; /* status: an entry names no read of the batch, or the seq_no of a read are not dense */
constexpr u32 FI_NONE = 0xFFFFFFFFu;

struct FragIndex {
    u32 n;      /* entries of order[]: the fragments of the batch (read through frag_index_len) */
    u32 status; /* 0, or FI_* bits: nothing behind the index may write */
};

/* the list as k_break_mask left it: counts[0] entries, counts[2] set when a list overflowed */
__device__ __forceinline__ u32 frag_list_len(const u32* __restrict__ counts, u32 frag_cap, FragIndex* __restrict__ fi) {
    const u32 n = counts[0];
    if (counts[2] || n > frag_cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&fi->status, FI_OVERFLOW);
        return 0;
    }
    return n;
}

__global__ void __launch_bounds__(FI_THREADS)
k_frag_count(const fpl_fragment* __restrict__ frags, const u32* __restrict__ counts, u32 frag_cap, u32 n_reads, u32* __restrict__ cnt,
             FragIndex* __restrict__ fi) {
    const u32 n = frag_list_len(counts, frag_cap, fi);
    for (u64 e = (u64)blockIdx.x * FI_THREADS + threadIdx.x; e < n; e += (u64)gridDim.x * FI_THREADS) {
        const u32 read = frags[e].read;
        if (read < n_reads) atomicAdd(&cnt[read], 1u);
        else atomicOr(&fi->status, FI_INCONSISTENT);
    }
}

/* one block: cnt[0 .. n_reads) -> first[0 .. n_reads]; fi->n */
__global__ void __launch_bounds__(FI_SCAN)
k_frag_first(const u32* __restrict__ cnt, u32 n_reads, const u32* __restrict__ counts, u32* __restrict__ first, FragIndex* __restrict__ fi) {
    __shared__ u32 w_sum[FI_SCAN / 64];
    __shared__ u64 carry; /* (64 bits: a sum that does not fit the list's 32 is a status, not a wrap) */
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (u32 base = 0; base < n_reads; base += FI_SCAN) { /* block-uniform */
        const u32 r = base + threadIdx.x;
        const u32 c = r < n_reads ? cnt[r] : 0u;
        const u32 ci = wave_scan_incl_u32(c);
        if (lane_id() == 63) w_sum[wave_in_block()] = ci;
        __syncthreads();
        u64 run = carry + ci - c;
        for (int k = 0; k < wave_in_block(); k++) run += w_sum[k];
        if (r < n_reads) first[r] = (u32)run;
        __syncthreads();
        if (threadIdx.x == FI_SCAN - 1) carry = run + c;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        first[n_reads] = (u32)carry;
        u32 st = fi->status;
        if (!st && carry != (u64)counts[0]) st = FI_INCONSISTENT; /* (an entry of a read >= n_reads was not counted) */
        fi->status = st;
        fi->n = st ? 0u : (u32)carry;
    }
}

__global__ void __launch_bounds__(FI_THREADS)
k_frag_place(const fpl_fragment* __restrict__ frags, const u32* __restrict__ cnt, const u32* __restrict__ first, u32 n_reads,
             u32* __restrict__ order, FragIndex* __restrict__ fi) {
    const u32 n = fi->n; /* (0 under a status of the kernels before) */
    for (u64 e = (u64)blockIdx.x * FI_THREADS + threadIdx.x; e < n; e += (u64)gridDim.x * FI_THREADS) {
        const u32 read = frags[e].read, seq_no = frags[e].seq_no;
        if (read < n_reads && seq_no < cnt[read]) order[first[read] + seq_no] = (u32)e; /* (first[read] + cnt[read] <= n) */
        else atomicOr(&fi->status, FI_INCONSISTENT);
    }
}

/* what runs behind the index: how many ordered fragments there are, and the list entry of the j-th (FI_NONE: nobody's) */
__device__ __forceinline__ u32 frag_index_len(const FragIndex* __restrict__ fi) { return fi->status ? 0u : fi->n; }
__device__ __forceinline__ u32 frag_entry(const u32* __restrict__ order, u32 j, u32 n) {
    const u32 e = order[j];
    return e < n ? e : FI_NONE;
}

/* Read::maskRegionWithN as the host's append_masked (host/format.cpp) clips it, for the fragment [start, start + len) of its
   read: a region that starts in front of the fragment or at / behind its end is skipped, the others are cut to its end.
   -> the region's place INSIDE the fragment */
__device__ __forceinline__ bool frag_clip_region(const fpl_region& rg, u32 start, u32 len, u32& a, u32& l) {
    if (rg.start < start || rg.start - start >= len) return false;
    a = rg.start - start;
    l = rg.len < len - a ? rg.len : len - a;
    return true;
}

/* the grid of k_frag_count / k_frag_place for a list of at most frag_cap entries (how many there are only the device knows) */
inline u32 frag_index_blocks(u64 frag_cap, u32 n_cu) {
    const u64 blocks = (frag_cap + FI_THREADS - 1) / FI_THREADS;
    const u64 cap = 8ull * n_cu;
    return (u32)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

}  // namespace fpl
#endif
