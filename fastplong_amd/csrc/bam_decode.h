/*
 * bam_decode.h -- BAM records -> CSR batch ON THE DEVICE (fpl_process_bam_async / fpl_decode_bam, include/fastplong_amd.h).
 *
 * The host inflates a BAM's BGZF blocks and walks its records (host/bam.cpp): it uploads the inflated record bytes as they
 * are, with the byte offset of every record's start and the CSR offsets of the output (n + 1, from l_seq).  This kernel reads
 * each record's fixed fields itself (l_read_name +12, n_cigar_op +16, flag +18, l_seq +20, the name at +36), finds the packed
 * bases (4-bit codes "=ACMGRSVTWYHKDBN", high nibble first) and the raw phred qualities behind them, and writes ASCII bases and
 * min(qual, 93) + 33 where the per-read kernels expect a batch (csrc/pipeline.h).  Flag 0x10: the bases are reverse-complemented
 * (the complement of a code is its four bits reversed, "=TGKCYSBAWRDMHVN") and the qualities reversed -- `samtools fastq`'s
 * twin of the record.
 *
 * Shape: one lane per 16 bytes of OUTPUT, aligned to 16 bytes of the output arrays, whatever the reads' lengths.  A lane finds
 * the read(s) its 16 bytes belong to (a binary search inside the block's range of reads), decodes the 16 bases and qualities of
 * each, and writes both 16-byte words with one store each -- only the last word of the batch is partial.  Reads of 1 base and of
 * 1.2 Mb mix freely: a short read is a piece of some lane's word, a long one spreads over as many lanes as it has words, so no
 * lane idles on a short read (the trims need their lane-per-read / wave-per-read forms because their work is per read; this
 * kernel's is per byte).  Loads are unaligned 16-byte loads of the packed bases (9 bytes used) and of the qualities; the nibble
 * decode is two v_perm_b32 lookups per 4 bases and a byte select, no branch per base.
 */
#ifndef FPL_BAM_DECODE_H
#define FPL_BAM_DECODE_H

#include "dev_prims.h"

namespace fpl {

constexpr int BAM_THREADS = 256;
constexpr int BAM_PAD = 64; /* bytes the record buffer must hold behind its end: the 16-byte loads of a read's last word run over */

/* the 16 codes as ASCII, 4 per dword (byte k of word k / 4 = code k) */
constexpr u32 BAM_FWD[4] = {0x4D43413Du /* =ACM */, 0x56535247u /* GRSV */, 0x48595754u /* TWYH */, 0x4E42444Bu /* KDBN */};
constexpr u32 BAM_REV[4] = {0x4B47543Du /* =TGK */, 0x42535943u /* CYSB */, 0x44525741u /* AWRD */, 0x4E56484Du /* MHVN */};

/* v_perm_b32: byte i of the result = byte sel_i of the 8-byte pool {lo (bytes 0-3), hi (bytes 4-7)}; sel bytes < 8 only */
__device__ __forceinline__ u32 bam_perm(u32 hi, u32 lo, u32 sel) {
#ifdef FPL_EMU
    const u64 pool = ((u64)hi << 32) | lo;
    u32 r = 0;
    for (int i = 0; i < 4; i++) r |= (u32)((pool >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return r;
#else
    return __builtin_amdgcn_perm(hi, lo, sel);
#endif
}

/* four 4-bit codes (one per byte of `codes`) -> four ASCII bytes of table t */
__device__ __forceinline__ u32 bam_lookup4(u32 codes, const u32 (&t)[4]) {
    const u32 s = codes & 0x07070707u;
    const u32 lo = bam_perm(t[1], t[0], s), hi = bam_perm(t[3], t[2], s);
    const u32 m = ((codes >> 3) & 0x01010101u) * 0xFFu;
    return (hi & m) | (lo & ~m);
}

__device__ __forceinline__ u32x4 bam_load16(const u8* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

/* the 16 codes of nibbles k .. k + 15 of the packed bases at `sq` (k may be negative: the bytes in front are the record's own) */
__device__ __forceinline__ void bam_codes16(const u8* sq, long long k, u32 (&c)[4]) {
    const u32x4 v = bam_load16(sq + (k >> 1)); /* (an arithmetic shift: floor for negative k) */
    u64 y = (u64)v.x | ((u64)v.y << 32);
    if (k & 1) /* start on a low nibble: shift the byte stream by half a byte (byte i = low nibble of i, high nibble of i + 1) */
        y = ((y & 0x0F0F0F0F0F0F0F0Full) << 4) | ((y >> 12) & 0x000F0F0F0F0F0F0Full) | ((u64)((v.z >> 4) & 0xF) << 56);
    const u64 H = (y >> 4) & 0x0F0F0F0F0F0F0F0Full, L = y & 0x0F0F0F0F0F0F0F0Full;
    const u32 h0 = (u32)H, h1 = (u32)(H >> 32), l0 = (u32)L, l1 = (u32)(L >> 32);
    /* interleave: base 2i = high nibble of byte i, base 2i + 1 its low nibble */
    c[0] = bam_perm(h0, l0, 0x01050004u);
    c[1] = bam_perm(h0, l0, 0x03070206u);
    c[2] = bam_perm(h1, l1, 0x01050004u);
    c[3] = bam_perm(h1, l1, 0x03070206u);
}

/* four raw phred bytes -> min(q, 93) + 33, bytewise in one register: bit 7 of a byte of gt is set when the byte is >= 94 (its low
   seven bits + 34 reach 128, or its own bit 7 is set; no carry crosses a byte), and such bytes become 93 */
__device__ __forceinline__ u32 bam_clamp_q4(u32 x) {
    const u32 gt = (((x & 0x7F7F7F7Fu) + 0x22222222u) | x) & 0x80808080u;
    const u32 m = (gt >> 7) * 0xFFu;
    return ((x & ~m) | (0x5D5D5D5Du & m)) + 0x21212121u;
}

__device__ __forceinline__ u32 bam_bswap(u32 x) {
#ifdef FPL_EMU
    return __builtin_bswap32(x);
#else
    return __builtin_amdgcn_perm(0u, x, 0x00010203u);
#endif
}

/* bytes [p, p + 16) of read r's output (p relative to the read's start; only the bytes inside [0, l) are meaningful) */
__device__ __forceinline__ void bam_piece(const u8* __restrict__ bam, uint64_t rs, long long p, u32x4& sb, u32x4& qb) {
    const u8* rec = bam + rs;
    const u32x4 h = bam_load16(rec + 8); /* bytes 8..23: l_read_name (12), n_cigar_op (16), flag (18), l_seq (20) in one load */
    const u32 l_name = h.y & 0xFFu;
    const u32 n_cigar = h.z & 0xFFFFu;
    const u32 flag = h.z >> 16;
    const long long l = (long long)h.w;
    const u8* sq = rec + 36 + l_name + 4 * (size_t)n_cigar;
    const u8* ql = sq + ((l + 1) >> 1);
    u32 c[4];
    if (!(flag & 0x10u)) {
        bam_codes16(sq, p, c);
        sb.x = bam_lookup4(c[0], BAM_FWD);
        sb.y = bam_lookup4(c[1], BAM_FWD);
        sb.z = bam_lookup4(c[2], BAM_FWD);
        sb.w = bam_lookup4(c[3], BAM_FWD);
        const u32x4 q = bam_load16(ql + p);
        qb.x = bam_clamp_q4(q.x);
        qb.y = bam_clamp_q4(q.y);
        qb.z = bam_clamp_q4(q.z);
        qb.w = bam_clamp_q4(q.w);
    } else { /* output byte j is source position l - 1 - (p + j): decode [s0, s0 + 16) forwards, complement, reverse the 16 bytes */
        const long long s0 = l - 16 - p;
        bam_codes16(sq, s0, c);
        sb.x = bam_bswap(bam_lookup4(c[3], BAM_REV));
        sb.y = bam_bswap(bam_lookup4(c[2], BAM_REV));
        sb.z = bam_bswap(bam_lookup4(c[1], BAM_REV));
        sb.w = bam_bswap(bam_lookup4(c[0], BAM_REV));
        const u32x4 q = bam_load16(ql + s0);
        qb.x = bam_clamp_q4(bam_bswap(q.w));
        qb.y = bam_clamp_q4(bam_bswap(q.z));
        qb.z = bam_clamp_q4(bam_bswap(q.y));
        qb.w = bam_clamp_q4(bam_bswap(q.x));
    }
}

/* reads r with off[r] <= a, counted in [lo, hi] (off non-decreasing): the read that holds output byte a is the last of them */
__device__ __forceinline__ u32 bam_upper(const uint64_t* __restrict__ off, u32 lo, u32 hi, uint64_t a) {
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (off[mid] <= a) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void bam_merge(u32& dst, u32 v, u32 m) { dst = (dst & ~m) | (v & m); }

/* grid: one lane per 16-byte word of the output in [off[0], off[n]) (word u covers bytes [16 u, 16 u + 16) of seq / qual) */
__global__ void __launch_bounds__(BAM_THREADS)
k_bam_decode(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ off, u32 n_reads,
             u64 word0, u64 n_words, u8* __restrict__ seq, u8* __restrict__ qual) {
    __shared__ u32 s_range[2];
    const u64 wb = word0 + (u64)blockIdx.x * BAM_THREADS; /* the block's first word */
    if (threadIdx.x == 0) { /* the reads the block's words touch: [first, last] */
        const u64 wl = min(wb + BAM_THREADS, word0 + n_words) - 1;
        const u32 f = bam_upper(off, 0, n_reads + 1, 16 * wb);
        const u32 l = bam_upper(off, f ? f - 1 : 0, n_reads + 1, 16 * wl + 15);
        s_range[0] = f ? f - 1 : 0;
        s_range[1] = l;
    }
    __syncthreads();
    const u64 w = wb + threadIdx.x;
    if (w >= word0 + n_words) return;
    const uint64_t a = 16 * w;
    /* the last read that starts at or before the word: a run of empty reads in front of it is passed over by the search */
    u32 r = bam_upper(off, s_range[0], s_range[1], a);
    r = r ? r - 1 : 0;
    u32x4 sb = {0, 0, 0, 0}, qb = {0, 0, 0, 0};
    u32 have = 0; /* bytes of the word written, bit i = byte i */
    for (; r < n_reads;) {
        const uint64_t o0 = off[r], o1 = off[r + 1];
        if (o0 >= a + 16) break;
        if (o1 > a && o1 > o0) {
            u32x4 s, q;
            bam_piece(bam, rec_start[r], (long long)a - (long long)o0, s, q); /* (l_seq = o1 - o0: the caller built off from it) */
            const u32 lo = o0 > a ? (u32)(o0 - a) : 0u, hi = (u32)min<uint64_t>(o1 - a, 16);
            const u32 bits = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
            have |= bits;
            u32 m[4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const u32 b4 = (bits >> (4 * d)) & 0xFu;
                m[d] = ((b4 & 1u) ? 0xFFu : 0u) | ((b4 & 2u) ? 0xFF00u : 0u) | ((b4 & 4u) ? 0xFF0000u : 0u) | ((b4 & 8u) ? 0xFF000000u : 0u);
        }
        bam_merge(sb.x, s.x, m[0]);
        bam_merge(sb.y, s.y, m[1]);
        bam_merge(sb.z, s.z, m[2]);
        bam_merge(sb.w, s.w, m[3]);
        bam_merge(qb.x, q.x, m[0]);
        bam_merge(qb.y, q.y, m[1]);
        bam_merge(qb.z, q.z, m[2]);
        bam_merge(qb.w, q.w, m[3]);
        }
        if (o1 >= a + 16) break;
        /* the next read with a byte in the word: the LAST of the reads that start at o1 -- a run of empty reads there costs one search,
           not one step each (entries from s_range[1] on lie behind the block's last byte, so behind o1) */
        r = bam_upper(off, r + 1, s_range[1], o1) - 1;
    }
    if (have == 0xFFFFu) {
        *(u32x4*)(seq + a) = sb;
        *(u32x4*)(qual + a) = qb;
    } else {
        const u32 sw[4] = {sb.x, sb.y, sb.z, sb.w}, qw[4] = {qb.x, qb.y, qb.z, qb.w};
        for (int i = 0; i < 16; i++)
            if (have & (1u << i)) {
                seq[a + i] = (u8)(sw[i >> 2] >> (8 * (i & 3)));
                qual[a + i] = (u8)(qw[i >> 2] >> (8 * (i & 3)));
            }
    }
}

/* words of the output [off[0], off[n]): the launch's extent */
inline void bam_words(uint64_t o_begin, uint64_t o_end, u64& word0, u64& n_words) {
    word0 = o_begin / 16;
    n_words = o_end > o_begin ? (o_end + 15) / 16 - word0 : 0;
}

}  // namespace fpl
#endif
