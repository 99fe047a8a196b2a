/*
 * bgzf_inflate.h -- the BGZF blocks of a BAM inflated ON THE DEVICE (fpl_inflate_bgzf, include/fastplong_amd.h).
 *
 * A BGZF block is an independent raw deflate stream (RFC 1951) of at most 64 KiB of output whose trailer says how many bytes it
 * makes and what their CRC-32 is; the host finds the blocks from their headers and hands over descriptors (fpl_bgzf_block).
 *
 *   k_bgzf_inflate   ONE WAVE PER BLOCK, blocks taken off a work counter.  Decoding the symbols of one stream is serial, so that
 *                    part is wave-uniform: the bit buffer, the input position and every table lookup are the same in all lanes
 *                    (uniform_u32 keeps them in scalar registers), and the lanes are used for what is parallel --
 *                      input:   a window of 512 bytes, 8 per lane in a register; the decoder takes its next 32 bits with a
 *                               v_readlane at a uniform index.  Reads stay inside [comp_off, comp_off + comp_len): a lane whose
 *                               8 bytes cross the end loads byte by byte, and what lies behind the end reads as zero bits.
 *                      tables:  code lengths -> canonical codes -> a direct table over the low bits of the bit buffer (10 for
 *                               literal/length, 8 for distance, 7 for the code-length code); a longer code takes the bit-serial
 *                               canonical walk over count[] and the sorted symbols.
 *                      literals: up to 64 gathered one per lane in a register, stored as one coalesced run.
 *                      matches / stored blocks: lane i copies byte i, i + 64, ...; for dist < len the source is
 *                               start - dist + (i % dist).
 *                      CRC-32:  every lane takes a stretch of the output, the remainders are shifted (gz_mulmod / gz_xpow8 of
 *                               gz_emit.h) and folded with a butterfly.
 *                    The output goes straight to global memory and a match reads it back from there.  Stores and loads of ONE
 *                    wave to the same bytes come from different lanes, so the wave orders them itself: before a match whose
 *                    source reaches into bytes stored since the last wait, bgzf_order_stores() waits for the outstanding stores
 *                    (docs/kernels.md "k_bgzf_inflate").  LDS holds the tables only: BGZF_LDS_PER_WAVE bytes a wave.
 *
 * The kernel refuses rather than guesses: status 0 is given only to a stream it decoded completely, with the size and the CRC of
 * the trailer; whatever it does not vouch for the host inflates again (host/bam.cpp), and the host's verdict is the verdict.  It
 * is stricter than zlib in one place: EVERY incomplete code-length set is refused, the single 1-bit distance code included.
 */
#ifndef FPL_BGZF_INFLATE_H
#define FPL_BGZF_INFLATE_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"
#include "gz_emit.h"

namespace fpl {

constexpr int BGZF_THREADS = 256; /* four waves, each with a block of its own */
constexpr u32 BGZF_MAX_ISIZE = 65536;
constexpr u32 BGZF_MAX_COMP = 1u << 24; /* payload bytes of one block the library lets through (a BGZF block has < 64 KiB) */
constexpr u32 BGZF_LIT_BITS = 10, BGZF_DIST_BITS = 8, BGZF_CL_BITS = 7;
constexpr u32 BGZF_NLIT = 288, BGZF_NDIST = 32, BGZF_NCL = 19;

/* one code: the direct table (entry: symbol << 4 | code length; 0: a code longer than the table's bits), and for the
   canonical walk the symbols sorted by (length, symbol) and how many there are of each length */
struct BgzfWaveLds {
    u16 lit_tab[1u << BGZF_LIT_BITS];
    u16 dist_tab[1u << BGZF_DIST_BITS];
    u16 cl_tab[1u << BGZF_CL_BITS];
    u16 lit_sorted[BGZF_NLIT], dist_sorted[BGZF_NDIST], cl_sorted[BGZF_NCL + 1];
    u16 lit_cnt[16], dist_cnt[16], cl_cnt[16];
    u16 code[BGZF_NLIT]; /* scratch of a build: the canonical code of every symbol */
    u8 lens[BGZF_NLIT + BGZF_NDIST]; /* the code lengths of the block in hand: HLIT of them, then HDIST */
    u8 cl_lens[BGZF_NCL + 1];
};
constexpr u32 BGZF_LDS_PER_WAVE = (u32)sizeof(BgzfWaveLds);

/* Stores this wave has issued become visible to loads of its other lanes.  Device: an explicit s_waitcnt vmcnt(0) -- on gfx9
   stores count in vmcnt like loads, and the count falls when the write has been acknowledged, so behind the wait every byte the
   wave stored is where its later loads (through the same CU's vector cache, which is write-through) find it.  A release fence at
   workgroup scope does NOT give this wait (LLVM emits none below agent scope when workgroups are not split over CUs), which is
   why it is written out; the asm's memory clobber and the wave barrier keep the compiler from moving any lane's memory
   operation across it.  Emulator: the lanes meet. */
__device__ __forceinline__ void bgzf_order_stores() {
#ifdef FPL_EMU
    emu_wave_barrier();
#else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#endif
}

/* the compressed bytes of one block, as a stream of bits (all members wave-uniform but the window) */
struct BgzfIn {
    const u8* base; /* comp + comp_off */
    u32 len;        /* comp_len */
    u32 wpos;       /* byte offset of the window */
    u32 wi;         /* next 32-bit word of the window, 0 .. 128 */
    u64 bits;
    u32 nb;
    WaveVals64 win;

    __device__ __forceinline__ void load_window() {
        const u32 at = wpos + 8u * (u32)lane_id();
        u64 v = 0;
        if (at < len) {
            if (len - at >= 8) {
                __builtin_memcpy(&v, base + at, 8);
            } else {
                for (u32 k = 0; k < len - at; k++) v |= (u64)base[at + k] << (8 * k);
            }
        }
        win = wave_publish(v);
    }
    __device__ __forceinline__ void seek(u32 pos) {
        wpos = pos;
        wi = 0;
        bits = 0;
        nb = 0;
        load_window();
    }
    /* at least 32 bits in the buffer.  false: everything in it lies behind the end of the input already (overrun) */
    __device__ __forceinline__ bool refill() {
        if (nb >= 32) return true;
        if (wi == 128) {
            wpos += 512;
            wi = 0;
            load_window();
        }
        if (wpos + 4 * wi >= len + 8) return false;
        const u64 q = win.get((int)(wi >> 1));
        const u32 w = (wi & 1u) ? (u32)(q >> 32) : (u32)q;
        wi++;
        bits |= (u64)w << nb;
        nb += 32;
        return true;
    }
    __device__ __forceinline__ u32 peek(u32 n) const { return (u32)bits & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(u32 n) {
        bits >>= n;
        nb -= n;
    }
    __device__ __forceinline__ u32 take(u32 n) {
        const u32 v = peek(n);
        drop(n);
        return v;
    }
    __device__ __forceinline__ u64 consumed_bits() const { return 8ull * ((u64)wpos + 4ull * wi) - nb; }
};

/* Code lengths -> tables.  Every lane calls (wave-uniform control flow); returns false for an over-subscribed or an incomplete
   set (no code at all is incomplete too).  lens[0 .. n): 0 .. 15, n <= BGZF_NLIT. */
__device__ inline bool bgzf_build(const u8* lens, u32 n, u16* tab, u32 tab_bits, u16* sorted, u16* cnt, u16* code) {
    const u32 lane = (u32)lane_id();
    wave_sync();
    if (lane < 16) { /* lane L counts the symbols of length L */
        u32 c = 0;
        for (u32 s = 0; s < n; s++) c += lens[s] == lane ? 1u : 0u;
        cnt[lane] = (u16)c;
    }
    for (u32 i = lane; i < (1u << tab_bits); i += WAVE) tab[i] = 0;
    wave_sync();
    int left = 1;
    for (u32 l = 1; l <= 15; l++) {
        left = 2 * left - (int)uniform_u32(cnt[l]);
        if (left < 0) return false; /* over-subscribed */
    }
    if (left != 0) return false; /* incomplete */
    if (lane >= 1 && lane < 16) { /* lane L hands out the codes of length L, in symbol order */
        u32 first = 0, at = 0;
        for (u32 l = 1; l < lane; l++) {
            first = (first + cnt[l]) << 1;
            at += cnt[l];
        }
        for (u32 s = 0; s < n; s++)
            if (lens[s] == lane) {
                code[s] = (u16)first++;
                sorted[at++] = (u16)s; /* at < n: the lengths 1 .. 15 count at most n symbols */
            }
    }
    wave_sync();
    const u32 mask = (1u << tab_bits) - 1u;
    for (u32 s = lane; s < n; s += WAVE) {
        const u32 l = lens[s];
        if (l == 0 || l > tab_bits) continue;
        const u32 r = brev32((u32)code[s]) >> (32 - l); /* the code as the bit buffer shows it: first bit lowest */
        for (u32 k = r; k <= mask; k += 1u << l) tab[k & mask] = (u16)((s << 4) | l);
    }
    wave_sync();
    return true;
}

/* one symbol off the bit buffer (>= 15 bits in it, or zero bits behind the end).  false: no code matched (cannot happen with a
   complete code; kept as a bound on the walk) */
__device__ __forceinline__ bool bgzf_symbol(BgzfIn& in, const u16* tab, u32 tab_bits, const u16* sorted, const u16* cnt, u32 n, u32& sym) {
    const u32 e = uniform_u32(tab[in.peek(tab_bits)]);
    if (e & 15u) {
        in.drop(e & 15u);
        sym = e >> 4;
        return true;
    }
    u32 code = 0, first = 0, index = 0;
    u32 b = (u32)in.bits;
    for (u32 l = 1; l <= 15; l++) {
        code |= b & 1u;
        b >>= 1;
        const u32 c = uniform_u32(cnt[l]);
        if (code - first < c) {
            const u32 k = index + (code - first);
            if (k >= n) return false;
            sym = uniform_u32(sorted[k]);
            in.drop(l);
            return true;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return false;
}

/* the stretches' remainders -> the CRC-32 of out[0 .. n) (every lane calls; the stores are ordered by the caller) */
__device__ inline u32 bgzf_crc(const u8* out, u32 n, const u32* crc_tab) {
    const u32 lane = (u32)lane_id();
    const u32 stretch = ((n + 63) / 64 + 15) & ~15u;
    const u32 a0 = min(n, lane * stretch), a1 = min(n, (lane + 1) * stretch);
    u32 c = 0;
    u32 i = a0;
    for (; i + 16 <= a1; i += 16) {
        u32x4 v;
        __builtin_memcpy(&v, out + i, 16);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c ^= w[k];
#pragma unroll
            for (int j = 0; j < 4; j++) c = crc_tab[c & 0xFFu] ^ (c >> 8);
        }
    }
    for (; i < a1; i++) c = crc_tab[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
    c = c ? gz_mulmod(c, gz_xpow8((u64)(n - a1))) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) c ^= shfl_xor_u32(c, d);
    return c ^ gz_mulmod(0xFFFFFFFFu, gz_xpow8(n)) ^ 0xFFFFFFFFu;
}

/* the whole of one block; returns its status.  Wave-uniform but for the lanes' shares of the copies. */
__device__ inline u32 bgzf_inflate_block(const u8* comp, u32 comp_len, u8* out, u32 isize, u32 want_crc, BgzfWaveLds& L, const u32* crc_tab) {
    const u32 lane = (u32)lane_id();
    BgzfIn in;
    in.base = comp;
    in.len = comp_len;
    in.seek(0);
    u32 op = 0;       /* bytes of output made */
    u32 ordered = 0;  /* out[0 .. ordered) was stored before the last bgzf_order_stores() */
    u32 qn = 0;       /* literals gathered, lane k holds the k-th */
    u32 lit = 0;
    auto flush = [&]() {
        if (lane < qn) out[op + lane] = (u8)lit; /* op + qn <= isize: checked when the literal was taken */
        op += qn;
        qn = 0;
    };
    for (;;) { /* deflate blocks */
        if (!in.refill()) return FPL_BGZF_OVERRUN;
        const u32 last = in.take(1), type = in.take(2);
        if (type == 3) return FPL_BGZF_MALFORMED;
        if (type == 0) {
            flush();
            in.drop(in.nb & 7u);
            if (!in.refill()) return FPL_BGZF_OVERRUN;
            const u32 len = in.take(16), nlen = in.take(16);
            if ((len ^ 0xFFFFu) != nlen) return FPL_BGZF_MALFORMED;
            const u64 cb = in.consumed_bits();
            if (cb > 8ull * comp_len) return FPL_BGZF_OVERRUN;
            const u32 p = (u32)(cb >> 3);
            if (len > comp_len - p) return FPL_BGZF_OVERRUN;
            if (len > isize - op) return FPL_BGZF_SIZE;
            for (u32 i = lane; i < len; i += WAVE) out[op + i] = comp[p + i];
            op += len;
            in.seek(p + len);
        } else {
            u32 hlit = BGZF_NLIT, hdist = BGZF_NDIST;
            wave_sync(); /* (no lane still reads the tables of the block before) */
            if (type == 1) {
                for (u32 s = lane; s < BGZF_NLIT + BGZF_NDIST; s += WAVE)
                    L.lens[s] = (u8)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
            } else {
                if (!in.refill()) return FPL_BGZF_OVERRUN;
                hlit = in.take(5) + 257;
                hdist = in.take(5) + 1;
                const u32 hclen = in.take(4) + 4;
                if (hlit > 286 || hdist > 30) return FPL_BGZF_MALFORMED;
                for (u32 i = 0; i < BGZF_NCL; i++) {
                    u32 v = 0;
                    if (i < hclen) {
                        if (!in.refill()) return FPL_BGZF_OVERRUN;
                        v = in.take(3);
                    }
                    /* the order of RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15 */
                    const u32 pos = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;
                    if (lane == 0) L.cl_lens[pos] = (u8)v;
                }
                if (!bgzf_build(L.cl_lens, BGZF_NCL, L.cl_tab, BGZF_CL_BITS, L.cl_sorted, L.cl_cnt, L.code)) return FPL_BGZF_MALFORMED;
                u32 n = 0, prev = 0;
                bool have_prev = false;
                while (n < hlit + hdist) {
                    if (!in.refill()) return FPL_BGZF_OVERRUN;
                    u32 sym;
                    if (!bgzf_symbol(in, L.cl_tab, BGZF_CL_BITS, L.cl_sorted, L.cl_cnt, BGZF_NCL, sym)) return FPL_BGZF_MALFORMED;
                    if (sym < 16) {
                        if (lane == 0) L.lens[n] = (u8)sym;
                        n++;
                        prev = sym;
                        have_prev = true;
                        continue;
                    }
                    u32 rep, val = 0;
                    if (sym == 16) {
                        if (!have_prev) return FPL_BGZF_MALFORMED;
                        val = prev;
                        rep = 3 + in.take(2);
                    } else if (sym == 17) {
                        rep = 3 + in.take(3);
                    } else {
                        rep = 11 + in.take(7);
                    }
                    if (rep > hlit + hdist - n) return FPL_BGZF_MALFORMED;
                    if (lane == 0)
                        for (u32 k = 0; k < rep; k++) L.lens[n + k] = (u8)val;
                    n += rep;
                    prev = val;
                    have_prev = true;
                }
                wave_sync();
                if (L.lens[256] == 0) return FPL_BGZF_MALFORMED; /* no end-of-block code */
            }
            if (!bgzf_build(L.lens, hlit, L.lit_tab, BGZF_LIT_BITS, L.lit_sorted, L.lit_cnt, L.code)) return FPL_BGZF_MALFORMED;
            if (!bgzf_build(L.lens + hlit, hdist, L.dist_tab, BGZF_DIST_BITS, L.dist_sorted, L.dist_cnt, L.code)) return FPL_BGZF_MALFORMED;
            for (;;) { /* symbols */
                if (!in.refill()) return FPL_BGZF_OVERRUN;
                u32 sym;
                if (!bgzf_symbol(in, L.lit_tab, BGZF_LIT_BITS, L.lit_sorted, L.lit_cnt, hlit, sym)) return FPL_BGZF_MALFORMED;
                if (sym < 256) {
                    if (op + qn >= isize) return FPL_BGZF_SIZE;
                    lit = lane == qn ? sym : lit;
                    if (++qn == WAVE) flush();
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) return FPL_BGZF_MALFORMED;
                const u32 k = sym - 257;
                u32 len;
                if (k < 8) {
                    len = 3 + k;
                } else if (k == 28) {
                    len = 258;
                } else {
                    const u32 eb = (k >> 2) - 1;
                    len = 3 + ((4 + (k & 3u)) << eb) + in.take(eb);
                }
                if (!in.refill()) return FPL_BGZF_OVERRUN;
                u32 ds;
                if (!bgzf_symbol(in, L.dist_tab, BGZF_DIST_BITS, L.dist_sorted, L.dist_cnt, hdist, ds)) return FPL_BGZF_MALFORMED;
                if (ds > 29) return FPL_BGZF_MALFORMED;
                u32 dist;
                if (ds < 4) {
                    dist = 1 + ds;
                } else {
                    const u32 eb = (ds >> 1) - 1;
                    dist = 1 + ((2 + (ds & 1u)) << eb) + in.take(eb);
                }
                flush();
                if (dist > op) return FPL_BGZF_MALFORMED; /* reaches before the block's output */
                if (len > isize - op) return FPL_BGZF_SIZE;
                const u32 src = op - dist;
                if (src + min(len, dist) > ordered) {
                    bgzf_order_stores();
                    ordered = op;
                }
                if (dist >= len) {
                    for (u32 i = lane; i < len; i += WAVE) out[op + i] = out[src + i];
                } else {
                    for (u32 i = lane; i < len; i += WAVE) out[op + i] = out[src + i % dist];
                }
                op += len;
            }
        }
        if (last) break;
    }
    flush();
    if (in.consumed_bits() > 8ull * comp_len) return FPL_BGZF_OVERRUN;
    if (op != isize) return FPL_BGZF_SIZE;
    bgzf_order_stores();
    return bgzf_crc(out, isize, crc_tab) == want_crc ? FPL_BGZF_OK : FPL_BGZF_CRC;
}

/* blocks[0 .. n_blocks): ranges checked by the caller (fpl_inflate_bgzf); *next: the work counter, zero at the launch */
__global__ void __launch_bounds__(BGZF_THREADS) k_bgzf_inflate(const u8* comp, fpl_bgzf_block* blocks, u32 n_blocks, u8* out, u32* next) {
    __shared__ u32 crc_tab[256];
    __shared__ BgzfWaveLds lds[BGZF_THREADS / WAVE];
    crc_tab[threadIdx.x] = gz_crc_table_entry(threadIdx.x);
    __syncthreads();
    BgzfWaveLds& L = lds[wave_in_block()];
    for (;;) {
        u32 b = 0;
        if (lane_id() == 0) b = atomicAdd(next, 1u);
        b = uniform_u32(shfl_u32(b, 0));
        if (b >= n_blocks) break;
        const fpl_bgzf_block d = blocks[b];
        const u32 st = bgzf_inflate_block(comp + uniform_u64(d.comp_off), uniform_u32(d.comp_len), out + uniform_u64(d.out_off), uniform_u32(d.isize), uniform_u32(d.crc32), L, crc_tab);
        if (lane_id() == 0) blocks[b].status = st;
        /* Invariant: a convergent operation stands between lane 0's status store and lane 0's next atomicAdd.  The two branches
           have the same condition; with nothing convergent between them the compiler may join them into a path of lane 0's own,
           and the broadcast of the counter's value would then run without the lane that holds it. */
        wave_sync();
    }
}

}  // namespace fpl
#endif
