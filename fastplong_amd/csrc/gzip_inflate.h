/*
 * gzip_inflate.h -- ONE LONG deflate stream (the payload of an ordinary one-member .gz) inflated ON THE DEVICE, a window of
 * compressed bytes per call (fpl_inflate_gzip, include/fastplong_amd.h).  The two-pass scheme of pugz / rapidgzip on top of the
 * pieces of bgzf_inflate.h (BgzfIn, bgzf_build, bgzf_symbol, the CRC helpers of gz_emit.h):
 *
 *   the window's payload is cut into CHUNKS of chunk_bytes.  Chunk 0 starts at a bit the caller knows to be a block start; where
 *   the blocks start inside the other chunks is guessed, the guess is then PROVEN by the decode of the chunk in front landing on
 *   it, and nothing that is not proven is given out.
 *
 *   k_gzip_find     lane = bit offset.  For every chunk but the first: the first bit offset in it that parses as the header of a
 *                   non-final dynamic-Huffman block (gzip_header_ok: the list of conditions is there).  No such offset: the
 *                   chunk has no candidate and its bytes are decoded by the chunk in front.  Stored and fixed blocks are not
 *                   searched for.
 *   k_gzip_decode   one wave per chunk that has a candidate, from its start bit, block after block, until a block ends at or
 *                   behind the start bit of the next chunk that has a candidate, or with BFINAL, or until it cannot go on.  The
 *                   output is 16-bit ELEMENTS in the chunk's room: a byte value, or 0x8000 | i for "byte i of the 32 KiB in
 *                   front of this chunk" where a match reaches before the chunk's start; a match copies elements, so markers
 *                   propagate.  What counts is what stood at the end of the last COMPLETE block: a chunk that completed one is
 *                   good up to there (status 0, confirmed only when that end is exactly the next candidate), one that completed
 *                   none carries the reason as its status.
 *   k_gzip_windows  one workgroup walks the chain from chunk 0: a chunk is ACCEPTED when it was reached (chunk 0, or the chunk in
 *                   front of it in the chain ended exactly on its start bit) and has status 0 and its bytes fit out_cap.  For
 *                   every accepted chunk: where its bytes go (the running sum of the element counts -- the walk is serial
 *                   anyway) and the 32 KiB window behind it, resolved against the window in front of it.  The walk ends at the
 *                   first chunk that is not accepted, that was not confirmed, or that held the final block.  A FALSE CANDIDATE
 *                   (the chunk in front ran past it) therefore ends the window where the chunk in front ended -- a proven block
 *                   boundary --, and the caller's next call goes on from there: the earlier chunk "runs on" in the next call
 *                   instead of in a second round.
 *   k_gzip_resolve  all accepted chunks in parallel: markers replaced from the window in front, bytes to their final offsets,
 *                   the CRC remainder of the chunk's bytes (every thread a stretch of its own, shifted with gz_mulmod / gz_xpow8).
 *   k_gzip_finish   one thread folds the remainders along the chain into the CRC-32 of the window's bytes and writes the result.
 *
 * k_gzip_decode decodes from positions that may be no block starts: GARBAGE IS ITS NORMAL INPUT.  By construction, as in
 * bgzf_inflate_block: the bit reader (BgzfIn) never loads outside [comp, comp + comp_len) and gives zero bits behind the end; every
 * store is preceded by a comparison with the chunk's room; a marker's index is 32768 + s with -32768 <= s < 0, because a distance
 * is at most 32768 and the output position at least 0; every loop either takes input bits (and ends with refill() behind the
 * end) or is bounded by a length checked against the room.  Running out of room is a status.
 *
 * Unlike k_bgzf_inflate this decoder takes the two incomplete distance codes zlib writes: none at all, and a single 1-bit code.
 */
#ifndef FPL_GZIP_INFLATE_H
#define FPL_GZIP_INFLATE_H

#include "bgzf_inflate.h"

namespace fpl {

constexpr int GZIP_THREADS = 256;      /* find, decode, resolve: four waves */
constexpr int GZIP_WIN_THREADS = 1024; /* the one workgroup of k_gzip_windows */
constexpr u32 GZIP_WINDOW = 32768;
constexpr u32 GZIP_ROOM_FACTOR = 8; /* elements of room per compressed byte of a chunk (a chunk without a candidate lends its room
                                       to the chunk that decodes it) */
constexpr u32 GZIP_ROOM0 = 8u << 20;
constexpr u64 GZIP_NONE = ~0ull;
constexpr u64 GZIP_MAX_COMP = 1ull << 27; /* payload bytes of one call: element counts and room offsets of a chunk stay below 2^31 */
constexpr u32 GZIP_MIN_CHUNK = 64, GZIP_MAX_CHUNK = 1u << 24, GZIP_DEFAULT_CHUNK = 32768;
enum { GZIP_CONFIRMED = 1, GZIP_FINAL = 2, GZIP_ACCEPTED = 4, GZIP_BAD_MARKER = 8 };

struct GzipChunk { /* 48 bytes */
    u64 start_bit; /* find (chunk 0: the caller's): GZIP_NONE = no candidate */
    u64 end_bit;   /* decode: behind the last complete block */
    u64 out_off;   /* windows: where its bytes go */
    u32 count;     /* decode: elements at end_bit */
    u32 status;    /* decode: FPL_GZIP_* when no block was completed */
    u32 flags;
    u32 next;      /* decode: the next chunk with a candidate, n_chunks when there is none */
    u32 prev_slot; /* windows: the slot of the window in front of it */
    u32 crc_raw;   /* resolve: the remainder of its bytes (no initial / final inversion) */
};

struct GzipJob {
    const u8* comp; /* the payload, from the byte that holds the start bit */
    u32 comp_len;
    u32 start_bit; /* 0 .. 7 */
    u32 chunk_bytes, n_chunks;
    u32 room_per_chunk; /* chunk_bytes * GZIP_ROOM_FACTOR elements */
    u32 room0_extra;    /* ... and so many more for chunk 0, whose start is known: one call always gets through one block of up to
                           GZIP_ROOM0 bytes, however well it compressed, so a stream of long runs is taken too, in more calls */
    u32 dict_len;       /* valid bytes at the END of window slot 0 */
    u64 out_cap;
    GzipChunk* chunks; /* n_chunks */
    unsigned short* room; /* room0_extra + n_chunks * room_per_chunk elements: chunk 0 at 0, chunk c at room0_extra + c * room_per_chunk */
    u8* wins;          /* (n_chunks + 1) windows of 32 KiB: slot 0 the caller's, slot c + 1 the one behind chunk c */
    u8* out;
    fpl_gzip_window* res;
};

__device__ __forceinline__ unsigned short* gzip_room(const GzipJob& job, u32 c) {
    return job.room + (c ? (u64)job.room0_extra + (u64)c * job.room_per_chunk : 0ull);
}

/* n <= 32 bits at bit offset `bit` of base[0 .. len); what lies behind the end reads as zero bits (any lane, any offset) */
__device__ __forceinline__ u32 gzip_peek(const u8* base, u32 len, u64 bit, u32 n) {
    const u64 at = bit >> 3;
    u64 v = 0;
    if (at + 8 <= (u64)len) {
        __builtin_memcpy(&v, base + at, 8);
    } else {
        for (u32 k = 0; k < 8; k++)
            if (at + k < (u64)len) v |= (u64)base[at + k] << (8 * k);
    }
    v >>= (u32)(bit & 7u);
    return n >= 32 ? (u32)v : (u32)v & ((1u << n) - 1u);
}

/* Does a non-final dynamic-Huffman block header parse at `bit`?  One lane, registers only.
     BFINAL = 0, BTYPE = 2; HLIT <= 29 and HDIST <= 29; a complete code-length code; the 257 + HLIT + 1 + HDIST lengths decode
     inside the input, no repeat without a previous length, none across the end; symbol 256 has a length; a complete
     literal/length code; a distance code that is complete, or empty, or a single 1-bit code.
   The code-length code is kept packed: 3 bits of length per symbol, its symbols sorted by (length, symbol) at 5 bits each, the
   counts per length at 5 bits each.  Completeness is Kraft's sum: exactly one. */
__device__ inline bool gzip_header_ok(const u8* base, u32 len, u64 bit) {
    const u64 end = 8ull * len;
    const u32 h = gzip_peek(base, len, bit, 17);
    if ((h & 7u) != 4u) return false;
    const u32 hlit = ((h >> 3) & 31u), hdist = (h >> 8) & 31u, hclen = ((h >> 13) & 15u) + 4;
    if (hlit > 29 || hdist > 29) return false;
    u64 p = bit + 17;
    const u64 w = (u64)gzip_peek(base, len, p, 30) | ((u64)gzip_peek(base, len, p + 30, 27) << 30);
    u64 cl = 0;
    u32 kraft = 0;
    for (u32 i = 0; i < hclen; i++) {
        const u32 v = (u32)(w >> (3 * i)) & 7u;
        const u32 pos = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2; /* RFC 1951 3.2.7 */
        cl |= (u64)v << (3 * pos);
        if (v) kraft += 128u >> v;
    }
    if (kraft != 128u) return false;
    p += 3 * hclen;
    u64 s0 = 0, s1 = 0, cnt = 0; /* sorted symbols 0 .. 11 and 12 .. 18; counts of the lengths 0 .. 7 */
    u32 ns = 0;
    for (u32 l = 1; l <= 7; l++) {
        u32 c = 0;
        for (u32 s = 0; s < BGZF_NCL; s++)
            if (((u32)(cl >> (3 * s)) & 7u) == l) {
                if (ns < 12)
                    s0 |= (u64)s << (5 * ns);
                else
                    s1 |= (u64)s << (5 * (ns - 12));
                ns++;
                c++;
            }
        cnt |= (u64)c << (5 * l);
    }
    const u32 nlit = 257 + hlit, total = nlit + 1 + hdist;
    u32 n = 0, prev = 0, kraft_lit = 0, kraft_dist = 0, ndist = 0;
    bool have_prev = false, has256 = false;
    while (n < total) {
        if (p >= end) return false;
        u32 b = gzip_peek(base, len, p, 14);
        u32 code = 0, first = 0, index = 0, sym = 0, used = 0;
        for (u32 l = 1; l <= 7; l++) {
            code |= b & 1u;
            b >>= 1;
            const u32 c = (u32)(cnt >> (5 * l)) & 31u;
            if (code - first < c) {
                const u32 k = index + (code - first);
                sym = k < 12 ? (u32)(s0 >> (5 * k)) & 31u : (u32)(s1 >> (5 * (k - 12))) & 31u;
                used = l;
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (!used) return false; /* (a complete code always matches) */
        u32 rep = 1, val = sym;
        if (sym == 16) {
            if (!have_prev) return false;
            val = prev;
            rep = 3 + (b & 3u);
            used += 2;
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (b & 7u);
            used += 3;
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (b & 127u);
            used += 7;
        }
        p += used;
        if (rep > total - n) return false;
        if (val) {
            for (u32 k = 0; k < rep; k++) {
                if (n + k < nlit) {
                    kraft_lit += 32768u >> val;
                    has256 = has256 || n + k == 256;
                } else {
                    kraft_dist += 32768u >> val;
                    ndist++;
                }
            }
        }
        n += rep;
        prev = val;
        have_prev = true;
    }
    if (p > end || !has256 || kraft_lit != 32768u) return false;
    return kraft_dist == 32768u || ndist == 0 || (ndist == 1 && kraft_dist == 16384u);
}

__global__ void __launch_bounds__(GZIP_THREADS) k_gzip_find(GzipJob job) {
    const u32 lane = (u32)lane_id();
    const u32 wave = blockIdx.x * (GZIP_THREADS / WAVE) + (u32)wave_in_block(), n_waves = gridDim.x * (GZIP_THREADS / WAVE);
    if (wave == 0 && lane == 0) job.chunks[0].start_bit = job.start_bit;
    for (u32 c = 1 + wave; c < job.n_chunks; c += n_waves) { /* wave-uniform */
        const u64 lo = 8ull * c * job.chunk_bytes, hi = min(lo + 8ull * job.chunk_bytes, 8ull * job.comp_len);
        u64 found = GZIP_NONE;
        for (u64 at = lo; at < hi; at += WAVE) {
            const bool ok = at + lane < hi && gzip_header_ok(job.comp, job.comp_len, at + lane);
            const u64 m = wave_ballot(ok);
            if (m) {
                found = at + (u64)(__ffsll(m) - 1);
                break;
            }
        }
        if (lane == 0) job.chunks[c].start_bit = found;
    }
}

/* the distance code of the block in hand (L.lens[hlit .. hlit + hdist)): 0 = tables built, 1 = no code at all, 2 = a single
   1-bit code (its symbol in `single`), 3 = neither complete nor one of the two */
enum { GZIP_DIST_TABLE = 0, GZIP_DIST_NONE = 1, GZIP_DIST_SINGLE = 2, GZIP_DIST_BAD = 3 };
__device__ inline u32 gzip_build_dist(BgzfWaveLds& L, u32 hlit, u32 hdist, u32& single) {
    const u32 lane = (u32)lane_id();
    wave_sync();
    const u32 l = lane < hdist ? L.lens[hlit + lane] : 0u; /* hdist <= 32 */
    const u64 m = wave_ballot(l != 0);
    if (m == 0) return GZIP_DIST_NONE;
    if ((m & (m - 1)) == 0) {
        const u32 s = (u32)(__ffsll(m) - 1);
        if (uniform_u32(L.lens[hlit + s]) == 1) {
            single = s;
            return GZIP_DIST_SINGLE;
        }
    }
    return bgzf_build(L.lens + hlit, hdist, L.dist_tab, BGZF_DIST_BITS, L.dist_sorted, L.dist_cnt, L.code) ? GZIP_DIST_TABLE : GZIP_DIST_BAD;
}

struct GzipEnd { /* where a chunk's decode stood behind its last complete block */
    u64 bits;
    u32 count, blocks, flags;
};

/* One chunk from `start` on; returns why it stopped (0: at its stop bit or the final block), `e` says what is good.
   Wave-uniform but for the lanes' shares of the copies. */
__device__ inline u32 gzip_decode_chunk(const u8* comp, u32 comp_len, u64 start, u64 stop, unsigned short* out, u32 room, BgzfWaveLds& L,
                                        GzipEnd& e) {
    const u32 lane = (u32)lane_id();
    BgzfIn in;
    in.base = comp;
    in.len = comp_len;
    in.seek((u32)(start >> 3));
    e.bits = start, e.count = 0, e.blocks = 0, e.flags = 0;
    if (!in.refill()) return FPL_GZIP_OVERRUN;
    in.drop((u32)(start & 7u));
    u32 op = 0, ordered = 0, qn = 0, lit = 0;
    auto flush = [&]() {
        if (lane < qn) out[op + lane] = (unsigned short)lit; /* op + qn <= room: checked when the literal was taken */
        op += qn;
        qn = 0;
    };
    for (;;) { /* deflate blocks */
        if (!in.refill()) return FPL_GZIP_OVERRUN;
        const u32 last = in.take(1), type = in.take(2);
        if (type == 3) return FPL_GZIP_MALFORMED;
        if (type == 0) {
            in.drop(in.nb & 7u);
            if (!in.refill()) return FPL_GZIP_OVERRUN;
            const u32 len = in.take(16), nlen = in.take(16);
            if ((len ^ 0xFFFFu) != nlen) return FPL_GZIP_MALFORMED;
            const u64 cb = in.consumed_bits();
            if (cb > 8ull * comp_len) return FPL_GZIP_OVERRUN;
            const u32 p = (u32)(cb >> 3);
            if (len > comp_len - p) return FPL_GZIP_OVERRUN;
            if (len > room - op) return FPL_GZIP_ROOM;
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
                if (!in.refill()) return FPL_GZIP_OVERRUN;
                hlit = in.take(5) + 257;
                hdist = in.take(5) + 1;
                const u32 hclen = in.take(4) + 4;
                if (hlit > 286 || hdist > 30) return FPL_GZIP_MALFORMED;
                for (u32 i = 0; i < BGZF_NCL; i++) {
                    u32 v = 0;
                    if (i < hclen) {
                        if (!in.refill()) return FPL_GZIP_OVERRUN;
                        v = in.take(3);
                    }
                    const u32 pos = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 7 - (i - 5) / 2 : 8 + (i - 4) / 2;
                    if (lane == 0) L.cl_lens[pos] = (u8)v;
                }
                if (!bgzf_build(L.cl_lens, BGZF_NCL, L.cl_tab, BGZF_CL_BITS, L.cl_sorted, L.cl_cnt, L.code)) return FPL_GZIP_MALFORMED;
                u32 n = 0, prev = 0;
                bool have_prev = false;
                while (n < hlit + hdist) {
                    if (!in.refill()) return FPL_GZIP_OVERRUN;
                    u32 sym;
                    if (!bgzf_symbol(in, L.cl_tab, BGZF_CL_BITS, L.cl_sorted, L.cl_cnt, BGZF_NCL, sym)) return FPL_GZIP_MALFORMED;
                    if (sym < 16) {
                        if (lane == 0) L.lens[n] = (u8)sym;
                        n++;
                        prev = sym;
                        have_prev = true;
                        continue;
                    }
                    u32 rep, val = 0;
                    if (sym == 16) {
                        if (!have_prev) return FPL_GZIP_MALFORMED;
                        val = prev;
                        rep = 3 + in.take(2);
                    } else if (sym == 17) {
                        rep = 3 + in.take(3);
                    } else {
                        rep = 11 + in.take(7);
                    }
                    if (rep > hlit + hdist - n) return FPL_GZIP_MALFORMED;
                    if (lane == 0)
                        for (u32 k = 0; k < rep; k++) L.lens[n + k] = (u8)val;
                    n += rep;
                    prev = val;
                    have_prev = true;
                }
                wave_sync();
                if (uniform_u32(L.lens[256]) == 0) return FPL_GZIP_MALFORMED; /* no end-of-block code */
            }
            if (!bgzf_build(L.lens, hlit, L.lit_tab, BGZF_LIT_BITS, L.lit_sorted, L.lit_cnt, L.code)) return FPL_GZIP_MALFORMED;
            u32 single = 0;
            const u32 dmode = gzip_build_dist(L, hlit, hdist, single);
            if (dmode == GZIP_DIST_BAD) return FPL_GZIP_MALFORMED;
            for (;;) { /* symbols */
                if (!in.refill()) return FPL_GZIP_OVERRUN;
                u32 sym;
                if (!bgzf_symbol(in, L.lit_tab, BGZF_LIT_BITS, L.lit_sorted, L.lit_cnt, hlit, sym)) return FPL_GZIP_MALFORMED;
                if (sym < 256) {
                    if (op + qn >= room) return FPL_GZIP_ROOM;
                    lit = lane == qn ? sym : lit;
                    if (++qn == WAVE) flush();
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) return FPL_GZIP_MALFORMED;
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
                if (!in.refill()) return FPL_GZIP_OVERRUN;
                u32 ds;
                if (dmode == GZIP_DIST_NONE) return FPL_GZIP_MALFORMED;
                if (dmode == GZIP_DIST_SINGLE) {
                    if (in.take(1)) return FPL_GZIP_MALFORMED; /* the one code is the bit 0 */
                    ds = single;
                } else if (!bgzf_symbol(in, L.dist_tab, BGZF_DIST_BITS, L.dist_sorted, L.dist_cnt, hdist, ds)) {
                    return FPL_GZIP_MALFORMED;
                }
                if (ds > 29) return FPL_GZIP_MALFORMED;
                u32 dist; /* 1 .. 32768 */
                if (ds < 4) {
                    dist = 1 + ds;
                } else {
                    const u32 eb = (ds >> 1) - 1;
                    dist = 1 + ((2 + (ds & 1u)) << eb) + in.take(eb);
                }
                flush();
                if (len > room - op) return FPL_GZIP_ROOM;
                const int src = (int)op - (int)dist; /* >= -32768; op < 2^31 (GZIP_MAX_COMP) */
                if (src + (int)min(len, dist) > (int)ordered) {
                    bgzf_order_stores();
                    ordered = op;
                }
                for (u32 i = lane; i < len; i += WAVE) {
                    const int s = src + (int)(dist >= len ? i : i % dist);
                    out[op + i] = s < 0 ? (unsigned short)(0x8000u | (u32)(32768 + s)) : out[s];
                }
                op += len;
            }
        }
        flush();
        const u64 cb = in.consumed_bits();
        if (cb > 8ull * comp_len) return FPL_GZIP_OVERRUN;
        e.bits = cb, e.count = op, e.blocks++;
        if (last) {
            e.flags = GZIP_FINAL;
            return FPL_GZIP_OK;
        }
        if (cb >= stop) {
            e.flags = cb == stop ? GZIP_CONFIRMED : 0u;
            return FPL_GZIP_OK;
        }
    }
}

__global__ void __launch_bounds__(GZIP_THREADS) k_gzip_decode(GzipJob job) {
    __shared__ BgzfWaveLds lds[GZIP_THREADS / WAVE];
    BgzfWaveLds& L = lds[wave_in_block()];
    const u32 lane = (u32)lane_id();
    const u32 wave = blockIdx.x * (GZIP_THREADS / WAVE) + (u32)wave_in_block(), n_waves = gridDim.x * (GZIP_THREADS / WAVE);
    for (u32 c = wave; c < job.n_chunks; c += n_waves) { /* wave-uniform */
        const u64 start = uniform_u64(job.chunks[c].start_bit);
        if (start == GZIP_NONE) continue;
        u32 next = job.n_chunks;
        for (u32 k0 = c + 1; k0 < job.n_chunks; k0 += WAVE) {
            const u32 k = k0 + lane;
            const u64 m = wave_ballot(k < job.n_chunks && job.chunks[k].start_bit != GZIP_NONE);
            if (m) {
                next = k0 + (u32)(__ffsll(m) - 1);
                break;
            }
        }
        const u64 stop = next < job.n_chunks ? uniform_u64(job.chunks[next].start_bit) : GZIP_NONE;
        GzipEnd e;
        const u32 why = gzip_decode_chunk(job.comp, job.comp_len, start, stop, gzip_room(job, c),
                                          (next - c) * job.room_per_chunk + (c ? 0u : job.room0_extra), L, e);
        if (lane == 0) {
            GzipChunk& ch = job.chunks[c];
            ch.end_bit = e.bits;
            ch.count = e.count;
            ch.status = e.blocks ? (u32)FPL_GZIP_OK : why;
            ch.flags = e.flags;
            ch.next = next;
        }
        wave_sync(); /* (a convergent point between lane 0's stores and the next round: see k_bgzf_inflate) */
    }
}

/* what the whole workgroup stored is where its later loads find it (bgzf_order_stores, for a workgroup) */
__device__ __forceinline__ void gzip_block_sync() {
#ifndef FPL_EMU
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
}

__global__ void __launch_bounds__(GZIP_WIN_THREADS) k_gzip_windows(GzipJob job) {
    __shared__ u32 bad;
    const u32 tid = threadIdx.x;
    u32 cur = 0, prev_slot = 0, n_acc = 0, why = FPL_GZIP_OK;
    u64 off = 0;
    if (tid == 0) bad = 0; /* (set at most once: whoever sees it set leaves the walk, so it is never cleared while someone may still read it) */
    for (;;) { /* block-uniform */
        gzip_block_sync();
        const GzipChunk ch = job.chunks[cur];
        if (ch.status != FPL_GZIP_OK) {
            why = ch.status;
            break;
        }
        if (ch.count > job.out_cap - off) {
            why = FPL_GZIP_ROOM;
            break;
        }
        const u64 valid = min((u64)GZIP_WINDOW, (u64)job.dict_len + off); /* bytes of the window in front that exist */
        const u8* wp = job.wins + (u64)prev_slot * GZIP_WINDOW;
        u8* wn = job.wins + (u64)(cur + 1) * GZIP_WINDOW;
        const unsigned short* el = gzip_room(job, cur);
        for (u32 k = tid; k < GZIP_WINDOW; k += GZIP_WIN_THREADS) {
            const long long p = (long long)ch.count - (long long)GZIP_WINDOW + k; /* the element that becomes byte k; >= -32768 */
            u32 b;
            if (p >= 0) {
                const u32 v = el[p];
                if (v & 0x8000u) {
                    const u32 idx = v & 0x7FFFu;
                    if (idx < GZIP_WINDOW - valid) bad = 1; /* a distance that reaches before the member's first byte */
                    b = wp[idx];
                } else {
                    b = v;
                }
            } else {
                b = wp[GZIP_WINDOW + p];
            }
            wn[k] = (u8)b;
        }
        gzip_block_sync();
        if (bad) {
            why = FPL_GZIP_MALFORMED;
            break;
        }
        if (tid == 0) {
            GzipChunk& g = job.chunks[cur];
            g.out_off = off;
            g.prev_slot = prev_slot;
            g.flags = ch.flags | GZIP_ACCEPTED;
        }
        off += ch.count;
        n_acc++;
        prev_slot = cur + 1;
        if ((ch.flags & GZIP_FINAL) || !(ch.flags & GZIP_CONFIRMED) || ch.next >= job.n_chunks) break;
        cur = ch.next;
    }
    if (tid == 0) job.res->status = n_acc ? (u32)FPL_GZIP_OK : why;
}

__global__ void __launch_bounds__(GZIP_THREADS) k_gzip_resolve(GzipJob job) {
    __shared__ u32 crc_tab[256];
    __shared__ u32 wsum[GZIP_THREADS / WAVE];
    __shared__ u32 bad;
    const u32 tid = threadIdx.x;
    crc_tab[tid] = gz_crc_table_entry(tid);
    for (u32 c = blockIdx.x; c < job.n_chunks; c += gridDim.x) { /* block-uniform */
        __syncthreads();
        const GzipChunk ch = job.chunks[c];
        if (ch.start_bit == GZIP_NONE || !(ch.flags & GZIP_ACCEPTED)) continue;
        if (tid == 0) bad = 0;
        __syncthreads();
        const u32 valid = (u32)min((u64)GZIP_WINDOW, (u64)job.dict_len + ch.out_off);
        const u8* wp = job.wins + (u64)ch.prev_slot * GZIP_WINDOW;
        const unsigned short* el = gzip_room(job, c);
        u8* dst = job.out + ch.out_off;
        const u32 n = ch.count;
        const u32 stretch = ((n + GZIP_THREADS - 1) / GZIP_THREADS + 15) & ~15u; /* < 2^24: tid * stretch stays below 2^32 */
        const u32 a0 = (u32)min((u64)n, (u64)tid * stretch), a1 = (u32)min((u64)n, (u64)(tid + 1) * stretch);
        u32 crc = 0;
        bool mine_bad = false;
        auto one = [&](u32 v) -> u32 {
            if (v & 0x8000u) {
                const u32 idx = v & 0x7FFFu;
                mine_bad = mine_bad || idx < GZIP_WINDOW - valid;
                v = wp[idx];
            }
            crc = crc_tab[(crc ^ v) & 0xFFu] ^ (crc >> 8);
            return v & 0xFFu;
        };
        u32 i = a0;
        for (; i + 4 <= a1; i += 4) {
            unsigned short v[4];
            __builtin_memcpy(v, el + i, 8);
            const u32 w = one(v[0]) | (one(v[1]) << 8) | (one(v[2]) << 16) | (one(v[3]) << 24);
            __builtin_memcpy(dst + i, &w, 4);
        }
        for (; i < a1; i++) dst[i] = (u8)one(el[i]);
        if (mine_bad) bad = 1;
        crc = crc ? gz_mulmod(crc, gz_xpow8((u64)(n - a1))) : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) crc ^= shfl_xor_u32(crc, d);
        if (lane_id() == 0) wsum[wave_in_block()] = crc;
        __syncthreads();
        if (tid == 0) {
            u32 r = 0;
            for (int k = 0; k < GZIP_THREADS / WAVE; k++) r ^= wsum[k];
            job.chunks[c].crc_raw = r;
            if (bad) job.chunks[c].flags = ch.flags | GZIP_BAD_MARKER;
        }
    }
}

/* the chain once more, by one thread: the result of the call */
__global__ void __launch_bounds__(WAVE) k_gzip_finish(GzipJob job) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    fpl_gzip_window r;
    r.status = job.res->status; /* k_gzip_windows: why chunk 0 was not accepted, or 0 */
    r.out_bytes = 0, r.end_bit = job.start_bit, r.crc32 = 0, r.final_block = 0, r.chunks = 0;
    u32 raw = 0, cur = 0;
    while (r.status == FPL_GZIP_OK) {
        const GzipChunk ch = job.chunks[cur];
        if (!(ch.flags & GZIP_ACCEPTED)) break;
        if (ch.flags & GZIP_BAD_MARKER) {
            if (r.chunks == 0) r.status = FPL_GZIP_MALFORMED;
            break;
        }
        raw = (raw ? gz_mulmod(raw, gz_xpow8(ch.count)) : 0u) ^ ch.crc_raw;
        r.out_bytes += ch.count;
        r.end_bit = ch.end_bit;
        r.chunks++;
        if (ch.flags & GZIP_FINAL) {
            r.final_block = 1;
            break;
        }
        if (!(ch.flags & GZIP_CONFIRMED) || ch.next >= job.n_chunks) break;
        cur = ch.next;
    }
    r.crc32 = raw ^ gz_mulmod(0xFFFFFFFFu, gz_xpow8(r.out_bytes)) ^ 0xFFFFFFFFu;
    *job.res = r;
}

#ifdef FPL_EMU
#define GZIP_LAUNCH(kernel, grid, block, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
typedef void* gzip_stream_t;
#else
#define GZIP_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__)
typedef hipStream_t gzip_stream_t;
#endif

/* the five launches of one call, in stream order (chunks, room, wins slot 0 and res->status need no initial value but slot 0) */
inline void gzip_enqueue(const GzipJob& job, u32 n_cu, gzip_stream_t s) {
    const u32 per_block = GZIP_THREADS / WAVE;
    const u32 blocks = (job.n_chunks + per_block - 1) / per_block;
    const u32 resident = std::max<u32>(1, n_cu * 4);
    GZIP_LAUNCH(k_gzip_find, dim3(blocks), dim3(GZIP_THREADS), s, job);
    GZIP_LAUNCH(k_gzip_decode, dim3(blocks), dim3(GZIP_THREADS), s, job);
    GZIP_LAUNCH(k_gzip_windows, dim3(1), dim3(GZIP_WIN_THREADS), s, job);
    GZIP_LAUNCH(k_gzip_resolve, dim3(std::min<u32>(job.n_chunks, resident * 4)), dim3(GZIP_THREADS), s, job);
    GZIP_LAUNCH(k_gzip_finish, dim3(1), dim3(WAVE), s, job);
}

/* the arguments fpl_inflate_gzip refuses before anything runs; fills the sizes of `job` */
inline bool gzip_plan(GzipJob& job, uint64_t comp_bytes, uint64_t start_bit, uint32_t dict_len, uint64_t out_cap, uint32_t chunk_bytes) {
    if (chunk_bytes == 0) chunk_bytes = GZIP_DEFAULT_CHUNK;
    if (chunk_bytes < GZIP_MIN_CHUNK || chunk_bytes > GZIP_MAX_CHUNK || dict_len > GZIP_WINDOW) return false;
    if (comp_bytes == 0 || start_bit >= 8ull * comp_bytes) return false;
    const uint64_t len = comp_bytes - (start_bit >> 3);
    if (len > GZIP_MAX_COMP) return false;
    job.comp_len = (u32)len;
    job.start_bit = (u32)(start_bit & 7u);
    job.chunk_bytes = chunk_bytes;
    job.n_chunks = (u32)((len + chunk_bytes - 1) / chunk_bytes);
    job.room_per_chunk = chunk_bytes * GZIP_ROOM_FACTOR;
    job.room0_extra = (u32)std::min<uint64_t>(out_cap, GZIP_ROOM0);
    job.dict_len = dict_len;
    job.out_cap = out_cap;
    return true;
}

}  // namespace fpl
#endif
