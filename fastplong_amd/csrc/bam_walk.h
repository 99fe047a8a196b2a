/*
 * bam_walk.h -- the record walk of a BAM ON THE DEVICE (fpl_process_bgzf_bam_async, include/fastplong_amd.h): the inflated bytes
 * of a submission stay where k_bgzf_inflate put them, and what the host's walk (host/bam.cpp, BamReader::walk) would have
 * uploaded -- where every record starts, the CSR offsets, the names -- is made here.
 *
 * A record says where the next one starts (block_size), so the walk is a linked list.  It is taken in the guess-and-prove shape
 * gzip_inflate.h uses for deflate blocks: the buffer is cut into segments of seg_bytes, every segment guesses where a record
 * starts in it and walks from there on a wave of its own, and one serial pass then goes through the segments with the TRUE
 * position and keeps a segment's walk only where its guess was that position.  Nothing a guess produced is given out unless the
 * chain proved it.
 *
 * The buffer of a slot is [room for the tail | the inflated bytes of this submission]: the inflated part starts at the fixed
 * offset tail_cap, the tail of the submission before (the bytes behind its last whole record) is placed so that it ends there.
 * Positions are byte offsets into that buffer; lo = tail_cap - tail_len is known on the device only, hi = tail_cap + total.
 * Segment s is [s * seg_bytes, (s + 1) * seg_bytes) of the buffer, cut at hi; segments in front of lo hold nothing.
 *
 *   k_bam_place_tail  the context's tail, right-aligned in front of the inflated bytes.
 *   k_bam_find        a wave per segment, lanes as byte positions: the first position that passes bam_find_ok, a cheap filter
 *                     that need not be exact.  The segment that holds the entry (lo, or lo + skip) needs no guess.
 *   k_bam_walk_seg    a wave per segment with a candidate: walks from it to the first record start at or behind the segment's
 *                     end (bam_walk_range; wave-uniform, the lanes share the search for a name's NUL).
 *   k_bam_chain       ONE wave, the only serial part: 64 segments' candidates and exits in registers at a time, the entry
 *                     handed along with v_readlane; a segment whose guess was wrong is walked again from the entry.  Then the
 *                     exclusive sums over the accepted segments, the verdict, the header and the context's new state.
 *   k_bam_compact     a wave per accepted segment: dense record starts, 64-bit CSR offsets, name offsets and names ('@' + the
 *                     name up to its NUL, as the host's walk builds them); all blocks together save the new tail.
 *
 * The rules of a record are csrc/bam_rules.h, the host's own.  The device does not word errors: a failing record gives status
 * RECORD with its index and position and the whole submission is refused; a refused submission counts nothing, leaves the tail as
 * it was and sets BamWalkState::refused, which every walk queued behind it reads (status CHAIN).
 *
 * Bounds hold by construction, whatever the bytes: a record is read only after avail (= hi - p) was compared with what is read;
 * every walk starts at or behind lo; a segment's list takes at most per_seg = seg_bytes / 36 + 1 starts (a step advances 36 bytes
 * at least, and only starts inside the segment are listed), and the loop ends with the segment; the dense arrays are written
 * below rec_cap, the names below names_cap, the tail below tail_cap.
 */
#ifndef FPL_BAM_WALK_H
#define FPL_BAM_WALK_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"
#include "bam_rules.h"

#include <algorithm>

namespace fpl {

constexpr int BAMW_THREADS = 256;             /* four waves, each with a segment of its own */
constexpr u32 BAMW_DEFAULT_SEG = 64u << 10;
constexpr u32 BAMW_MIN_SEG = 64;
constexpr u32 BAMW_FIND_MAX_BS = 1u << 28;    /* k_bam_find only: a larger block_size is no candidate (the chain still takes it) */
constexpr u64 BAMW_NO_CAND = ~0ull;

enum { BAMW_TAKE = 0, BAMW_SKIP = 1, BAMW_NEED = 2, BAMW_BAD = 3, BAMW_FULL = 4 }; /* (0: also "walked to the segment's end") */

/* the context's walk state, in device memory: carried from submission to submission by the order of the parse stream */
struct BamWalkState {
    u32 tail_len; /* bytes in the tail buffer */
    u32 refused;  /* a submission was refused: the walks behind it refuse too */
    u64 rec_base; /* records seen (skipped ones counted) by the accepted submissions of this file */
    u64 tail_src; /* k_bam_chain -> k_bam_compact: where in the slot's buffer the new tail starts */
};

/* what the walk of one segment found */
struct BamSeg {
    u64 exit;      /* the first record start at or behind the segment's end, or where the walk stopped */
    u64 sum_lseq;
    u32 taken, skipped, max_lseq, name_bytes;
    u32 status;    /* 0, BAMW_NEED (an incomplete record at the buffer's end), BAMW_BAD, BAMW_FULL */
    u32 bad_idx;   /* BAMW_BAD: records of the segment in front of the failing one */
};

/* where an accepted segment's records go in the dense arrays */
struct BamSegBase {
    u64 off, name;
    u32 rec, taken; /* taken 0: the segment gives nothing */
};

struct BamWalkJob {
    u8* buf;
    u64 tail_cap, total, skip;
    u32 seg_bytes, n_seg, per_seg, rec_cap;
    BamWalkState* st;
    u8* tail_buf; /* tail_cap bytes */
    const fpl_bgzf_block* blocks;
    u32 n_blocks;
    u64* cand;         /* n_seg */
    BamSeg* segs;      /* n_seg */
    u32* lists;        /* n_seg * per_seg: record starts relative to the segment's start */
    BamSegBase* bases; /* n_seg */
    fpl_bam_window* hdr;
    uint64_t *rec_start, *off, *name_off; /* rec_cap (+ 1) */
    u8* names;
    u64 names_cap;
};

__device__ __forceinline__ u64 bamw_shfl_up_u64(u64 v, unsigned d) {
    const u32 lo = shfl_up_u32((u32)v, d), hi = shfl_up_u32((u32)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}
/* inclusive prefix sum across lanes, 64 bits (all lanes call) */
__device__ inline u64 bamw_scan_incl_u64(u64 v) {
    const unsigned l = (unsigned)lane_id();
    for (unsigned d = 1; d < 64; d <<= 1) {
        const u64 o = bamw_shfl_up_u64(v, d);
        if (l >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ bamrule::Fields bamw_uniform(const bamrule::Fields& f) {
    bamrule::Fields g;
    g.bs = uniform_u32(f.bs);
    g.l_name = uniform_u32(f.l_name);
    g.n_cigar = uniform_u32(f.n_cigar);
    g.flag = uniform_u32(f.flag);
    g.l_seq = uniform_u32(f.l_seq);
    return g;
}

/* the record at p (< = hi; wave-uniform): the checks of BamReader::walk in its order */
__device__ inline u32 bam_walk_one(const u8* buf, u64 p, u64 hi, bamrule::Fields& f) {
    const u64 avail = hi - p;
    if (avail < 4) return BAMW_NEED;
    const u32 bs = uniform_u32(bamrule::rd32(buf + p));
    if (!bamrule::block_size_ok(bs)) return BAMW_BAD;
    if (avail < bamrule::HEAD) return BAMW_NEED;
    f = bamw_uniform(bamrule::fields(buf + p));
    if (!bamrule::fields_ok(f)) return BAMW_BAD;
    if (avail < 4 + (u64)f.bs) return BAMW_NEED;
    if (bamrule::skipped(f.flag)) return BAMW_SKIP;
    if (bamrule::paired(f.flag)) return BAMW_BAD;
    /* (the first quality byte lies inside the record: fixed_len <= block_size, and l_seq > 0) */
    if (f.l_seq > 0 && bamrule::no_qualities(f, (u8)uniform_u32(buf[p + bamrule::qual_offset(f)]))) return BAMW_BAD;
    return BAMW_TAKE;
}

/* strnlen(name, l_name - 1), the lanes looking at 64 bytes at a time (all lanes call; l_name >= 1, the bytes lie in the record) */
__device__ inline u32 bam_name_len(const u8* name, u32 l_name) {
    const u32 n = l_name - 1, lane = (u32)lane_id();
    for (u32 k = 0; k < n; k += WAVE) {
        const u32 i = k + lane;
        const u64 m = wave_ballot(i < n && name[i] == 0);
        if (m) return k + (u32)__ffsll((unsigned long long)m) - 1;
    }
    return n;
}
/* the same, one lane on its own (k_bam_compact: a record per lane) */
__device__ inline u32 bam_name_len_lane(const u8* name, u32 l_name) {
    u32 i = 0;
    while (i + 1 < l_name && name[i]) i++;
    return i;
}

/* from `from` (in [a, b), >= lo) to the first record start at or behind b, the segment's end; list: the starts of the records
   taken, relative to a, at most cap.  Wave-uniform; lane 0 writes. */
__device__ inline BamSeg bam_walk_range(const u8* buf, u64 from, u64 a, u64 b, u64 hi, u32* list, u32 cap) {
    BamSeg o;
    o.exit = from;
    o.sum_lseq = 0;
    o.taken = o.skipped = o.max_lseq = o.name_bytes = o.status = o.bad_idx = 0;
    u64 p = from;
    while (p < b) { /* (bounded: a step is 36 bytes at least) */
        bamrule::Fields f;
        const u32 r = bam_walk_one(buf, p, hi, f);
        if (r == BAMW_NEED || r == BAMW_BAD) {
            o.status = r;
            o.bad_idx = o.taken + o.skipped;
            break;
        }
        if (r == BAMW_TAKE) {
            if (o.taken >= cap) { /* (cannot be: cap starts of 36 bytes do not fit a segment) */
                o.status = BAMW_FULL;
                break;
            }
            const u32 nl = bam_name_len(buf + p + bamrule::HEAD, f.l_name);
            if (lane_id() == 0) list[o.taken] = (u32)(p - a);
            o.taken++;
            o.sum_lseq += f.l_seq;
            o.max_lseq = max(o.max_lseq, f.l_seq);
            o.name_bytes += 1 + nl;
        } else {
            o.skipped++;
        }
        p += 4 + (u64)f.bs;
    }
    o.exit = p;
    return o;
}

/* could a WHOLE record start at p (lo <= p < hi)?  The record must lie inside the buffer; of the record behind it what can be seen
   is checked, and what cannot is left to the chain. */
__device__ inline bool bam_find_ok(const u8* buf, u64 p, u64 hi) {
    const u64 avail = hi - p;
    if (avail < bamrule::HEAD) return false;
    const u32 bs = bamrule::rd32(buf + p);
    if (bs < bamrule::MIN_BLOCK_SIZE || bs > BAMW_FIND_MAX_BS) return false;
    if (avail < 4 + (u64)bs) return false; /* (an incomplete record is the chain's to find: it ends the chain, nothing is walked) */
    const bamrule::Fields f = bamrule::fields(buf + p);
    if (f.l_name < 1 || f.l_seq > 0x7FFFFFFFu || bamrule::fixed_len(f) > (u64)bs) return false;
    if (buf[p + bamrule::HEAD + f.l_name - 1] != 0) return false; /* (inside the record: fixed_len <= block_size) */
    const u64 q = p + 4 + (u64)bs;
    if (q < hi && hi - q >= bamrule::HEAD) {
        const bamrule::Fields g = bamrule::fields(buf + q);
        if (g.bs < bamrule::MIN_BLOCK_SIZE || g.bs > BAMW_FIND_MAX_BS || g.l_name < 1 || g.l_seq > 0x7FFFFFFFu ||
            bamrule::fixed_len(g) > (u64)g.bs)
            return false;
    }
    return true;
}

__device__ __forceinline__ u32 bamw_tail_len(const BamWalkJob& j) { return (u32)min((u64)j.st->tail_len, j.tail_cap); }

__global__ void __launch_bounds__(BAMW_THREADS) k_bam_place_tail(BamWalkJob j) {
    if (j.st->refused) return;
    const u32 tl = bamw_tail_len(j);
    u8* dst = j.buf + (j.tail_cap - tl);
    for (u64 i = (u64)blockIdx.x * BAMW_THREADS + threadIdx.x; i < tl; i += (u64)gridDim.x * BAMW_THREADS) dst[i] = j.tail_buf[i];
}

__global__ void __launch_bounds__(BAMW_THREADS) k_bam_find(BamWalkJob j) {
    const u32 s = blockIdx.x * (BAMW_THREADS / WAVE) + (u32)wave_in_block();
    if (s >= j.n_seg) return;
    const u64 hi = j.tail_cap + j.total;
    const u64 entry = min(j.tail_cap - bamw_tail_len(j) + j.skip, hi);
    const u64 a = (u64)s * j.seg_bytes, b = min(a + j.seg_bytes, hi);
    u64 c = BAMW_NO_CAND;
    if (entry < b) {
        if (entry >= a) {
            c = entry;
        } else {
            for (u64 p0 = a; p0 < b; p0 += WAVE) {
                const u64 p = p0 + (u64)lane_id();
                const u64 m = wave_ballot(p < b && bam_find_ok(j.buf, p, hi));
                if (m) {
                    c = p0 + (u64)__ffsll((unsigned long long)m) - 1;
                    break;
                }
            }
        }
    }
    if (lane_id() == 0) j.cand[s] = c;
}

__global__ void __launch_bounds__(BAMW_THREADS) k_bam_walk_seg(BamWalkJob j) {
    const u32 s = blockIdx.x * (BAMW_THREADS / WAVE) + (u32)wave_in_block();
    if (s >= j.n_seg) return;
    const u64 c = uniform_u64(j.cand[s]);
    if (c == BAMW_NO_CAND) return;
    const u64 hi = j.tail_cap + j.total;
    const u64 a = (u64)s * j.seg_bytes, b = min(a + j.seg_bytes, hi);
    if (c < a || c >= b) return; /* (k_bam_find gives nothing else) */
    const BamSeg o = bam_walk_range(j.buf, c, a, b, hi, j.lists + (size_t)s * j.per_seg, j.per_seg);
    if (lane_id() == 0) j.segs[s] = o;
}

__global__ void __launch_bounds__(WAVE) k_bam_chain(BamWalkJob j) {
    const u32 lane = (u32)lane_id();
    const u64 hi = j.tail_cap + j.total;
    const u32 tl = bamw_tail_len(j);
    const u64 lo = j.tail_cap - tl;
    fpl_bam_window h;
    h.status = FPL_BAMW_OK;
    h.n_reads = 0;
    h.n_bases = 0;
    h.max_read_len = 0;
    h.segments = j.n_seg;
    h.name_bytes = 0;
    h.records_seen = 0;
    h.tail_bytes = 0;
    h.rewalked = 0;
    h.bad_index = 0;
    h.bad_pos = 0;
    auto finish = [&](u32 status) {
        h.status = status;
        if (lane == 0) {
            *j.hdr = h;
            if (status != FPL_BAMW_OK && status != FPL_BAMW_CHAIN) j.st->refused = 1;
        }
    };
    if (uniform_u32(j.st->refused)) {
        finish(FPL_BAMW_CHAIN);
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
            finish(FPL_BAMW_BLOCK);
            return;
        }
    }
    u64 e = min(lo + j.skip, hi); /* the true entry of the next segment that holds a record start */
    u64 c_n = 0, c_off = 0, c_name = 0, c_seen = 0;
    u32 maxl = 0, rew = 0, stop = 0, stop_bad_idx = 0;
    u64 stop_pos = 0;
    for (u32 g = 0; g < j.n_seg; g += WAVE) {
        const u32 s = g + lane;
        BamSeg mine;
        mine.exit = 0;
        mine.sum_lseq = 0;
        mine.taken = mine.skipped = mine.max_lseq = mine.name_bytes = mine.status = mine.bad_idx = 0;
        u64 my_cand = BAMW_NO_CAND;
        if (s < j.n_seg) {
            my_cand = j.cand[s];
            if (my_cand != BAMW_NO_CAND) mine = j.segs[s];
        }
        const WaveVals64 cands = wave_publish(my_cand), exits = wave_publish(mine.exit),
                         stats = wave_publish((u64)mine.status | ((u64)mine.bad_idx << 32));
        u64 used_mask = 0;
        for (u32 k = 0; k < WAVE && g + k < j.n_seg && !stop; k++) {
            const u64 a = (u64)(g + k) * j.seg_bytes, b = min(a + j.seg_bytes, hi);
            if (e >= b) continue; /* a long record passes over the segment (or it lies in front of the tail) */
            u64 ex;
            u32 st, bi;
            if (uniform_u64(cands.get((int)k)) == e) {
                ex = uniform_u64(exits.get((int)k));
                const u64 sv = uniform_u64(stats.get((int)k));
                st = (u32)sv;
                bi = (u32)(sv >> 32);
            } else { /* the guess was wrong, or there was none */
                bamrule::Fields f;
                if (bam_walk_one(j.buf, e, hi, f) == BAMW_NEED) { /* the record at the entry is incomplete -- never a candidate --: the
                                                                     tail starts here, and there is nothing to walk */
                    stop = BAMW_NEED;
                    break;
                }
                /* the segment again, from the entry */
                const BamSeg r = bam_walk_range(j.buf, e, a, b, hi, j.lists + (size_t)(g + k) * j.per_seg, j.per_seg);
                rew++;
                if (lane == k) mine = r;
                ex = r.exit;
                st = r.status;
                bi = r.bad_idx;
            }
            if (st == BAMW_BAD || st == BAMW_FULL) { /* the segment gives nothing: the submission is refused */
                stop = st;
                stop_bad_idx = bi;
                stop_pos = ex;
                break;
            }
            used_mask |= 1ull << k;
            e = ex;
            if (st == BAMW_NEED) stop = BAMW_NEED; /* its whole records count; the tail starts at e, nothing behind it is looked at */
        }
        const bool used = (used_mask >> lane) & 1ull;
        const u32 t = used ? mine.taken : 0u, nb = used ? mine.name_bytes : 0u;
        const u64 ls = used ? mine.sum_lseq : 0ull;
        const u32 t_in = wave_scan_incl_u32(t);
        const u64 ls_in = bamw_scan_incl_u64(ls), nb_in = bamw_scan_incl_u64((u64)nb);
        if (s < j.n_seg) {
            BamSegBase B;
            B.off = c_off + ls_in - ls;
            B.name = c_name + nb_in - nb;
            B.rec = (u32)(c_n + t_in - t);
            B.taken = t;
            j.bases[s] = B;
        }
        c_n += wave_sum_u32(t);
        c_off += uniform_u64(shfl_u64(ls_in, 63));
        c_name += uniform_u64(shfl_u64(nb_in, 63));
        c_seen += wave_sum_u32(used ? mine.taken + mine.skipped : 0u);
        maxl = max(maxl, wave_max_u32(used ? mine.max_lseq : 0u));
    }
    h.rewalked = rew;
    if (stop == BAMW_BAD) {
        h.bad_index = j.st->rec_base + c_seen + stop_bad_idx;
        h.bad_pos = stop_pos - lo;
        finish(FPL_BAMW_RECORD);
        return;
    }
    if (stop == BAMW_FULL || c_n > j.rec_cap || c_name > j.names_cap) {
        finish(FPL_BAMW_TOO_MANY);
        return;
    }
    const u64 tail_src = min(e, hi); /* behind the last whole record: hi, or where an incomplete record starts */
    const u64 tail = hi - tail_src;
    h.tail_bytes = (u32)min(tail, (u64)0xFFFFFFFFu);
    if (tail > j.tail_cap) {
        finish(FPL_BAMW_TAIL_ROOM);
        return;
    }
    h.n_reads = (u32)c_n;
    h.n_bases = c_off;
    h.max_read_len = maxl;
    h.name_bytes = c_name;
    h.records_seen = c_seen;
    if (lane == 0) {
        j.st->tail_len = (u32)tail;
        j.st->rec_base += c_seen;
        j.st->tail_src = tail_src;
        j.off[c_n] = c_off;
        j.name_off[c_n] = c_name;
    }
    finish(FPL_BAMW_OK);
}

__global__ void __launch_bounds__(BAMW_THREADS) k_bam_compact(BamWalkJob j) {
    if (j.hdr->status != FPL_BAMW_OK) return;
    const u64 hi = j.tail_cap + j.total;
    { /* the new tail: the bytes behind the last whole record */
        const u64 tail = j.hdr->tail_bytes, src = j.st->tail_src;
        if (tail <= j.tail_cap && src <= hi && hi - src >= tail)
            for (u64 i = (u64)blockIdx.x * BAMW_THREADS + threadIdx.x; i < tail; i += (u64)gridDim.x * BAMW_THREADS) j.tail_buf[i] = j.buf[src + i];
    }
    const u32 s = blockIdx.x * (BAMW_THREADS / WAVE) + (u32)wave_in_block();
    if (s >= j.n_seg) return;
    const BamSegBase B = j.bases[s];
    const u32 taken = uniform_u32(min(B.taken, j.per_seg));
    if (!taken) return;
    const u32 lane = (u32)lane_id();
    const u64 a = (u64)s * j.seg_bytes;
    const u32* list = j.lists + (size_t)s * j.per_seg;
    u64 c_off = uniform_u64(B.off), c_name = uniform_u64(B.name);
    for (u32 k = 0; k < taken; k += WAVE) {
        const u32 i = k + lane;
        const bool live = i < taken;
        u64 rs = 0, ls = 0, nb = 0;
        if (live) {
            rs = a + list[i];
            const bamrule::Fields f = bamrule::fields(j.buf + rs); /* (a record the chain accepted: whole, inside the buffer) */
            ls = f.l_seq;
            nb = 1 + bam_name_len_lane(j.buf + rs + bamrule::HEAD, f.l_name);
        }
        const u64 ls_in = bamw_scan_incl_u64(ls), nb_in = bamw_scan_incl_u64(nb);
        const u64 r = (u64)B.rec + i;
        if (live && r < j.rec_cap) {
            j.rec_start[r] = rs;
            j.off[r] = c_off + ls_in - ls;
            const u64 no = c_name + nb_in - nb;
            j.name_off[r] = no;
            if (no + nb <= j.names_cap) {
                j.names[no] = '@';
                for (u64 x = 1; x < nb; x++) j.names[no + x] = j.buf[rs + bamrule::HEAD + x - 1];
            }
        }
        c_off += uniform_u64(shfl_u64(ls_in, 63));
        c_name += uniform_u64(shfl_u64(nb_in, 63));
    }
}

#ifdef FPL_EMU
#define BAMW_LAUNCH(kernel, grid, block, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
typedef void* bamw_stream_t;
#else
#define BAMW_LAUNCH(kernel, grid, block, stream, ...) hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__)
typedef hipStream_t bamw_stream_t;
#endif

/* the sizes of a submission of `total` inflated bytes; false: the arguments are refused */
inline bool bam_walk_plan(BamWalkJob& j, uint64_t tail_cap, uint64_t total, uint64_t skip, uint32_t seg_bytes) {
    if (seg_bytes == 0) seg_bytes = BAMW_DEFAULT_SEG;
    if (seg_bytes < BAMW_MIN_SEG || total > 0xFFFFFFF0ull || tail_cap > 0xFFFFFFF0ull || skip > total) return false;
    const uint64_t n_seg = (tail_cap + total + seg_bytes - 1) / seg_bytes;
    if (n_seg == 0 || n_seg > 0x7FFFFFFFull) return false;
    j.tail_cap = tail_cap;
    j.total = total;
    j.skip = skip;
    j.seg_bytes = seg_bytes;
    j.n_seg = (u32)n_seg;
    j.per_seg = seg_bytes / bamrule::HEAD + 1;
    return true;
}
/* records the dense arrays hold for `total` bytes: a record per 64 bytes, as for text; more is FPL_BAMW_TOO_MANY */
inline uint32_t bam_walk_rec_cap(uint64_t total) { return (uint32_t)(total / 64 + 1024); }

/* the five launches of one submission, in stream order (behind k_bgzf_inflate) */
inline void bam_walk_enqueue(const BamWalkJob& j, bamw_stream_t s) {
    const u32 per_block = BAMW_THREADS / WAVE;
    const u32 blocks = (j.n_seg + per_block - 1) / per_block;
    BAMW_LAUNCH(k_bam_place_tail, dim3(std::max<u32>(1, std::min<u32>(64, (u32)(j.tail_cap / BAMW_THREADS + 1)))), dim3(BAMW_THREADS), s, j);
    BAMW_LAUNCH(k_bam_find, dim3(blocks), dim3(BAMW_THREADS), s, j);
    BAMW_LAUNCH(k_bam_walk_seg, dim3(blocks), dim3(BAMW_THREADS), s, j);
    BAMW_LAUNCH(k_bam_chain, dim3(1), dim3(WAVE), s, j);
    BAMW_LAUNCH(k_bam_compact, dim3(blocks), dim3(BAMW_THREADS), s, j);
}

}  // namespace fpl
#endif
