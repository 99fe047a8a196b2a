/*
 * bam_moves.h -- the move table mv and the ts of a BAM batch's input records re-indexed for the trimmed and split records the
 * device composes (fpl_set_bam_moves; include/fastplong_amd.h).  The rule is csrc/bam_move_rules.h's, shared with the host's
 * converter (host/bam_out.cpp): what comes out inflates to what the host makes of the same batch.  With the switch off none of
 * this is launched: the kernels of csrc/bam_tags.h and csrc/bam_mods.h run as they are.
 *
 *   k_bam_tags_moves   k_bam_tags_mods's walk (with fpl_set_bam_mods off, without its notes), and in the same walk where the mv and
 *                      ts fields lie; a record that has an mv and a passing changed fragment is a CANDIDATE and gets a slot
 *   k_bam_moves_plan   in front of the layout and behind k_bam_mods_plan, a wave per candidate.  The moves, 16 bytes a lane a step
 *                      from wherever the field starts (the loads tolerate the offset; behind the table's end a lane's bytes are
 *                      masked away): every byte checked against {0, 1} by one AND per word, a lane's ones counted by popcounts, one
 *                      inclusive wave scan per step with a carry from step to step.  Up to four targets -- the (s + 1)-th and the
 *                      (s + n + 1)-th one of either fragment --: the lane whose running count crosses a target finds the byte
 *                      inside its 16.  With l_seq ones in all, the plan: per fragment a, b, the new ts and its type; the new
 *                      lengths go into BamTagInfo::len, the counters are set right -- a wave sums what its candidates add, a block
 *                      what its waves add, and one thread per counter adds that: every candidate adding for itself made the
 *                      kernel wait for some hundred thousand atomics on seven addresses.  A record or a fragment that fails a
 *                      condition keeps what the kernels before wrote: it is composed as without the switch
 *   k_bamout_compose_bam_moves   the compose with ONE tail for all four combinations of the two switches: a fragment re-indexed for
 *                                neither goes BamModTail's way; else lane 0 walks the fields, and every field is written from the
 *                                modification plan, from the move plan (a 9-byte head and one wave copy of the moves [a, b); ts from
 *                                the plan), verbatim, or not at all
 * The layout kernel is k_bamout_layout_bam_tags: it reads the lengths.  Nothing is read outside the record buffer and its BAM_PAD
 * bytes, nothing written outside [rec_off[i], rec_off[i + 1]): every store is clamped to the length the layout counted.  A
 * re-indexed record's tag bytes never exceed its input region (bam_move_rules.h, SIZE), so bamtag_extra_bound stands.
 */
#ifndef FPL_BAM_MOVES_H
#define FPL_BAM_MOVES_H

#include "bam_mods.h"
#include "bam_move_rules.h"

namespace fpl {

struct BamMoveInfo {
    u32 mv_at, mv_len, ts_at, ts_len; /* in the region; the last field of each tag */
    u32 counts; /* fields tagged mv | ts << 8 (255 at the most each); bit 16: a positional field that is neither tagged mv nor one of MM / ML / MN; bit 17: a positional MM / ML / MN field */
    u32 slot;   /* the candidate's slot, BAMMOD_NONE: not one */
};
struct BamMoveCut {
    u32 a, b;    /* the moves e_a .. e_(b-1) */
    u32 ts;      /* the new value ... */
    u32 ts_type; /* ... and its type (a record with a ts) */
};
struct BamMovePlan {
    BamMoveCut cut[2];
};
/* BamTagInfo::kept, bit 8 + f: fragment f's mv and ts are re-indexed (its len counts them) */
constexpr u32 BAMMOVE_KEPT_SHIFT = 8;
/* the counters of a context: four of fpl_get_bam_move_stats, then the candidates of the batch in flight (zeroed per batch) */
constexpr u32 BAMMOVE_COUNTERS = 5;
/* moves a wave takes in a step */
constexpr u32 BAMMOVE_STEP = 16 * 64;
/* the sums k_bam_moves_plan adds to the counters */
constexpr u32 BAMMOVE_SUMS = 6;

/* what the shared walk notes for this file */
struct BamWalkMoves {
    BamMoveInfo* vinfo;
    u32* cand;
    unsigned long long* move_counters;
    bammove::Found fd;
    bool other, mod_pos;
    __device__ __forceinline__ void begin() { fd = bammove::nothing_found(), other = false, mod_pos = false; }
    __device__ __forceinline__ void field(const u8* p, uint64_t at, uint64_t n, bool positional, bool mod) {
        bammove::note(fd, p, at, n);
        if (positional && mod) mod_pos = true;
        else if (positional && !bammove::mv_tag(p + at)) other = true;
    }
    __device__ __forceinline__ void end(u32 i, bool any_changed, u32 n_rec) {
        BamMoveInfo v;
        v.mv_at = (u32)fd.mv_at, v.mv_len = (u32)fd.mv_len, v.ts_at = (u32)fd.ts_at, v.ts_len = (u32)fd.ts_len;
        v.counts = (fd.n_mv < 255u ? fd.n_mv : 255u) | (fd.n_ts < 255u ? fd.n_ts : 255u) << 8 | (other ? 1u << 16 : 0u) | (mod_pos ? 1u << 17 : 0u);
        v.slot = BAMMOD_NONE;
        if (any_changed && bammove::any_found(fd)) {
            v.slot = (u32)atomicAdd(&move_counters[4], 1ull);
            if (v.slot < n_rec) cand[v.slot] = i;
        }
        vinfo[i] = v;
    }
};
/* minfo, mod_cand, mod_counters: nullptr without fpl_set_bam_mods */
__global__ void __launch_bounds__(256)
k_bam_tags_moves(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
                 u32 fragment_mode, BamTagInfo* __restrict__ info, unsigned long long* __restrict__ counters, BamModInfo* __restrict__ minfo,
                 u32* __restrict__ mod_cand, unsigned long long* __restrict__ mod_counters, BamMoveInfo* __restrict__ vinfo, u32* __restrict__ cand,
                 unsigned long long* __restrict__ move_counters) {
    BamWalkMoves more;
    more.vinfo = vinfo, more.cand = cand, more.move_counters = move_counters;
    bam_tags_mods_body(bam, buf_bytes, rec_start, res, n_rec, fragment_mode, info, counters, minfo, mod_cand, mod_counters, more);
}

/* inclusive scan over the lanes */
__device__ __forceinline__ u32 bammove_wave_scan(u32 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 up = shfl_u32(v, lane_id() - d < 0 ? lane_id() : lane_id() - d);
        if (lane_id() >= d) v += up;
    }
    return v;
}
__device__ __forceinline__ u32 bammove_wave_max(u32 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = shfl_xor_u32(v, d);
        v = o > v ? o : v;
    }
    return v;
}
/* the first `valid` bytes (0..4) of a word */
__device__ __forceinline__ u32 bammove_first_bytes(u32 valid) { return valid >= 4 ? 0xFFFFFFFFu : (1u << (8u * valid)) - 1u; }
/* where the r-th byte equal to 1 (r >= 1; there is one) lies among 16 bytes of 0 and 1 */
__device__ __forceinline__ u32 bammove_nth_one(u64 lo, u64 hi, u32 r) {
    const u32 in_lo = (u32)__popcll(lo);
    u64 x = lo;
    u32 at = 0;
    if (r > in_lo) x = hi, at = 8, r -= in_lo;
    for (u32 k = 1; k < r; k++) x &= x - 1; /* (drop the ones in front of it) */
    return at + ((u32)__builtin_ctzll(x) >> 3);
}

__global__ void __launch_bounds__(256)
k_bam_moves_plan(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
                 u32 fragment_mode, BamTagInfo* __restrict__ info, const BamMoveInfo* __restrict__ vinfo, const u32* __restrict__ cand,
                 BamMovePlan* __restrict__ plans, unsigned long long* __restrict__ counters, unsigned long long* __restrict__ move_counters) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    u64 n_cand = move_counters[4];
    if (n_cand > n_rec) n_cand = n_rec;
    /* what this wave's candidates add to the counters: records that keep every field now, tag bytes (modulo 2^64), then the four of
       fpl_get_bam_move_stats */
    unsigned long long sum[BAMMOVE_SUMS] = {0, 0, 0, 0, 0, 0};
    for (u32 slot = wave; slot < (u32)n_cand; slot += n_waves) { /* wave-uniform */
        const u32 i = cand[slot];
        if (i >= n_rec) continue;
        const u64 rs = rec_start[i];
        const u8* rc = bam + rs;
        const bamrule::Fields fld = bamrule::fields(rc);
        const BamTagInfo t = info[i];
        const BamMoveInfo v = vinfo[i];
        const fpl_read_result r = res[i];
        const u8* p = rc + t.at;
        const bammove::Found fd = {v.counts & 255u, (v.counts >> 8) & 255u, v.mv_at, v.mv_len, v.ts_at, v.ts_len};
        /* the fragments: their ends in the read, and the ones looked for: the (s + 1)-th and the (e + 1)-th (0: none) */
        bool active[2] = {false, false};
        uint64_t s[2] = {0, 0}, e[2] = {0, 0};
        u32 tgt[4] = {0, 0, 0, 0}, pos[4] = {0, 0, 0, 0};
        u32 n_active = 0;
        for (int f = 0; f < 2; f++) {
            if (r.dropped || f >= r.n_frag || r.code[f] != FPL_PASS_FILTER) continue;
            if (bamtag::unchanged(r.n_frag, r.kind[f], r.frag_start[f], r.frag_len[f], fld.l_seq, fld.flag, fragment_mode != 0)) continue;
            active[f] = true, n_active++;
            bammove::clamp_range(r.frag_start[f], r.frag_len[f], fld.l_seq, s[f], e[f]);
            tgt[2 * f] = (u32)s[f] + 1, tgt[2 * f + 1] = (u32)e[f] + 1;
        }
        if (!n_active) continue;
        bammove::Table T;
        bool ok = bammove::fields_ok(fd, p, fld.flag, fragment_mode != 0, T);
        /* (the walk clamped the region to the buffer, so the table lies inside it, and parsed the field, so the count is its length:
           both are asked again here, in front of the loads that rely on them) */
        ok = ok && rs + t.at + v.mv_at + v.mv_len <= buf_bytes && T.m + 9 == v.mv_len;
        /* ---- the moves ---- */
        const u8* mv = p + v.mv_at + 9;
        const u64 m = ok ? T.m : 0;
        u32 carry = 0; /* ones in front of this step */
        for (u64 base = 0; base < m; base += BAMMOVE_STEP) { /* wave-uniform */
            const u64 at = base + 16ull * lane;
            u32x4 q = {0, 0, 0, 0};
            if (at < m) q = load16(mv + at); /* (it may run 15 bytes over the table: other fields, the next record or BAM_PAD) */
            const u32 left = at < m ? (m - at < 16 ? (u32)(m - at) : 16u) : 0u;
            const u32 w0 = q.x & bammove_first_bytes(left), w1 = q.y & bammove_first_bytes(left > 4 ? left - 4 : 0u),
                      w2 = q.z & bammove_first_bytes(left > 8 ? left - 8 : 0u), w3 = q.w & bammove_first_bytes(left > 12 ? left - 12 : 0u);
            if (wave_ballot(((w0 | w1 | w2 | w3) & 0xFEFEFEFEu) != 0)) { /* a move that is neither 0 nor 1 */
                ok = false;
                break;
            }
            const u32 c = (u32)(__popc(w0) + __popc(w1) + __popc(w2) + __popc(w3));
            const u32 incl = carry + bammove_wave_scan(c), excl = incl - c;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (tgt[k] > excl && tgt[k] <= incl) /* (one lane at the most: it holds the tgt[k]-th one) */
                    pos[k] = (u32)at + bammove_nth_one((u64)w0 | (u64)w1 << 32, (u64)w2 | (u64)w3 << 32, tgt[k] - excl) + 1;
            carry = shfl_u32(incl, 63);
        }
        ok = ok && carry == fld.l_seq;
        if (!ok) {
            sum[3] += n_active;
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) pos[k] = bammove_wave_max(pos[k]);
        /* ---- the plan, the lengths and the counters ---- */
        BamTagInfo t2 = t;
        const bool other = (v.counts >> 16 & 1u) != 0, mod_pos = (v.counts >> 17 & 1u) != 0;
        bool done = false;
        for (int f = 0; f < 2; f++) {
            if (!active[f]) continue;
            /* p(k) of the rule: behind the last one lies m + 1 */
            const u64 p_s = s[f] + 1 > fld.l_seq ? m + 1 : pos[2 * f], p_e = e[f] + 1 > fld.l_seq ? m + 1 : pos[2 * f + 1];
            bammove::Cut c;
            bammove::ends(s[f], e[f], p_s, p_e, c);
            if (!bammove::finish(T, c)) {
                sum[3]++;
                continue;
            }
            done = true;
            sum[2]++, sum[4] += c.b - c.a, sum[5] += m - (c.b - c.a);
            const u32 n = t.len[f] + (u32)v.mv_len + (u32)bammove::growth(T, c); /* (the table comes in, less what the fields shrink by) */
            sum[1] += (unsigned long long)n - t.len[f];
            /* counted as "lost positional fields", and keeps every field now */
            if ((t.kept >> f & 1u) && !other && (!mod_pos || (t.kept >> (BAMMOD_KEPT_SHIFT + f) & 1u))) sum[0]++;
            t2.len[f] = n;
            t2.kept |= 1u << (BAMMOVE_KEPT_SHIFT + f);
            if (lane == 0) plans[slot].cut[f] = BamMoveCut{(u32)c.a, (u32)c.b, (u32)c.ts, c.ts_type};
        }
        if (lane == 0 && done) info[i] = t2;
    }
    /* (every lane of a wave holds the wave's sums: the loop and all it adds are wave-uniform) */
    __shared__ unsigned long long wsum[4][BAMMOVE_SUMS];
    if (lane == 0)
#pragma unroll
        for (u32 k = 0; k < BAMMOVE_SUMS; k++) wsum[(threadIdx.x >> 6) & 3u][k] = sum[k];
    __syncthreads();
    if (threadIdx.x < BAMMOVE_SUMS) {
        unsigned long long x = 0;
        for (u32 w = 0; w < 4 && w < (blockDim.x >> 6); w++) x += wsum[w][threadIdx.x];
        if (x) {
            if (threadIdx.x == 0) atomicAdd(&counters[0], x), atomicAdd(&counters[1], 0ull - x);
            else if (threadIdx.x == 1) atomicAdd(&counters[2], x);
            else atomicAdd(&move_counters[threadIdx.x - 2], x);
        }
    }
}

/* BamModTail, and for a fragment whose mv and ts are re-indexed the fields one by one, each by the switch that decides it */
struct BamMoveTail {
    BamModTail mods; /* (minfo and plans nullptr without fpl_set_bam_mods: no fragment carries its bit then) */
    const BamMoveInfo* vinfo;
    const BamMovePlan* vplans;
    __device__ __forceinline__ u8* operator()(u32 i, int f, u32 nl, u32 fl, u8* rec, u8* d) const {
        const BamTagInfo t = mods.tags.info[i];
        if (!(t.kept >> (BAMMOVE_KEPT_SHIFT + f) & 1u)) return mods(i, f, nl, fl, rec, d); /* (wave-uniform) */
        const u32 n = t.len[f];
        const u32 lane = (u32)lane_id();
        const u8* p = mods.tags.bam + mods.tags.rec_start[i] + t.at;
        const BamMoveInfo v = vinfo[i];
        const BamMoveCut c = vplans[v.slot].cut[f];
        const bool re_mods = (t.kept >> (BAMMOD_KEPT_SHIFT + f) & 1u) != 0;
        BamModInfo m = {0, 0, 0, 0, 0, 0, 0, 0, BAMMOD_NONE};
        if (re_mods) m = mods.minfo[i];
        const BamModPlan* plan = re_mods ? mods.plans + m.slot : nullptr;
        const bool has_ts = (v.counts >> 8 & 255u) != 0;
        if (lane < 4) rec[lane] = (u8)((bamout::fixed_word(0, nl, fl) + n) >> (8u * lane));
        BamTailOut w = {d, d + n};
        /* up to 16 bytes a lane each: lane k writes b */
        auto lanes = [&](u32 b, u32 len) {
            if (len > (u32)(w.end - w.d)) len = (u32)(w.end - w.d);
            if (lane < len) w.d[lane] = (u8)b;
            w.d += len;
        };
        for (u32 o = 0; o < t.prefix && w.d < w.end;) { /* wave-uniform */
            const u32 len = bam_tail_field_len(p, o, t.prefix);
            if (re_mods && bammod_put_field(w, p, o, len, m, plan, f, fl)) {
            } else if (o == v.mv_at) { /* tag, B, subtype; the count; the stride; the moves */
                const u32 count = 1u + (c.b - c.a);
                lanes(lane < 4 ? p[o + lane] : lane < 8 ? count >> (8u * (lane - 4)) : p[o + 8], 9);
                w.put(p + o + 8 + c.a, c.b - c.a);
            } else if (has_ts && o == v.ts_at) {
                lanes(lane < 2 ? p[o + lane] : lane == 2 ? c.ts_type : lane < 7 ? c.ts >> (8u * (lane - 3)) : 0u, 3 + bamtag::scalar_size(c.ts_type));
            } else if (!bamtag::positional(p + o))
                w.put(p + o, len);
            o += len;
        }
        return w.end;
    }
};
__global__ void __launch_bounds__(256)
k_bamout_compose_bam_moves(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                           const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const BamTagInfo* __restrict__ info,
                           const BamModInfo* __restrict__ minfo, const BamModPlan* __restrict__ plans, const BamMoveInfo* __restrict__ vinfo,
                           const BamMovePlan* __restrict__ vplans, const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    bamout_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap,
                        BamMoveTail{BamModTail{BamTagTail{bam, rec_start, info}, minfo, plans}, vinfo, vplans});
}

}  // namespace fpl
#endif
