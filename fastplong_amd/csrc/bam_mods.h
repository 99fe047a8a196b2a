/*
 * bam_mods.h -- MM / ML / MN of a BAM batch's input records re-indexed for the trimmed and split records the device composes
 * (fpl_set_bam_mods; include/fastplong_amd.h).  The rule is csrc/bam_mod_rules.h's, shared with the host's converter
 * (host/bam_out.cpp): what comes out inflates to what the host makes of the same batch.  With the switch off none of this is
 * launched: csrc/bam_tags.h's kernels run as they are.
 *
 *   k_bam_tags_mods   k_bam_tags, and in the same walk of a record's fields where its MM / ML / MN fields lie; a record that has
 *                     one and a passing changed fragment is a CANDIDATE and gets a slot in the candidate list
 *   k_bam_mods_plan   in front of the layout, a wave per candidate.  (1) the record's packed bases, 16 bytes a lane a step: A, C, G
 *                     and T counted by nibble compares up to either fragment's two ends and the read's own (an end at an odd base
 *                     splits a byte; the zero nibble behind an odd l_seq lies behind every end).  (2) the MM value, 64 bytes a
 *                     step, a lane a byte: a ballot of ',' and ';', every delimiter lane reads the digits in front of it (a delta
 *                     when a ',' stands in front of 1 to 9 digits, else the end of a group's header, which that lane checks), an
 *                     inclusive scan of (delta + 1) that carries from step to step and starts again behind every ';', and ballots
 *                     of the lanes whose occurrence lies in a fragment: the first and the last of them are j0 and j1 - 1.
 *                     (3) the plan: per fragment and group the new first delta, the verbatim delta bytes, the ML bytes; the new
 *                     lengths go into BamTagInfo::len, the counters are set right.  A record that is not re-indexable keeps what
 *                     k_bam_tags_mods wrote: it is composed as without the switch
 *   k_bamout_compose_bam_mods   k_bamout_compose_bam_tags with a tail that writes a re-indexed fragment's fields one by one:
 *                               lane 0 walks, the wave copies; the three fields come from the plan
 * The layout kernel is k_bamout_layout_bam_tags: it reads the lengths.  Nothing is read outside the record buffer and its BAM_PAD
 * bytes, nothing written outside [rec_off[i], rec_off[i + 1]).  A re-indexed record's tag bytes never exceed its input region
 * (bam_mod_rules.h, SIZE), so bamtag_extra_bound stands.
 */
#ifndef FPL_BAM_MODS_H
#define FPL_BAM_MODS_H

#include "bam_mod_rules.h"
#include "bam_tags.h"

namespace fpl {

constexpr u32 BAMMOD_NONE = 0xFFFFFFFFu;

struct BamModInfo {
    u32 mm_at, mm_len, ml_at, ml_len, mn_at, mn_len; /* in the region; the last field of each tag */
    u32 counts; /* fields tagged MM | ML << 8 | MN << 16 (255 at the most each); bit 24: another positional field; bit 25: the MN field is kept by bam_tag_rules.h (Mn) */
    u32 kept;   /* bytes of the non-positional fields */
    u32 slot;   /* the candidate's slot, BAMMOD_NONE: not one */
};
struct BamModCut {
    u32 first; /* the new first delta, BAMMOD_NONE: the group keeps nothing */
    u32 rest_at, rest_len; /* the verbatim delta bytes, in the MM value */
    u32 ml_at, ml_len;     /* in the ML values */
};
struct BamModPlan {
    u32 n_groups;
    u32 hdr_at[bammod::MAX_GROUPS], hdr_len[bammod::MAX_GROUPS];
    BamModCut cut[2][bammod::MAX_GROUPS];
    u32 ml_count[2];
};
/* BamTagInfo::kept, bit 4 + f: fragment f is re-indexed (its len is the new one) */
constexpr u32 BAMMOD_KEPT_SHIFT = 4;
/* the counters of a context: four of fpl_get_bam_mod_stats, then the candidates of the batch in flight (zeroed per batch) */
constexpr u32 BAMMOD_COUNTERS = 5;

/* what a sibling of k_bam_tags_mods notes in the same walk (csrc/bam_moves.h): here, nothing */
struct BamWalkNoMore {
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void field(const u8*, uint64_t, uint64_t, bool, bool) {}
    __device__ __forceinline__ void end(u32, bool, u32) {}
};
/* the walk of k_bam_tags_mods.  more: begin() per record, field(p, at, n, positional, mod) per field of its prefix, end(i, a passing
   fragment is changed, n_rec).  minfo == nullptr (a sibling's run without fpl_set_bam_mods): the modification fields are not noted */
template <class More>
__device__ __forceinline__ void bam_tags_mods_body(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start,
                                                   const fpl_read_result* __restrict__ res, u32 n_rec, u32 fragment_mode, BamTagInfo* __restrict__ info,
                                                   unsigned long long* __restrict__ counters, BamModInfo* __restrict__ minfo, u32* __restrict__ cand,
                                                   unsigned long long* __restrict__ mod_counters, More more) {
    unsigned long long c[4] = {0, 0, 0, 0};
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_rec; i += gridDim.x * blockDim.x) {
        const u64 rs = rec_start[i];
        const u8* rc = bam + rs;
        uint64_t at, len;
        bamtag::region(rc, at, len);
        const uint64_t room = buf_bytes > rs ? buf_bytes - rs : 0;
        if (at > room) at = room, len = 0;
        if (len > room - at) len = room - at;
        if (len > 0xFFFFFFFFull) len = 0xFFFFFFFFull;
        /* bamtag::walk and bammod::find in one pass */
        const u8* p = rc + at;
        bamtag::Walk w = {0, 0, false, false};
        bammod::Found fd = bammod::nothing_found();
        bool other = false;
        more.begin();
        while (w.prefix < len) {
            const uint64_t n = bamtag::field_len(p + w.prefix, len - w.prefix, BamTagScan8());
            if (!n) break;
            const u8* f = p + w.prefix;
            const bool mod = bammod::mm_tag(f) || bammod::ml_tag(f) || bammod::mn_tag(f);
            if (bamtag::positional(f)) w.positional = true, other = other || !mod;
            else w.kept += n;
            bammod::note(fd, p, w.prefix, n);
            more.field(p, w.prefix, n, bamtag::positional(f), mod);
            w.prefix += n;
        }
        w.whole = w.prefix == len;
        const bamrule::Fields fld = bamrule::fields(rc);
        const fpl_read_result r = res[i];
        BamTagInfo t = {(u64)at, (u32)w.prefix, {0, 0}, 0};
        bool any_changed = false;
        if (!r.dropped)
            for (int f = 0; f < r.n_frag && f < 2; f++) {
                if (r.code[f] != FPL_PASS_FILTER) continue;
                const bool changed = !bamtag::unchanged(r.n_frag, r.kind[f], r.frag_start[f], r.frag_len[f], fld.l_seq, fld.flag, fragment_mode != 0);
                const bool lose = changed && w.positional;
                any_changed = any_changed || changed;
                t.len[f] = (u32)(lose ? w.kept : w.prefix);
                if (lose) t.kept |= 1u << f;
                c[lose ? 1 : 0]++;
                c[2] += t.len[f];
                c[3] += w.whole ? 0 : 1;
            }
        info[i] = t;
        more.end(i, any_changed, n_rec);
        if (!minfo) continue;
        BamModInfo m;
        m.mm_at = (u32)fd.mm_at, m.mm_len = (u32)fd.mm_len, m.ml_at = (u32)fd.ml_at, m.ml_len = (u32)fd.ml_len, m.mn_at = (u32)fd.mn_at, m.mn_len = (u32)fd.mn_len;
        m.counts = (fd.n_mm < 255u ? fd.n_mm : 255u) | (fd.n_ml < 255u ? fd.n_ml : 255u) << 8 | (fd.n_mn < 255u ? fd.n_mn : 255u) << 16 | (other ? 1u << 24 : 0u);
        if (fd.n_mn && !bamtag::positional(p + fd.mn_at)) m.counts |= 1u << 25;
        m.kept = (u32)w.kept;
        m.slot = BAMMOD_NONE;
        if (any_changed && bammod::any_found(fd)) {
            m.slot = (u32)atomicAdd(&mod_counters[4], 1ull);
            if (m.slot < n_rec) cand[m.slot] = i;
        }
        minfo[i] = m;
    }
    for (int k = 0; k < 4; k++) {
        u64 v = c[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v += shfl_xor_u64(v, d);
        if (lane_id() == 0 && v) atomicAdd(&counters[k], (unsigned long long)v);
    }
}
__global__ void __launch_bounds__(256)
k_bam_tags_mods(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
                u32 fragment_mode, BamTagInfo* __restrict__ info, unsigned long long* __restrict__ counters, BamModInfo* __restrict__ minfo,
                u32* __restrict__ cand, unsigned long long* __restrict__ mod_counters) {
    bam_tags_mods_body(bam, buf_bytes, rec_start, res, n_rec, fragment_mode, info, counters, minfo, cand, mod_counters, BamWalkNoMore{});
}

/* nibbles of the word (4 packed bytes, 8 bases) equal to code: bit 4 k of the result for nibble k */
__device__ __forceinline__ u32 bammod_eq_nibbles(u32 word, u32 code) {
    const u32 x = word ^ (code * 0x11111111u);
    return ~(x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u;
}
/* the nibbles of the first r bases (0 <= r <= 8) of such a word: base 2 k is the HIGH nibble of byte k */
__device__ __forceinline__ u32 bammod_first_bases(u32 r) {
    const u32 sh = 8u * (r >> 1);
    const u64 m = ((1ull << sh) - 1ull) | ((r & 1u) ? 0xF0ull << sh : 0ull);
    return (u32)m;
}
__device__ __forceinline__ u32 bammod_wave_sum(u32 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += shfl_xor_u32(v, d);
    return v;
}
/* inclusive scan over the lanes */
__device__ __forceinline__ u64 bammod_wave_scan(u64 v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = shfl_u64(v, lane_id() - d < 0 ? lane_id() : lane_id() - d);
        if (lane_id() >= d) v += up;
    }
    return v;
}
__device__ __forceinline__ u64 bammod_lanes_below(u32 lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ u64 bammod_lanes_from_to(u32 lo, u32 hi) { /* lo <= hi <= 63 */
    return (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1ull) & ~bammod_lanes_below(lo);
}

__global__ void __launch_bounds__(256)
k_bam_mods_plan(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
                u32 fragment_mode, BamTagInfo* __restrict__ info, const BamModInfo* __restrict__ minfo, const u32* __restrict__ cand,
                BamModPlan* __restrict__ plans, unsigned long long* __restrict__ counters, unsigned long long* __restrict__ mod_counters) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    u64 n_cand = mod_counters[4];
    if (n_cand > n_rec) n_cand = n_rec;
    for (u32 slot = wave; slot < (u32)n_cand; slot += n_waves) { /* wave-uniform */
        const u32 i = cand[slot];
        if (i >= n_rec) continue;
        const u64 rs = rec_start[i];
        const u8* rc = bam + rs;
        const bamrule::Fields fld = bamrule::fields(rc);
        const BamTagInfo t = info[i];
        const BamModInfo m = minfo[i];
        const fpl_read_result r = res[i];
        const u8* p = rc + t.at;
        BamModPlan* plan = plans + slot;
        bammod::Found fd = {m.counts & 255u, (m.counts >> 8) & 255u, (m.counts >> 16) & 255u, m.mm_at, m.mm_len, m.ml_at, m.ml_len, m.mn_at, m.mn_len};
        const u64 pk_at = bamrule::qual_offset(fld) - ((u64)fld.l_seq + 1) / 2, pk_bytes = ((u64)fld.l_seq + 1) / 2;
        bool ok = !(fld.flag & 0x10u) && !fragment_mode && bammod::fields_ok(fd, p, fld.l_seq) && rs + pk_at + pk_bytes <= buf_bytes;
        /* the fragments: their ends in the read */
        bool active[2] = {false, false};
        u32 end[5] = {0, 0, 0, 0, fld.l_seq}; /* s0, e0, s1, e1, l_seq */
        u32 n_active = 0;
        for (int f = 0; f < 2; f++) {
            if (r.dropped || f >= r.n_frag || r.code[f] != FPL_PASS_FILTER) continue;
            if (bamtag::unchanged(r.n_frag, r.kind[f], r.frag_start[f], r.frag_len[f], fld.l_seq, fld.flag, fragment_mode != 0)) continue;
            active[f] = true, n_active++;
            const u64 a = r.frag_start[f], b = (u64)r.frag_start[f] + r.frag_len[f];
            end[2 * f] = (u32)(a < fld.l_seq ? a : fld.l_seq), end[2 * f + 1] = (u32)(b < fld.l_seq ? b : fld.l_seq);
        }
        if (!n_active) continue;
        /* ---- (1) the bases: cnt[e][c], code 1 << c among the first end[e] bases ---- */
        u32 cnt[5][4];
        for (int e = 0; e < 5; e++)
            for (int c = 0; c < 4; c++) cnt[e][c] = 0;
        if (ok) {
            const u8* pk = rc + pk_at;
            for (u64 b0 = 16ull * lane; b0 < pk_bytes; b0 += 16 * 64) { /* (a load may run 15 bytes over the packed bases: qualities, fields or BAM_PAD) */
                const u32x4 v = load16(pk + b0);
                const u32 word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u64 base0 = 2 * (b0 + 4 * (u64)k);
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const u32 z = bammod_eq_nibbles(word[k], 1u << c);
#pragma unroll
                        for (int e = 0; e < 5; e++) {
                            const u32 r8 = end[e] <= base0 ? 0u : (end[e] - base0 >= 8 ? 8u : (u32)(end[e] - base0));
                            cnt[e][c] += (u32)__popc(z & bammod_first_bases(r8));
                        }
                    }
                }
            }
            for (int e = 0; e < 5; e++)
                for (int c = 0; c < 4; c++) cnt[e][c] = bammod_wave_sum(cnt[e][c]);
        }
        /* ---- (2) the MM value ---- */
        const u8* v = p + m.mm_at + 3;
        const u32 L = ok ? m.mm_len - 4 : 0;
        u64 sum = 0, ml_base = 0; /* of the open group: (delta + 1) so far; ML values in front of the group */
        u32 j = 0, gs = 0, n_groups = 0; /* its deltas so far, its first byte; closed groups */
        bool last_semi = true;           /* the last delimiter so far is a ';' (or there is none) */
        u32 g_hl = 0, g_k = 1, g_code = 0;
        bool have[2] = {false, false};
        u32 first[2] = {0, 0}, rat[2] = {0, 0}, rend[2] = {0, 0}, j0[2] = {0, 0}, j1[2] = {0, 0};
        u32 mm_new[2] = {4, 4}, ml_new[2] = {0, 0}, kept[2] = {0, 0}, gone[2] = {0, 0};
        for (u32 base = 0; base < L && ok; base += 64) { /* wave-uniform */
            const u32 pos = base + lane;
            const u32 ch = pos < L ? v[pos] : 0u;
            const bool semi = ch == ';', delim = semi || ch == ',';
            const u64 S = wave_ballot(semi), D = wave_ballot(delim);
            u32 nd = 0, hl = 0, hk = 1, hcode = 0;
            bool is_delta = false, is_hdr = false, bad = false;
            u64 val = 0;
            if (delim) {
                while (nd < bammod::MAX_DIGITS + 1 && pos > nd && bammod::digit(v[pos - nd - 1])) nd++;
                const u32 q = pos > nd ? v[pos - nd - 1] : (u32)';';
                if (q == ',') {
                    is_delta = nd >= 1 && nd <= bammod::MAX_DIGITS;
                    bad = !is_delta;
                    if (is_delta) val = (u64)bammod::number(v, pos - nd, pos) + 1;
                } else {
                    is_hdr = true;
                    const u64 below = D & bammod_lanes_below(lane), sbelow = S & bammod_lanes_below(lane);
                    const bool prev_semi = below ? ((S >> (63 - __clzll(below))) & 1ull) != 0 : last_semi;
                    const u32 gstart = sbelow ? base + (63 - (u32)__clzll(sbelow)) + 1 : gs;
                    hl = bammod::header_len(v, L, gstart, hcode, hk);
                    bad = !prev_semi || hl == 0 || hl != pos - gstart;
                }
            }
            if (wave_ballot(bad)) {
                ok = false;
                break;
            }
            const u64 Dm = wave_ballot(is_delta), Hm = wave_ballot(is_hdr);
            const u64 P = bammod_wave_scan(val);
            u32 lo = 0;
            u64 rest = S;
            for (;;) { /* the groups of this step: wave-uniform */
                const bool closed = rest != 0;
                const u32 hi = closed ? (u32)__builtin_ctzll(rest) : 63u;
                const u64 seg = bammod_lanes_from_to(lo, hi);
                if (Hm & seg) {
                    const int h = __builtin_ctzll(Hm & seg);
                    g_hl = shfl_u32(hl, h), g_k = shfl_u32(hk, h), g_code = shfl_u32(hcode, h);
                }
                const u64 p_base = lo ? shfl_u64(P, (int)lo - 1) : 0;
                const u64 o_incl = sum + P - p_base; /* occurrences up to and including this lane's delta */
                const u32 j_incl = j + (u32)__popcll(Dm & seg & (bammod_lanes_below(lane) | (1ull << lane)));
                const u32 cs = bammod::code_slot(g_code);
                for (int f = 0; f < 2; f++) {
                    if (!active[f]) continue; /* wave-uniform */
                    u32 c0 = end[2 * f], c1 = end[2 * f + 1];
                    for (int c = 0; c < 4; c++)
                        if (cs == (u32)c) c0 = cnt[2 * f][c], c1 = cnt[2 * f + 1][c];
                    const bool in = is_delta && ((seg >> lane) & 1ull) && o_incl - 1 >= c0 && o_incl - 1 < c1;
                    const u64 im = wave_ballot(in);
                    if (!im) continue;
                    const int a = __builtin_ctzll(im), b = 63 - __clzll(im);
                    if (!have[f]) {
                        have[f] = true;
                        first[f] = (u32)(shfl_u64(o_incl, a) - 1 - c0);
                        rat[f] = base + (u32)a;
                        j0[f] = shfl_u32(j_incl, a) - 1;
                    }
                    rend[f] = base + (u32)b;
                    j1[f] = shfl_u32(j_incl, b);
                }
                const u64 sum_end = sum + shfl_u64(P, (int)hi) - p_base;
                const u32 j_end = j + (u32)__popcll(Dm & seg);
                if (!closed) {
                    sum = sum_end, j = j_end;
                    break;
                }
                u64 total = fld.l_seq;
                for (int c = 0; c < 4; c++)
                    if (cs == (u32)c) total = cnt[4][c];
                if (sum_end > total || n_groups == bammod::MAX_GROUPS) {
                    ok = false;
                    break;
                }
                for (int f = 0; f < 2; f++) {
                    const u32 n_kept = have[f] ? j1[f] - j0[f] : 0u;
                    BamModCut cut = {BAMMOD_NONE, 0, 0, 0, 0};
                    if (have[f]) {
                        cut.first = first[f], cut.rest_at = rat[f], cut.rest_len = rend[f] - rat[f];
                        cut.ml_at = (u32)(ml_base + (u64)j0[f] * g_k), cut.ml_len = n_kept * g_k;
                        mm_new[f] += 1 + bammod::digits_of(first[f]) + cut.rest_len;
                    }
                    if (lane == 0) plan->cut[f][n_groups] = cut;
                    mm_new[f] += g_hl + 1;
                    ml_new[f] += n_kept * g_k;
                    kept[f] += n_kept, gone[f] += j_end - n_kept;
                    have[f] = false;
                }
                if (lane == 0) plan->hdr_at[n_groups] = gs, plan->hdr_len[n_groups] = g_hl;
                ml_base += (u64)j_end * g_k;
                n_groups++;
                sum = 0, j = 0, gs = base + hi + 1;
                rest &= rest - 1;
                lo = hi + 1;
                if (lo > 63) break;
            }
            if (D) last_semi = ((S >> (63 - __clzll(D))) & 1ull) != 0;
        }
        ok = ok && gs == L && ml_base == (u64)bamrule::rd32(p + m.ml_at + 4);
        /* ---- (3) the lengths and the counters ---- */
        if (!ok) {
            if (lane == 0) atomicAdd(&mod_counters[1], (unsigned long long)n_active);
            continue;
        }
        BamTagInfo t2 = t;
        const bool other = (m.counts >> 24 & 1u) != 0;
        unsigned long long add_kept = 0, add_gone = 0, bytes = 0, moved = 0;
        for (int f = 0; f < 2; f++) {
            if (!active[f]) continue;
            const u32 n = m.kept - ((m.counts >> 25 & 1u) ? m.mn_len : 0u) + mm_new[f] + 8u + ml_new[f] + (fd.n_mn ? m.mn_len : 0u);
            bytes += (unsigned long long)n - t.len[f];
            if ((t.kept >> f & 1u) && !other) moved++; /* counted as "lost positional fields", and keeps every field now */
            t2.len[f] = n;
            t2.kept |= 1u << (BAMMOD_KEPT_SHIFT + f);
            add_kept += kept[f], add_gone += gone[f];
            if (lane == 0) plan->ml_count[f] = ml_new[f];
        }
        if (lane == 0) {
            plan->n_groups = n_groups;
            info[i] = t2;
            if (moved) atomicAdd(&counters[0], moved), atomicAdd(&counters[1], 0ull - moved);
            if (bytes) atomicAdd(&counters[2], bytes); /* (modulo 2^64: a record may shrink) */
            atomicAdd(&mod_counters[0], (unsigned long long)n_active);
            if (add_kept) atomicAdd(&mod_counters[2], add_kept);
            if (add_gone) atomicAdd(&mod_counters[3], add_gone);
        }
    }
}

/* where a tail that writes a fragment's fields one by one stands: d runs to end, the fragment's last tag byte */
struct BamTailOut {
    u8* d;
    u8* end;
    /* len bytes of src, never past the fragment's end (never: the lengths are the plan kernels') */
    __device__ __forceinline__ void put(const u8* src, u32 len) {
        if (len > (u32)(end - d)) len = (u32)(end - d);
        gz_wave_copy(d, src, len);
        d += len;
    }
};
/* the field of len bytes at p + o of a fragment whose modification fields are re-indexed: one of the three is written from the plan
   (true), any other is left to the caller */
__device__ __forceinline__ bool bammod_put_field(BamTailOut& w, const u8* p, u32 o, u32 len, const BamModInfo& m, const BamModPlan* plan, int f, u32 fl) {
    const u32 lane = (u32)lane_id();
    const bool has_mn = (m.counts >> 16 & 255u) != 0;
    if (o == m.mm_at) {
        const u8* v = p + o + 3;
        w.put(p + o, 3);
        for (u32 g = 0; g < plan->n_groups && g < bammod::MAX_GROUPS; g++) {
            w.put(v + plan->hdr_at[g], plan->hdr_len[g]);
            const BamModCut c = plan->cut[f][g];
            if (c.first != BAMMOD_NONE) {
                const u32 nd = bammod::digits_of(c.first);
                u8 head[16]; /* ',' and the digits */
                head[0] = (u8)',';
                u32 x = c.first;
                for (u32 k = nd; k >= 1; k--) head[k] = (u8)('0' + x % 10u), x /= 10u;
                const u32 hn = nd + 1 > (u32)(w.end - w.d) ? (u32)(w.end - w.d) : nd + 1;
                if (lane < hn) w.d[lane] = head[lane];
                w.d += hn;
                w.put(v + c.rest_at, c.rest_len);
            }
            const u8 semi = (u8)';';
            if (w.d < w.end) {
                if (lane == 0) w.d[0] = semi;
                w.d++;
            }
        }
        if (w.d < w.end) {
            if (lane == 0) w.d[0] = 0;
            w.d++;
        }
        return true;
    }
    if (o == m.ml_at) {
        w.put(p + o, 4);
        if (w.end - w.d >= 4) {
            if (lane < 4) w.d[lane] = (u8)(plan->ml_count[f] >> (8u * lane));
            w.d += 4;
        }
        for (u32 g = 0; g < plan->n_groups && g < bammod::MAX_GROUPS; g++) {
            const BamModCut c = plan->cut[f][g];
            if (c.first != BAMMOD_NONE) w.put(p + o + 8 + c.ml_at, c.ml_len);
        }
        return true;
    }
    if (has_mn && o == m.mn_at) {
        w.put(p + o, 3);
        const u32 nv = len - 3 > (u32)(w.end - w.d) ? (u32)(w.end - w.d) : len - 3;
        if (lane < nv) w.d[lane] = (u8)(lane < 4 ? fl >> (8u * lane) : 0u);
        w.d += nv;
        return true;
    }
    return false;
}
/* the bytes of the next field of the prefix, at p + o: lane 0 walks */
__device__ __forceinline__ u32 bam_tail_field_len(const u8* p, u32 o, u32 prefix) {
    u32 len = 0;
    if (lane_id() == 0) {
        len = (u32)bamtag::field_len(p + o, prefix - o, BamTagScan8());
        if (!len) len = prefix - o; /* (every field of the prefix parses: the walk kernel went over it by the same rule) */
    }
    return shfl_u32(len, 0);
}
/* BamTagTail, and for a re-indexed fragment the fields one by one */
struct BamModTail {
    BamTagTail tags;
    const BamModInfo* minfo;
    const BamModPlan* plans;
    __device__ __forceinline__ u8* operator()(u32 i, int f, u32 nl, u32 fl, u8* rec, u8* d) const {
        const BamTagInfo t = tags.info[i];
        if (!(t.kept >> (BAMMOD_KEPT_SHIFT + f) & 1u)) return tags(i, f, nl, fl, rec, d); /* (wave-uniform) */
        const u32 n = t.len[f];
        const u32 lane = (u32)lane_id();
        const u8* p = tags.bam + tags.rec_start[i] + t.at;
        const BamModInfo m = minfo[i];
        const BamModPlan* plan = plans + m.slot;
        if (lane < 4) rec[lane] = (u8)((bamout::fixed_word(0, nl, fl) + n) >> (8u * lane));
        BamTailOut w = {d, d + n};
        for (u32 o = 0; o < t.prefix && w.d < w.end;) { /* wave-uniform */
            const u32 len = bam_tail_field_len(p, o, t.prefix);
            if (!bammod_put_field(w, p, o, len, m, plan, f, fl) && !bamtag::positional(p + o)) w.put(p + o, len);
            o += len;
        }
        return w.end;
    }
};
__global__ void __launch_bounds__(256)
k_bamout_compose_bam_mods(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                          const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const BamTagInfo* __restrict__ info,
                          const BamModInfo* __restrict__ minfo, const BamModPlan* __restrict__ plans, const u64* __restrict__ rec_off,
                          u8* __restrict__ comp, u64 comp_cap) {
    bamout_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap,
                        BamModTail{BamTagTail{bam, rec_start, info}, minfo, plans});
}

}  // namespace fpl
#endif
