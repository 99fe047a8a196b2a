/*
 * bam_tags.h -- the auxiliary fields of a BAM batch's input records behind the qualities of the records the device composes
 * (fpl_set_bam_tags; include/fastplong_amd.h).  The rule is csrc/bam_tag_rules.h's, shared with the host's converter
 * (host/bam_out.cpp): what comes out inflates to what the host makes of the same batch.
 *
 *   k_bam_tags   full grid, a lane per input record, in front of the layout: walks the record's aux region by the shared rule (Z / H
 *                eight bytes a step, everything else clamped to the region, the region clamped to the record buffer) and writes
 *                where the region lies, its parsed prefix, and for either fragment of the read how many tag bytes it gets and
 *                whether those are the whole prefix or its non-positional fields only; adds to the four counters.  (Not in the
 *                layout kernel: that is ONE block with lane = read, and a chain of some twenty dependent loads per record there
 *                would put the whole batch behind one CU.)
 *   k_bamout_layout_bam_tags    k_bamout_layout_bam with the fragment's tag bytes in part b (behind the qualities); the cut rule is
 *                               unchanged, no forced cut at the first tag byte
 *   k_bamout_compose_bam_tags   k_bamout_compose_bam, and behind a record's qualities one wave copy of the prefix, or the kept
 *                               fields as runs of consecutive kept fields: lane 0 walks, the run's ends are broadcast, the wave copies
 * Nothing is read outside the record, nothing written outside [rec_off[i], rec_off[i + 1]).
 */
#ifndef FPL_BAM_TAGS_H
#define FPL_BAM_TAGS_H

#include "bam_emit.h"
#include "bam_tag_rules.h"

namespace fpl {

struct BamTagInfo {
    u64 at;      /* the region's first byte, from the record's block_size field */
    u32 prefix;  /* bytes of the parsed prefix */
    u32 len[2];  /* tag bytes of fragment 0 / 1 (0: it writes none) */
    u32 kept;    /* bit f: fragment f gets the non-positional fields only (else the prefix verbatim) */
};
/* what the bounds of bam_emit.h grow by with the switch on: both fragments of a split read carry the read's fields, and a field
   is part of its record */
inline u64 bamtag_extra_bound(u64 record_bytes) { return 2 * record_bytes; }

/* the Z / H scan of the shared walk, eight bytes a step: it may read up to 7 bytes behind v + left (the record buffer holds
   BAM_PAD bytes behind its end) and never counts a NUL it finds there */
struct BamTagScan8 {
    FPL_BAMTAG_HD uint64_t operator()(const u8* v, uint64_t left) const {
        for (uint64_t k = 0; k < left; k += 8) {
            u64 w;
            __builtin_memcpy(&w, v + k, 8);
            const u64 z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;
            if (z) {
                const uint64_t at = k + ((u32)__builtin_ctzll(z) >> 3);
                return at < left ? at + 1 : 0;
            }
        }
        return 0;
    }
};

/* counters: kept every field, lost positional fields, tag bytes, regions that did not parse to their end -- per OUTPUT record.
   buf_bytes: the record buffer's extent, which a region never passes whatever block_size says */
__global__ void __launch_bounds__(256)
k_bam_tags(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
           u32 fragment_mode, BamTagInfo* __restrict__ info, unsigned long long* __restrict__ counters) {
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
        const bamtag::Walk w = bamtag::walk(rc + at, len, BamTagScan8());
        const bamrule::Fields fd = bamrule::fields(rc);
        const fpl_read_result r = res[i];
        BamTagInfo t = {(u64)at, (u32)w.prefix, {0, 0}, 0};
        if (!r.dropped)
            for (int f = 0; f < r.n_frag && f < 2; f++) {
                if (r.code[f] != FPL_PASS_FILTER) continue;
                const bool changed = !bamtag::unchanged(r.n_frag, r.kind[f], r.frag_start[f], r.frag_len[f], fd.l_seq, fd.flag, fragment_mode != 0);
                const bool lose = changed && w.positional;
                t.len[f] = (u32)(lose ? w.kept : w.prefix);
                if (lose) t.kept |= 1u << f;
                c[lose ? 1 : 0]++;
                c[2] += t.len[f];
                c[3] += w.whole ? 0 : 1;
            }
        info[i] = t;
    }
    for (int k = 0; k < 4; k++) {
        u64 v = c[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v += shfl_xor_u64(v, d);
        if (lane_id() == 0 && v) atomicAdd(&counters[k], (unsigned long long)v);
    }
}

/* the BAM source with the tags' lengths beside every record */
struct GzRecTags : GzRec {
    u32 tag_len[2];
};
struct GzBamTagSrc : GzBamSrc {
    typedef GzRecTags Rec;
    const BamTagInfo* info;
    __device__ __forceinline__ GzRecTags with(const GzRec& g, u32 r) const {
        GzRecTags t;
        (GzRec&)t = g;
        t.tag_len[0] = info[r].len[0], t.tag_len[1] = info[r].len[1];
        return t;
    }
    __device__ __forceinline__ GzRecTags rec(u32 r) const { return with(GzBamSrc::rec(r), r); }
    __device__ __forceinline__ GzRecTags rec_wave(u32 r) const { return with(GzBamSrc::rec_wave(r), r); }
};
/* BamRecForm with the tag bytes in part b: behind the qualities */
struct BamTagRecForm {
    static __device__ __forceinline__ void prep(GzRec& g) { BamRecForm::prep(g); }
    static __device__ __forceinline__ void frag_len(const GzRecTags& g, const fpl_read_result& r, int f, u64& a, u64& b) {
        BamRecForm::frag_len(g, r, f, a, b);
        b += g.tag_len[f];
    }
};
__global__ void __launch_bounds__(1024)
k_bamout_layout_bam_tags(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                         const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const BamTagInfo* __restrict__ info,
                         u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_body<BamTagRecForm>(GzBamTagSrc{{bam, rec_start, seq, qual, off}, info}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}

/* what bamout_compose_body appends behind fragment f's qualities at d (the whole wave calls it) -> the record's new end */
struct BamTagTail {
    const u8* bam;
    const uint64_t* rec_start;
    const BamTagInfo* info;
    __device__ __forceinline__ u8* operator()(u32 i, int f, u32 nl, u32 fl, u8* rec, u8* d) const {
        const BamTagInfo t = info[i];
        const u32 n = t.len[f];
        if (n == 0) return d; /* (wave-uniform) */
        const u8* p = bam + rec_start[i] + t.at;
        /* block_size counts the tag bytes */
        if (lane_id() < 4) rec[lane_id()] = (u8)((bamout::fixed_word(0, nl, fl) + n) >> (8u * (u32)lane_id()));
        if (!(t.kept >> f & 1u)) {
            gz_wave_copy(d, p, n);
            return d + n;
        }
        /* the kept fields, run by run: lane 0 finds the next run of consecutive kept fields inside the parsed prefix */
        u8* const end = d + n;
        for (u32 o = 0; o < t.prefix && d < end;) { /* wave-uniform */
            u32 s = t.prefix, e = t.prefix;
            if (lane_id() == 0) {
                u32 x = o;
                auto step = [&](u32 at) { /* (every field of the prefix parses: k_bam_tags walked it by the same rule) */
                    const u32 len = (u32)bamtag::field_len(p + at, t.prefix - at, BamTagScan8());
                    return len ? len : t.prefix - at;
                };
                while (x < t.prefix && bamtag::positional(p + x)) x += step(x);
                s = x;
                while (x < t.prefix && !bamtag::positional(p + x)) x += step(x);
                e = x;
            }
            s = shfl_u32(s, 0), e = shfl_u32(e, 0);
            u32 run = e - s;
            if (run > (u32)(end - d)) run = (u32)(end - d); /* (never: the lengths are k_bam_tags's) */
            gz_wave_copy(d, p + s, run);
            d += run;
            o = e;
        }
        return end;
    }
};
__global__ void __launch_bounds__(256)
k_bamout_compose_bam_tags(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                          const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const BamTagInfo* __restrict__ info,
                          const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    bamout_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap, BamTagTail{bam, rec_start, info});
}

}  // namespace fpl
#endif
