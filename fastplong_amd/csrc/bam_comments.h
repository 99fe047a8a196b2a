/*
 * bam_comments.h -- the auxiliary fields of a BAM batch's input records as COMMENTS behind the names of the FASTQ text the device
 * composes (fpl_set_bam_comments; include/fastplong_amd.h).  The rule is csrc/bam_comment_rules.h's, shared with the host's form
 * (host/bam_comments.cpp): what comes out inflates to what the host makes of the same batch.  With the switch off none of this is
 * launched: k_gz_layout_bam / k_gz_compose_bam run as they are.
 *
 * Which bytes a fragment's record would carry is what k_bam_tags_mods and k_bam_mods_plan (csrc/bam_mods.h) already say, and how
 * to write them is what BamTagTail / BamModTail already do.  So the fields are MATERIALISED first and formatted from there:
 *
 *   k_bam_comment_tags   a wave per input record, full grid: BamModTail writes either fragment's tag bytes -- the prefix verbatim,
 *                        the kept fields, or the re-indexed ones -- into a scratch array of the record buffer's size, fragment f
 *                        of record i at rec_start[i] + (where its region lies) of array f.  No scan is needed: a record's tag
 *                        bytes never exceed its input region (bam_mod_rules.h, SIZE).  The four bytes in front, inside the same
 *                        record's span, take the block_size the tails patch
 *   k_bam_comment_len    a wave per input record, full grid, in front of the layout (which is ONE block with a lane per record and
 *                        must not walk fields): the text bytes of either fragment's comment, and the four counters
 *   k_gz_layout_bam_comments    gz_layout_body over a source whose record carries the two lengths; they are part of a fragment's
 *                               name line (part a).  Same cuts, no new forced cut
 *   k_gz_compose_bam_comments   gz_compose_body with the comment written behind the name
 *
 * The text is written ONCE, bamcomment_wave_text, templated on a sink: BamNoteCount for the length kernel, BamNoteStore for the
 * compose kernel.  Lane 0 walks the fields (bamtag::field_len with BamTagScan8, as BamTagTail does) and the wave takes each:
 * a scalar is formatted by every lane alike and stored by the first lanes; a Z / H value goes through gz_wave_copy after a ballot
 * for control bytes; a B array goes 64 elements a step -- a lane formats its element with its comma, an inclusive scan of the widths
 * gives every lane its offset, the step's total is wave-uniform.
 *
 * Nothing is read outside the record buffer with its BAM_PAD bytes or the scratch arrays (the same size), nothing written outside
 * [rec_off[i], rec_off[i + 1]): every store of the compose form is clamped to the comment's end, which the length kernel found.
 */
#ifndef FPL_BAM_COMMENTS_H
#define FPL_BAM_COMMENTS_H

#include "bam_comment_rules.h"
#include "bam_mods.h"

namespace fpl {

/* what the bounds of gz_emit.h grow by with the switch on: both fragments of a split read carry the read's fields as text, a
   field's text is at most 5 times its bytes (bamcomment::field_text_bound), and a record's tag bytes never exceed its region */
inline u64 bamcomment_extra_bound(u64 record_bytes) { return 2 * bamcomment::field_text_bound(record_bytes); }

/* ---- the sinks ---- */
struct BamNoteCount {
    u64 n = 0;
    __device__ __forceinline__ void head(const u8*, u32, u32 k) { n += k; }
    __device__ __forceinline__ void copy(const u8*, u32 len) { n += len; }
    __device__ __forceinline__ void lanes(const char*, u32, u32, u32 total) { n += total; }
};
struct BamNoteStore {
    u8* d;
    u8* end;
    __device__ __forceinline__ u32 room(u32 want) const { return want > (u64)(end - d) ? (u32)(end - d) : want; }
    /* "\tXX:t:" and, for a B array (k == 7), its subtype */
    __device__ __forceinline__ void head(const u8* f, u32 type, u32 k) {
        const u32 lane = (u32)lane_id();
        const u32 b = lane == 0 ? (u32)'\t' : lane == 1 ? f[0] : lane == 2 ? f[1] : lane == 4 ? type : lane == 6 ? f[3] : (u32)':';
        k = room(k);
        if (lane < k) d[lane] = (u8)b;
        d += k;
    }
    __device__ __forceinline__ void copy(const u8* src, u32 len) {
        len = room(len);
        gz_wave_copy(d, src, len);
        d += len;
    }
    /* every lane its w bytes of e at offset at; total: the wave's */
    __device__ __forceinline__ void lanes(const char* e, u32 w, u32 at, u32 total) {
        const u64 left = (u64)(end - d);
#pragma unroll
        for (u32 k = 0; k < 1 + bamcomment::SCALAR_TEXT_MAX; k++)
            if (k < w && (u64)at + k < left) d[at + k] = (u8)e[k];
        d += room(total);
    }
};

/* The comment of the tag bytes p[0, len) under the selection into `sink`: the whole wave calls it with the same arguments.
   fields / left_out: added to (wave-uniform) */
template <class Sink>
__device__ __forceinline__ void bamcomment_wave_text(const u8* __restrict__ p, u32 len, const bamcomment::Selection& sel, Sink& sink, u32& fields,
                                                     u32& left_out) {
    const u32 lane = (u32)lane_id();
    for (u32 o = 0; o < len;) { /* wave-uniform */
        u32 n = 0;
        if (lane == 0) n = (u32)bamtag::field_len(p + o, len - o, BamTagScan8());
        n = shfl_u32(n, 0);
        if (!n) break; /* (never: the tails wrote fields that parse) */
        const u8* f = p + o;
        o += n;
        if (!bamcomment::selected(sel, f)) continue;
        const u32 t = f[2];
        if (t == 'A' || t == 'Z' || t == 'H') {
            const u32 vl = t == 'A' ? 1u : n - 4;
            bool ctl = false;
            for (u32 k = lane; k < vl; k += 64) ctl = ctl || bamcomment::control_byte(f[3 + k]);
            if (wave_ballot(ctl)) {
                left_out++;
                continue;
            }
            sink.head(f, t, 6);
            sink.copy(f + 3, vl);
        } else if (t == 'B') {
            const u32 sub = f[3], sz = bamtag::scalar_size(sub), count = bamrule::rd32(f + 4);
            sink.head(f, t, 7);
            for (u32 k0 = 0; k0 < count; k0 += 64) { /* wave-uniform */
                char e[1 + bamcomment::SCALAR_TEXT_MAX];
                u32 w = 0;
                if (k0 + lane < count) {
                    e[0] = ',';
                    w = 1 + bamcomment::scalar_text(sub, f + 8 + (u64)(k0 + lane) * sz, e + 1);
                }
                const u32 incl = wave_scan_incl_u32(w);
                sink.lanes(e, w, incl - w, shfl_u32(incl, 63));
            }
        } else {
            char e[1 + bamcomment::SCALAR_TEXT_MAX];
            const u32 w = bamcomment::scalar_text(t, f + 3, e); /* (every lane alike) */
            sink.head(f, (u32)bamcomment::text_type(t), 6);
            sink.lanes(e, lane == 0 ? w : 0u, 0, w);
        }
        fields++;
    }
}

/* a wave per input record: the tag bytes of either passing fragment into scratch[f] (each buf_bytes + BAM_PAD bytes) */
__global__ void __launch_bounds__(256)
k_bam_comment_tags(const u8* __restrict__ bam, u64 buf_bytes, const uint64_t* __restrict__ rec_start, const fpl_read_result* __restrict__ res, u32 n_rec,
                   const BamTagInfo* __restrict__ info, const BamModInfo* __restrict__ minfo, const BamModPlan* __restrict__ plans,
                   u8* __restrict__ scratch0, u8* __restrict__ scratch1) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const BamModTail tail = {BamTagTail{bam, rec_start, info}, minfo, plans};
    for (u32 i = wave; i < n_rec; i += n_waves) { /* wave-uniform */
        const BamTagInfo t = info[i];
        const u64 rs = rec_start[i];
        const fpl_read_result r = res[i];
        for (int f = 0; f < 2; f++) {
            const u32 n = t.len[f];
            /* (a fragment's bytes lie inside its record's region: never past the buffer, never in the record's first four bytes) */
            if (n == 0 || t.at < 4 || rs + t.at + n > buf_bytes) continue;
            u8* d = (f ? scratch1 : scratch0) + rs + t.at;
            (void)tail(i, f, 0, r.frag_len[f], d - 4, d);
        }
    }
}

/* a wave per input record: clen[2 i + f] = the text bytes of fragment f's comment.  counters: output records that got at least
   one field, fields written, comment bytes, fields left out for control bytes */
__global__ void __launch_bounds__(256)
k_bam_comment_len(const u8* __restrict__ scratch0, const u8* __restrict__ scratch1, u64 buf_bytes, const uint64_t* __restrict__ rec_start, u32 n_rec,
                  const BamTagInfo* __restrict__ info, bamcomment::Selection sel, u64* __restrict__ clen, unsigned long long* __restrict__ counters) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    unsigned long long c[4] = {0, 0, 0, 0};
    for (u32 i = wave; i < n_rec; i += n_waves) { /* wave-uniform */
        const BamTagInfo t = info[i];
        const u64 rs = rec_start[i];
        for (int f = 0; f < 2; f++) {
            const u32 n = t.len[f];
            u64 bytes = 0;
            if (n != 0 && t.at >= 4 && rs + t.at + n <= buf_bytes) {
                BamNoteCount sink;
                u32 fields = 0, left = 0;
                bamcomment_wave_text((f ? scratch1 : scratch0) + rs + t.at, n, sel, sink, fields, left);
                bytes = sink.n;
                c[0] += fields ? 1 : 0, c[1] += fields, c[2] += bytes, c[3] += left;
            }
            if (lane_id() == 0) clen[2 * (size_t)i + f] = bytes;
        }
    }
    if (lane_id() == 0)
        for (int k = 0; k < 4; k++)
            if (c[k]) atomicAdd(&counters[k], c[k]);
}

/* the BAM source with the comments' lengths beside every record */
struct GzRecNotes : GzRec {
    u64 note_len[2];
};
struct GzBamNoteSrc : GzBamSrc {
    typedef GzRecNotes Rec;
    const u64* clen;
    __device__ __forceinline__ GzRecNotes rec(u32 r) const {
        GzRecNotes t;
        (GzRec&)t = GzBamSrc::rec(r);
        t.note_len[0] = clen[2 * (size_t)r], t.note_len[1] = clen[2 * (size_t)r + 1];
        return t;
    }
};
/* GzFastqForm with the comment in part a: behind the name */
struct GzFastqNoteForm {
    static __device__ __forceinline__ void prep(GzRec&) {}
    static __device__ __forceinline__ void frag_len(const GzRecNotes& g, const fpl_read_result& r, int f, u64& a, u64& b) {
        gz_frag_len(g, r, f, a, b);
        a += g.note_len[f];
    }
};
__global__ void __launch_bounds__(1024)
k_gz_layout_bam_comments(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                         const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const u64* __restrict__ clen,
                         u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_body<GzFastqNoteForm>(GzBamNoteSrc{{bam, rec_start, seq, qual, off}, clen}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}

/* what gz_compose_body writes behind fragment f's name: the comment, clamped to the length the layout counted */
struct GzBamNote {
    const u8* scratch0;
    const u8* scratch1;
    const uint64_t* rec_start;
    const BamTagInfo* info;
    const u64* clen;
    const bamcomment::Selection* sel;
    __device__ __forceinline__ u8* operator()(u32 i, int f, u8* d) const {
        const u64 n = clen[2 * (size_t)i + f];
        if (n == 0) return d; /* (wave-uniform) */
        const BamTagInfo t = info[i];
        BamNoteStore sink = {d, d + n};
        u32 fields = 0, left = 0;
        bamcomment_wave_text((f ? scratch1 : scratch0) + rec_start[i] + t.at, t.len[f], *sel, sink, fields, left);
        return d + n;
    }
};
__global__ void __launch_bounds__(256)
k_gz_compose_bam_comments(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                          const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const BamTagInfo* __restrict__ info,
                          const u8* __restrict__ scratch0, const u8* __restrict__ scratch1, const u64* __restrict__ clen, bamcomment::Selection sel,
                          const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    gz_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap,
                    GzBamNote{scratch0, scratch1, rec_start, info, clen, &sel});
}

}  // namespace fpl
#endif
