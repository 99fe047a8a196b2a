/*
 * bam_emit.h -- the passing reads of a TEXT batch or a BAM batch as unaligned BAM RECORDS in BGZF blocks, composed ON THE DEVICE
 * (fpl_set_gzip_records; include/fastplong_amd.h).  The rules of a record are csrc/bam_out_rules.h's, shared with the host's
 * converter (host/bam_out.cpp); what comes out inflates to what fastq_to_bam_records makes of the host's formatted text.
 *
 * The same two record sources as gz_emit.h (GzTextSrc, GzBamSrc), the same single-block layout body with another form of the
 * composed bytes (BamRecForm in place of GzFastqForm), a compose kernel of its own, and then gz_emit.h's four block kernels in
 * their BGZF framing, unchanged: they are literal-only Huffman coders and do not care whether the bytes are text.
 *
 *   k_bamout_layout    one block, lane = read: the name cut (first space or tab, at most 254 bytes with the split prefix), the
 *                      record lengths 36 + name + 1 + (fl + 1) / 2 + fl, their prefix sums, and where deflate blocks start: at
 *                      every multiple of GZ_B, and for a fragment with fl + 1 >= GZ_L at its record's first byte and at its
 *                      first quality byte, so packed bases and qualities get tables of their own
 *   k_bamout_compose   a wave per record: lanes write the 36 fixed bytes and the name; a lane packs 32 bases (two unaligned
 *                      16-byte loads, codes out of a 256-byte LDS copy of the shared table) into one 16-byte store and takes 33
 *                      off 16 qualities; ragged ends byte by byte, a lane each.  Nothing outside [rec_off[i], rec_off[i + 1]).
 * k_bamout_layout_bam / k_bamout_compose_bam: the BAM-source forms (the decoded arrays: ASCII, already the twin's orientation).
 *
 * 1.5 bytes per base are written where the FASTQ form writes 2, so the block kernels see a quarter fewer bytes; a SHORT record is
 * longer than its text (36 fixed bytes against the 6 of '@', '+' and four line ends): bounds of its own below.
 */
#ifndef FPL_BAM_EMIT_H
#define FPL_BAM_EMIT_H

#include "bam_out_rules.h"
#include "gz_emit.h"

namespace fpl {

/* Worst case of one BGZF block of records: the smallest record with forced cuts has GZ_L - 1 bases and a one-byte name, 36 + 2 +
   512 + 1 023 = 1 573 bytes, so a stripe holds at most 3 + 2 * ceil(49 152 / 1 573) + 1 = 68 deflate blocks (its three multiples of
   GZ_B, two forced starts per such record, one for what is left of a record that began in the stripe before), each grows by at
   most GZ_SLACK: 49 152 + 5 * 68 + 31 = 49 523 bytes, far inside BGZF's 65 536. */
constexpr u32 BAMOUT_MIN_FORCED = bamout::FIXED + 2 + GZ_L / 2 + (GZ_L - 1);
static_assert(GZ_STRIPE + GZ_SLACK * (3 + 2 * ((GZ_STRIPE + BAMOUT_MIN_FORCED - 1) / BAMOUT_MIN_FORCED) + 1) + GZ_BGZF_EXTRA <= GZ_BGZF_MAX,
              "a stripe of BAM records must fit a BGZF block in its worst case");
/* most bytes of the records of a text chunk / of a BAM batch: the fragments of a read are pieces of it (1.5 bytes a base, rounded
   up), and each of a read's two fragments writes 36 fixed bytes, a name of at most 254 and its NUL */
constexpr u64 BAMOUT_PER_FRAG = bamout::FIXED + bamout::NAME_BYTES + 1 + 1;
inline u64 bamout_total_bound(u64 text_bytes, u64 n_rec) { return 2 * text_bytes + 2 * BAMOUT_PER_FRAG * n_rec; }
inline u64 bamout_blocks_bound(u64 text_bytes, u64 n_rec) { return bamout_total_bound(text_bytes, n_rec) / GZ_B + 2 + 4 * n_rec; }
inline u64 bamout_bam_total_bound(u64 n_bases, u64 n_rec) { return 2 * n_bases + 2 * BAMOUT_PER_FRAG * n_rec; }
inline u64 bamout_bam_blocks_bound(u64 n_bases, u64 n_rec) { return bamout_bam_total_bound(n_bases, n_rec) / GZ_B + 2 + 4 * n_rec; }

/* bytes of rest in front of its first space or tab, NAME_BYTES at the most; eight bytes a step while eight are left */
__device__ __forceinline__ u32 bamout_name_scan(const u8* __restrict__ rest, u32 rest_len) {
    const u32 cap = rest_len < bamout::NAME_BYTES ? rest_len : bamout::NAME_BYTES;
    u32 n = 0;
    for (; n + 8 <= cap; n += 8) {
        u64 w;
        __builtin_memcpy(&w, rest + n, 8);
        const u64 s = w ^ 0x2020202020202020ull, t = w ^ 0x0909090909090909ull;
        const u64 z = (((s - 0x0101010101010101ull) & ~s) | ((t - 0x0101010101010101ull) & ~t)) & 0x8080808080808080ull;
        if (z) return n + ((u32)__builtin_ctzll(z) >> 3); /* (the lowest flagged byte is always a true one) */
    }
    while (n < cap && !bamout::name_ends(rest[n])) n++;
    return n;
}
/* the same for a whole wave that looks at one name: four bytes a lane */
__device__ __forceinline__ u32 bamout_name_scan_wave(const u8* __restrict__ rest, u32 rest_len) {
    const u32 cap = rest_len < bamout::NAME_BYTES ? rest_len : bamout::NAME_BYTES;
    const u32 at = 4u * (u32)lane_id();
    u32 hit = 4;
    for (u32 k = 0; k < 4; k++)
        if (hit == 4 && at + k < cap && bamout::name_ends(rest[at + k])) hit = k;
    const u64 any = wave_ballot(hit < 4);
    if (!any) return cap;
    const int first = __builtin_ctzll(any);
    return 4u * (u32)first + shfl_u32(hit, first);
}

/* The records' form of the composed bytes.  prep: the name line cut ONCE per record -- name_len becomes the '@' and the bytes in
   front of the first space or tab, so that gz_prefix_len keeps its meaning (an empty line gets no prefix). */
struct BamRecForm {
    static __device__ __forceinline__ void prep(GzRec& g) {
        if (g.name_len) g.name_len = 1u + bamout_name_scan(g.name_rest, g.name_len - 1u);
    }
    static __device__ __forceinline__ void prep_wave(GzRec& g) { /* (wave-uniform) */
        if (g.name_len) g.name_len = 1u + bamout_name_scan_wave(g.name_rest, g.name_len - 1u);
    }
    /* fragment of kind `kind`: bytes of the prefix, bytes of the name behind it */
    static __device__ __forceinline__ void name_parts(const GzRec& g, u32 kind, u32& pl, u32& cut) {
        pl = gz_prefix_len(kind, g.name_len);
        const u32 rest = g.name_len ? g.name_len - 1u : 0u, room = bamout::name_room(pl);
        cut = rest < room ? rest : room;
    }
    /* a: fixed bytes, name, NUL, packed bases; b: qualities */
    static __device__ __forceinline__ void frag_len(const GzRec& g, const fpl_read_result& r, int f, u64& a, u64& b) {
        u32 pl, cut;
        name_parts(g, r.kind[f], pl, cut);
        const u64 fl = r.frag_len[f];
        b = fl;
        a = bamout::record_len(bamout::name_len(pl, cut), fl) - fl;
    }
};

__global__ void __launch_bounds__(1024)
k_bamout_layout(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
                const fpl_read_result* __restrict__ res, u32 n_rec, u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap,
                GzHeader* __restrict__ hdr) {
    gz_layout_body<BamRecForm>(GzTextSrc{text, line, nl_pos}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}
__global__ void __launch_bounds__(1024)
k_bamout_layout_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                    const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, u64* __restrict__ rec_off,
                    u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_body<BamRecForm>(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}

/* four bases -> two bytes, high nibble first */
__device__ __forceinline__ u32 bamout_pack4(const u8* tab, u32 w) {
    const u32 lo = ((u32)tab[w & 255u] << 4) | tab[(w >> 8) & 255u], hi = ((u32)tab[(w >> 16) & 255u] << 4) | tab[w >> 24];
    return lo | (hi << 8);
}
/* fl bases -> (fl + 1) / 2 bytes, the wave together; neither side is aligned.  A lane takes 32 bases; what is left behind the
   last whole 32 is at most 16 bytes, a lane each, and the last of them has a low nibble of 0 when fl is odd */
__device__ __forceinline__ void bamout_wave_pack(u8* __restrict__ dst, const u8* __restrict__ src, u32 fl, const u8* tab) {
    const u32 lane = (u32)lane_id();
    const u32 whole = fl & ~31u;
    for (u32 i = 32 * lane; i < whole; i += 32 * 64) {
        const u32x4 a = load16(src + i), b = load16(src + i + 16);
        u32x4 o;
        o.x = bamout_pack4(tab, a.x) | (bamout_pack4(tab, a.y) << 16);
        o.y = bamout_pack4(tab, a.z) | (bamout_pack4(tab, a.w) << 16);
        o.z = bamout_pack4(tab, b.x) | (bamout_pack4(tab, b.y) << 16);
        o.w = bamout_pack4(tab, b.z) | (bamout_pack4(tab, b.w) << 16);
        __builtin_memcpy(dst + i / 2, &o, 16);
    }
    const u32 left = fl - whole;
    if (lane < (left + 1) / 2) {
        const u32 hi = tab[src[whole + 2 * lane]], lo = 2 * lane + 1 < left ? tab[src[whole + 2 * lane + 1]] : 0u;
        dst[whole / 2 + lane] = (u8)((hi << 4) | lo);
    }
}
__device__ __forceinline__ u32 bamout_qual4(u32 w) {
    return bamout::qual_code(w & 255u) | (bamout::qual_code((w >> 8) & 255u) << 8) | (bamout::qual_code((w >> 16) & 255u) << 16) |
           (bamout::qual_code(w >> 24) << 24);
}
/* fl quality bytes, 33 taken off (what is below 33 gives 0); 16 bytes a lane */
__device__ __forceinline__ void bamout_wave_quals(u8* __restrict__ dst, const u8* __restrict__ src, u32 fl) {
    const u32 lane = (u32)lane_id();
    const u32 whole = fl & ~15u;
    for (u32 i = 16 * lane; i < whole; i += 16 * 64) {
        u32x4 v = load16(src + i);
        v.x = bamout_qual4(v.x), v.y = bamout_qual4(v.y), v.z = bamout_qual4(v.z), v.w = bamout_qual4(v.w);
        __builtin_memcpy(dst + i, &v, 16);
    }
    if (lane < (fl & 15u)) dst[whole + lane] = (u8)bamout::qual_code(src[whole + lane]);
}

/* what a record gets behind its qualities: nothing (csrc/bam_tags.h has the tail that appends auxiliary fields) */
struct BamNoTail {
    __device__ __forceinline__ u8* operator()(u32, int, u32, u32, u8*, u8* d) const { return d; }
};
/* a wave per record; comp holds hdr->total bytes (the caller sized it after the layout: comp_cap is checked all the same).
   blockDim.x is 256: a thread fills one entry of the block's copy of the base table.
   tail(read, fragment, name bytes, bases, the record's first byte, its end so far) -> the record's end */
template <class Src, class Tail = BamNoTail>
__device__ __forceinline__ void bamout_compose_body(const Src& src, const fpl_read_result* __restrict__ res, u32 n_rec,
                                                    const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap,
                                                    const Tail& tail = Tail()) {
    __shared__ u8 tab[256];
    tab[threadIdx.x & 255u] = (u8)bamout::base_code(threadIdx.x & 255u);
    __syncthreads();
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    for (u32 i = wave; i < n_rec; i += n_waves) { /* wave-uniform */
        const u64 o0 = rec_off[i], o1 = rec_off[i + 1];
        if (o1 == o0 || o1 > comp_cap) continue;
        GzRec g = src.rec_wave(i);
        BamRecForm::prep_wave(g);
        const fpl_read_result r = res[i];
        u8* d = comp + o0;
        for (int f = 0; f < r.n_frag && f < 2; f++) {
            if (r.code[f] != FPL_PASS_FILTER) continue;
            u32 pl, cut;
            BamRecForm::name_parts(g, r.kind[f], pl, cut);
            const u32 nl = bamout::name_len(pl, cut);
            const u32 fl = r.frag_len[f], fs = r.frag_start[f];
            if (lane < bamout::FIXED) d[lane] = (u8)(bamout::fixed_word(lane >> 2, nl, fl) >> (8u * (lane & 3u)));
            u8* nm = d + bamout::FIXED;
            if (pl + cut == 0) { /* (wave-uniform) what is left empty */
                if (lane == 0) nm[0] = (u8)'*';
            } else {
                if (lane < pl) {
                    const char* pf = pl == 22 ? "split-by-adapter-left-" : "split-by-adapter-right-";
                    nm[lane] = (u8)pf[lane];
                }
                gz_wave_copy(nm + pl, g.name_rest, cut);
            }
            if (lane == 0) nm[nl] = 0;
            u8* pk = nm + nl + 1;
            bamout_wave_pack(pk, g.seq + fs, fl, tab);
            u8* q = pk + ((u64)fl + 1) / 2;
            bamout_wave_quals(q, g.qual + fs, fl);
            d = tail(i, f, nl, fl, d, q + fl);
        }
    }
}
__global__ void __launch_bounds__(256)
k_bamout_compose(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
                 const fpl_read_result* __restrict__ res, u32 n_rec, const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    bamout_compose_body(GzTextSrc{text, line, nl_pos}, res, n_rec, rec_off, comp, comp_cap);
}
__global__ void __launch_bounds__(256)
k_bamout_compose_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                     const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const u64* __restrict__ rec_off,
                     u8* __restrict__ comp, u64 comp_cap) {
    bamout_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap);
}

}  // namespace fpl
#endif
