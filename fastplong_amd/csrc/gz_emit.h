/*
 * gz_emit.h -- the passing reads of a TEXT batch or a BAM batch as gzip members, composed and Huffman-coded ON THE DEVICE
 * (fpl_set_text_gzip / fpl_wait_text_gz, fpl_set_bam_gzip / fpl_wait_bam_gz, include/fastplong_amd.h).
 *
 * Input: the per-read records and a record source -- the chunk's text with where its lines start and end (text_parse.h: line[],
 * nl_pos[]: GzTextSrc), or a BAM batch's record bytes, record starts, decoded bases / qualities and CSR offsets (bam_decode.h:
 * GzBamSrc).  k_gz_layout / k_gz_compose are the text forms and k_gz_layout_bam / k_gz_compose_bam the BAM forms of ONE body each,
 * templated on the source, so the cuts and the length arithmetic exist once.  Output: one
 * gzip member (RFC 1952) whose inflation is exactly what fplh::format_batch (host/format.cpp, format_range without a fragment
 * list) appends for that batch; nothing at all when no read passed.  Long-read FASTQ has next to nothing for LZ77 to find, so the
 * deflate stream holds literals only: the gain is the entropy code, and blocks are cut so that bases and qualities -- which share
 * byte values -- mostly get tables of their own.
 *
 *   k_gz_layout   one block, lane = read: output length of every record, exclusive prefix sums, and where deflate blocks START:
 *                 at every multiple of GZ_B of the output, and for a fragment whose bases line has at least GZ_L bytes at its
 *                 name line and at its '+' line (so [name + bases] and ['+' + qualities] are blocks of their own; what follows a
 *                 long fragment joins its quality block up to the next multiple of GZ_B).  No block is longer than GZ_B.
 *   k_gz_compose  a wave per record: the pieces to their offsets, 16 bytes a lane where the lengths allow
 *   k_gz_block    a workgroup per deflate block: the bytes into LDS, a 257-bin histogram, the raw CRC of the block, code lengths
 *                 limited to 15 bits (Moffat-Katajainen on the sorted counts, then a Kraft repair on the counts per length),
 *                 canonical codes, the dynamic header (code-length code limited to 7 bits, zero runs as symbols 17 / 18, one
 *                 distance code), and the pack: every thread owns GZ_STRETCH symbols, a prefix sum of their bits says where its
 *                 codes go, words inside its range are stored, the two at its ends merged with LDS atomics.  A block ends with an
 *                 empty stored block that byte-aligns it (what pigz does), so blocks are independent; a block that would not get
 *                 smaller is one stored block.  The result goes to a slot of its own: at most its length + GZ_SLACK bytes.
 *   k_gz_finish   one block: prefix sums of the blocks' sizes, the member's CRC-32 folded from the blocks' (every block's raw
 *                 remainder times x^(8 * bytes behind it) mod P: no order between blocks), the gzip header, the final empty
 *                 block and the trailer
 *   k_gz_compact  a workgroup per deflate block: its bytes to their place in the member
 *
 * Worst case: gz_len <= GZ_MEMBER_EXTRA + total + GZ_SLACK * n_blocks, n_blocks <= total / GZ_B + 1 + 2 * (long fragments).
 *
 * The BGZF form (fpl_set_gzip_framing): the same layout and compose; the text in stripes of GZ_STRIPE bytes, one BGZF block each
 *   k_gz_block_bgzf   k_gz_block's body with two distance code lengths in the dynamic header (a complete set) and the block's CRC
 *                     remainder shifted to the end of its stripe
 *   k_gz_finish_bgzf  one block: the same prefix sums, every block placed behind the frames in front of it; the batch's CRC-32
 *   k_gz_frame        a thread per stripe: header with BSIZE, final empty block, CRC-32 and ISIZE of the stripe
 *   k_gz_compact      unchanged
 * Worst case: gz_len <= total + GZ_SLACK * n_blocks + GZ_BGZF_EXTRA * ceil(total / GZ_STRIPE) (beside GZ_STRIPE below).
 *
 * The fragment forms (fpl_set_fragment_output): a context with break_enabled / mask_enabled writes from its fragment list, whose
 * order frag_index.h makes on the device.  k_gz_layout_frag[_bam] / k_gz_compose_frag[_bam] run the same scan, the same cuts and
 * the same wave copy with a lane / a wave per ordered FRAGMENT; the bytes are format_range's with a fragment list ("r<i>-" in the
 * name, the fragment's regions as N).  Everything from k_gz_block on runs unchanged.
 *
 * The layout body is also templated on the FORM of the composed bytes (GzFastqForm here); csrc/bam_emit.h has the form of unaligned
 * BAM records (fpl_set_gzip_records), a compose kernel of its own, and runs the BGZF block kernels on what it composes.
 */
#ifndef FPL_GZ_EMIT_H
#define FPL_GZ_EMIT_H

#include "../../include/fastplong_amd.h"
#include "dev_prims.h"
#include "frag_index.h"

namespace fpl {

typedef uint16_t u16;
constexpr u32 GZ_B = 16384;  /* most bytes of a deflate block (docs/kernels.md: the table behind GZ_B and GZ_L) */
constexpr u32 GZ_L = 1024;   /* a bases line of at least this many bytes starts blocks of its own */
constexpr int GZ_THREADS = 256;
constexpr u32 GZ_STRETCH = GZ_B / GZ_THREADS; /* symbols a thread packs */
constexpr u32 GZ_SLACK = 5;                   /* a stored block's header: the most a block grows by */
constexpr u32 GZ_MEMBER_EXTRA = 10 + 5 + 8;   /* gzip header, final empty block, CRC-32 + ISIZE */
/* The BGZF form (fpl_set_gzip_framing): BGZF block k of a batch holds bytes [k * GZ_STRIPE, min((k + 1) * GZ_STRIPE, total)) of the
   composed text.  Every multiple of GZ_B starts a deflate block, so a stripe is a whole number of the deflate blocks the layout
   cuts, whatever their compressed sizes.  Worst case of one BGZF block: a stripe holds at most 3 + 2 * ceil(49 152 / 2 050) + 1 =
   52 deflate blocks (its three multiples of GZ_B, two forced starts per fragment of at least GZ_L - 1 bases -- such a fragment
   writes at least 2 * (GZ_L - 1) + 4 = 2 050 bytes --, one for what is left of a fragment that began in the stripe before), each
   grows by at most GZ_SLACK, so the block stays below 49 152 + 5 * 53 + 31 = 49 448 bytes: far inside BGZF's 65 536.
   The fragment forms (k_gz_layout_frag) keep the bound: their forced cuts come from the same rule (gz_frag_cuts), so a forced cut
   still needs a fragment of at least GZ_L - 1 bases -- 2 050 bytes of output and more, the "r<i>-" of its name besides. */
constexpr u32 GZ_STRIPE = 3 * GZ_B;
constexpr u32 GZ_BGZF_HEAD = 18;                       /* gzip header with the BC extra field */
constexpr u32 GZ_BGZF_EXTRA = GZ_BGZF_HEAD + 5 + 8;    /* header, final empty block, CRC-32 + ISIZE: per BGZF block */
constexpr u32 GZ_BGZF_MAX = 65536;
static_assert(GZ_STRIPE % GZ_B == 0 && GZ_STRIPE + GZ_SLACK * (3 + 2 * ((GZ_STRIPE + 2 * GZ_L + 1) / (2 * GZ_L + 2)) + 2) + GZ_BGZF_EXTRA <= GZ_BGZF_MAX,
              "a stripe's worst case must fit a BGZF block");
constexpr u32 GZ_CRC_POLY = 0xEDB88320u;
constexpr int GZ_NSYM = 257; /* 256 literals + end-of-block */

struct GzHeader {
    u64 total;    /* bytes of the composed text */
    u64 gz_len;   /* bytes of the member, or of the batch's BGZF blocks together (0 when total is 0) */
    u32 n_blocks; /* deflate blocks with data */
    u32 status;   /* bit 0: more blocks than the caller's arrays hold (nothing usable) */
    u32 crc;      /* CRC-32 of the composed text */
    u32 pad;
};

/* most deflate blocks a chunk of text_bytes bytes and n_rec records can be cut into (both fragments of a split read repeat the
   name and the '+' line, and each may start two blocks) */
/* the output bound of either form: what the buffers are sized by */
inline u64 gz_bgzf_blocks(u64 total) { return (total + GZ_STRIPE - 1) / GZ_STRIPE; }
inline u64 gz_out_bound(u64 total, u64 n_blocks, bool bgzf) {
    return total + (u64)GZ_SLACK * n_blocks + (bgzf ? (u64)GZ_BGZF_EXTRA * gz_bgzf_blocks(total) : (u64)GZ_MEMBER_EXTRA);
}
inline u64 gz_total_bound(u64 text_bytes, u64 n_rec) { return 2 * text_bytes + 46 * n_rec; }
inline u64 gz_blocks_bound(u64 text_bytes, u64 n_rec) { return gz_total_bound(text_bytes, n_rec) / GZ_B + 2 + 4 * n_rec; }
/* the same for a BAM batch of n_bases bases: a fragment is at most its read, and writes a name line of at most 1 + 254 + 23 bytes,
   the '+' line and four line ends besides its bases and qualities */
inline u64 gz_bam_total_bound(u64 n_bases, u64 n_rec) { return 4 * n_bases + 2 * (255 + 23 + 6) * n_rec; }
inline u64 gz_bam_blocks_bound(u64 n_bases, u64 n_rec) { return gz_bam_total_bound(n_bases, n_rec) / GZ_B + 2 + 4 * n_rec; }
/* the fragment forms (fpl_set_fragment_output): a read's name is written once per fragment, so the bounds above do not hold.  By
   the capacity of the fragment list (break_mask_caps, which the host knows without asking the device): the fragments of a read
   are disjoint windows of it, every fragment writes its name line (1 + 7 + 23 + the name), the '+' line and four line ends -- 320
   bytes cover a BAM's 254-byte name; a text batch whose name and '+' lines are longer than that on the average of its fragments
   runs out of block slots, which is a status of the layout --, and only a fragment of at least GZ_L - 1 bases forces cuts */
inline u64 gz_frag_total_bound(u64 n_bases, u64 frag_cap) { return 2 * n_bases + 320 * frag_cap; }
inline u64 gz_frag_blocks_bound(u64 n_bases, u64 frag_cap) {
    const u64 forced = n_bases / (GZ_L - 1);
    return gz_frag_total_bound(n_bases, frag_cap) / GZ_B + 2 + 2 * (forced < frag_cap ? forced : frag_cap);
}

/* ---- CRC-32 arithmetic (reflected: bit 31 is x^0) ---- */
__device__ __forceinline__ u32 gz_mulmod(u32 a, u32 b) { /* a * b mod P */
    u32 p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? GZ_CRC_POLY : 0u);
    }
    return p;
}
__device__ __forceinline__ u32 gz_xpow8(u64 n) { /* x^(8 n) mod P */
    u32 r = 0x80000000u, sq = 0x00800000u; /* x^0, x^8 */
    while (n) {
        if (n & 1ull) r = gz_mulmod(r, sq);
        sq = gz_mulmod(sq, sq);
        n >>= 1;
    }
    return r;
}
/* where the stripe of byte `at` ends: the next multiple of GZ_STRIPE, or the end of the text */
__device__ __forceinline__ u64 gz_stripe_end(u64 at, u64 total) {
    const u64 e = (at / GZ_STRIPE + 1) * (u64)GZ_STRIPE;
    return e < total ? e : total;
}
__device__ __forceinline__ u32 gz_crc_table_entry(u32 i) {
    u32 c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? GZ_CRC_POLY : 0u);
    return c;
}

/* ---- what a read writes ---- */
/* The pieces of one record, whatever the batch came in as.  The name line is `lead`, the prefix of a split read, and the
   name_len - 1 bytes at name_rest; name_len counts the lead (0: an empty line, nothing is written).  strand == nullptr says the
   '+' line is the one byte '+'.  seq / qual are the read's first base and quality: pointers, so a batch may pass 4 GiB. */
struct GzRec {
    const u8* name_rest;
    const u8* strand;
    const u8* seq;
    const u8* qual;
    u32 name_len, strand_len;
    u8 lead;
};
__device__ __forceinline__ u32 gz_line_len(const u8* __restrict__ text, u32 at, u32 nl) {
    u32 e = nl; /* the '\n' */
    if (e > at && text[e - 1] == '\r') e--;
    return e - at;
}
/* where the records come from: a type with rec(r).  The layout and compose kernels are templated on it, so that the cuts and the
   length arithmetic exist once. */
/* a TEXT batch: the chunk's text through the line starts and line ends text_parse.h found */
struct GzTextSrc {
    typedef GzRec Rec; /* (what rec() gives: a source may hand out more than the pieces -- csrc/bam_tags.h) */
    const u8* text;
    const u32* line;
    const u32* nl_pos;
    __device__ __forceinline__ GzRec rec(u32 r) const {
        GzRec g;
        const u32 name_at = line[4 * (size_t)r], strand_at = line[4 * (size_t)r + 2];
        g.seq = text + line[4 * (size_t)r + 1];
        g.qual = text + line[4 * (size_t)r + 3];
        g.name_len = gz_line_len(text, name_at, nl_pos[4 * (size_t)r]);
        g.strand_len = gz_line_len(text, strand_at, nl_pos[4 * (size_t)r + 2]);
        g.lead = g.name_len ? text[name_at] : (u8)0;
        g.name_rest = text + name_at + 1;
        g.strand = text + strand_at;
        return g;
    }
    /* the same for a whole wave that asks for one record (k_gz_compose) */
    __device__ __forceinline__ GzRec rec_wave(u32 r) const { return rec(r); }
};
/* a BAM batch (bam_decode.h): the name out of the record -- '@' and the l_read_name - 1 bytes at record + 36, so the line is never
   empty --, the bases and qualities out of the decoded arrays (already the twin's: reversed for flag 0x10, min(q, 93) + 33) */
struct GzBamSrc {
    typedef GzRec Rec;
    const u8* bam;
    const uint64_t* rec_start;
    const u8* seq;
    const u8* qual;
    const uint64_t* off;
    /* the name ends at its first NUL, as the host's reader takes it (host/bam.cpp): l_read_name - 1 bytes in every BAM that keeps
       to the format; 8 bytes a step (the record buffer holds BAM_PAD bytes behind its end) */
    static __device__ __forceinline__ u32 name_bytes(const u8* rc) {
        const u32 cap = rc[12] ? rc[12] - 1u : 0u;
        u32 nl = 0;
        for (; nl < cap; nl += 8) {
            u64 w;
            __builtin_memcpy(&w, rc + 36 + nl, 8);
            const u64 z = (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull;
            if (z) {
                nl += (u32)__builtin_ctzll(z) >> 3;
                break;
            }
        }
        return nl < cap ? nl : cap;
    }
    __device__ __forceinline__ GzRec rec(u32 r) const { return make(r, name_bytes(bam + rec_start[r])); }
    /* a whole wave asks for one record: lane 0 walks the name, the others take its answer */
    __device__ __forceinline__ GzRec rec_wave(u32 r) const {
        u32 nl = 0;
        if (lane_id() == 0) nl = name_bytes(bam + rec_start[r]);
        return make(r, shfl_u32(nl, 0));
    }
    __device__ __forceinline__ GzRec make(u32 r, u32 nl) const {
        GzRec g;
        const u8* rc = bam + rec_start[r];
        g.name_len = 1u + nl; /* (the '@' is always there: a BAM name line is never empty) */
        g.lead = (u8)'@';
        g.name_rest = rc + 36;
        g.strand = nullptr;
        g.strand_len = 1;
        g.seq = seq + off[r];
        g.qual = qual + off[r];
        return g;
    }
};
__device__ __forceinline__ u32 gz_prefix_len(u32 kind, u32 name_len) { /* "split-by-adapter-left-" / "split-by-adapter-right-" */
    return name_len == 0 ? 0u : (kind == 1 ? 22u : (kind == 2 ? 23u : 0u));
}
/* bytes of fragment f's name + bases lines (a) and of its '+' + quality lines (b) */
__device__ __forceinline__ void gz_frag_len(const GzRec& g, const fpl_read_result& r, int f, u64& a, u64& b) {
    a = (u64)g.name_len + gz_prefix_len(r.kind[f], g.name_len) + 1 + (u64)r.frag_len[f] + 1;
    b = (u64)g.strand_len + 1 + (u64)r.frag_len[f] + 1;
}
/* the form of the composed bytes: what a fragment writes in front of its second forced cut (a) and behind it (b).  FASTQ text here;
   csrc/bam_emit.h has the BAM records' form.  prep: once per record, before the lengths are asked for. */
struct GzFastqForm {
    static __device__ __forceinline__ void prep(GzRec&) {}
    static __device__ __forceinline__ void frag_len(const GzRec& g, const fpl_read_result& r, int f, u64& a, u64& b) { gz_frag_len(g, r, f, a, b); }
};
/* the block starts inside [s, e): s itself when forced or on a multiple of GZ_B, and every multiple of GZ_B behind it */
template <class F>
__device__ __forceinline__ void gz_cuts(u64 s, u64 e, bool force, F&& emit) {
    if (e <= s) return;
    if (force || s % GZ_B == 0) emit(s);
    for (u64 m = (s / GZ_B + 1) * GZ_B; m < e; m += GZ_B) emit(m);
}
/* the block starts of one output read at o: a bytes of name + bases, b bytes of '+' + qualities.  THE forced-cut rule: a bases
   line of at least GZ_L bytes (its line end counted) starts a block at its name line and another at its '+' line */
template <class F>
__device__ __forceinline__ void gz_frag_cuts(u64 o, u64 a, u64 b, u32 bases, F&& emit) {
    if ((u64)bases + 1 >= GZ_L) {
        gz_cuts(o, o + a, true, emit);
        gz_cuts(o + a, o + a + b, true, emit);
    } else {
        gz_cuts(o, o + a + b, false, emit);
    }
}
template <class Form = GzFastqForm, class Rec, class F>
__device__ __forceinline__ void gz_read_cuts(const Rec& g, const fpl_read_result& r, u64 o, F&& emit) {
    if (r.dropped) return;
    for (int f = 0; f < r.n_frag && f < 2; f++) {
        if (r.code[f] != FPL_PASS_FILTER) continue;
        u64 a, b;
        Form::frag_len(g, r, f, a, b);
        gz_frag_cuts(o, a, b, r.frag_len[f], emit);
        o += a + b;
    }
}

__device__ __forceinline__ u64 gz_scan_incl_u64(u64 v) {
    u64 incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = shfl_u64(incl, lane_id() - d < 0 ? lane_id() : lane_id() - d);
        if (lane_id() >= d) incl += up;
    }
    return incl;
}

/* What a lane of the layout is: a record of the batch (GzReadItem) or, with fpl_set_fragment_output, one ordered fragment of its
   --break / --mask list (GzFragItem below).  load(i): what the lane keeps; len(): the bytes it writes; cuts(): its block starts. */
template <class Form, class Src>
struct GzReadItem {
    Src src;
    const fpl_read_result* res;
    struct State {
        typename Src::Rec g;
        fpl_read_result r;
    };
    __device__ __forceinline__ State load(u32 i) const {
        State s;
        s.g = src.rec(i);
        Form::prep(s.g);
        s.r = res[i];
        return s;
    }
    __device__ __forceinline__ u64 len(const State& s) const {
        u64 len = 0;
        if (!s.r.dropped)
            for (int f = 0; f < s.r.n_frag && f < 2; f++)
                if (s.r.code[f] == FPL_PASS_FILTER) {
                    u64 a, b;
                    Form::frag_len(s.g, s.r, f, a, b);
                    len += a + b;
                }
        return len;
    }
    template <class F>
    __device__ __forceinline__ void cuts(const State& s, u64 o, F&& emit) const { gz_read_cuts<Form>(s.g, s.r, o, emit); }
};

/* one block.  rec_off[i] = where item i's output starts (n + 1 entries), blk_start[b] = where deflate block b starts
   (n_blocks + 1 entries, the last one the total) */
template <class Item>
__device__ __forceinline__ void gz_layout_scan(const Item& it, u32 n, u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap,
                                               GzHeader* __restrict__ hdr) {
    __shared__ u64 wsum[16];
    __shared__ u64 carry_len, carry_blk;
    if (threadIdx.x == 0) carry_len = 0, carry_blk = 0;
    __syncthreads();
    for (u32 base = 0; base < n; base += 1024) { /* block-uniform */
        const u32 i = base + threadIdx.x;
        typename Item::State s = {};
        u64 len = 0;
        if (i < n) {
            s = it.load(i);
            len = it.len(s);
        }
        u64 incl = gz_scan_incl_u64(len);
        if (lane_id() == 63) wsum[wave_in_block()] = incl;
        __syncthreads();
        u64 o = carry_len + incl - len;
        for (int k = 0; k < wave_in_block(); k++) o += wsum[k];
        if (i < n) rec_off[i] = o;
        __syncthreads();
        if (threadIdx.x == 1023) carry_len = o + len;
        /* the blocks that start inside this item */
        u64 cnt = 0;
        if (i < n) it.cuts(s, o, [&](u64) { cnt++; });
        incl = gz_scan_incl_u64(cnt);
        if (lane_id() == 63) wsum[wave_in_block()] = incl;
        __syncthreads();
        u64 k0 = carry_blk + incl - cnt;
        for (int k = 0; k < wave_in_block(); k++) k0 += wsum[k];
        if (i < n) {
            u64 k = k0;
            it.cuts(s, o, [&](u64 p) {
                if (k < blk_cap) blk_start[k] = p;
                k++;
            });
        }
        __syncthreads();
        if (threadIdx.x == 1023) carry_blk = k0 + cnt;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rec_off[n] = carry_len;
        hdr->total = carry_len;
        hdr->gz_len = 0;
        hdr->crc = 0;
        hdr->pad = 0;
        if (carry_blk < blk_cap) {
            blk_start[carry_blk] = carry_len;
            hdr->n_blocks = (u32)carry_blk;
            hdr->status = 0;
        } else {
            hdr->n_blocks = 0;
            hdr->status = 1;
        }
    }
}
template <class Form = GzFastqForm, class Src>
__device__ __forceinline__ void gz_layout_body(const Src& src, const fpl_read_result* __restrict__ res, u32 n_rec, u64* __restrict__ rec_off,
                                               u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_scan(GzReadItem<Form, Src>{src, res}, n_rec, rec_off, blk_start, blk_cap, hdr);
}

__global__ void __launch_bounds__(1024)
k_gz_layout(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
            const fpl_read_result* __restrict__ res, u32 n_rec, u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap,
            GzHeader* __restrict__ hdr) {
    gz_layout_body(GzTextSrc{text, line, nl_pos}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}
/* the BAM form: the slot of a batch fpl_process_bam_async decoded */
__global__ void __launch_bounds__(1024)
k_gz_layout_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, u64* __restrict__ rec_off,
                u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, blk_start, blk_cap, hdr);
}

/* len bytes, the wave together; neither side is aligned */
__device__ __forceinline__ void gz_wave_copy(u8* __restrict__ dst, const u8* __restrict__ src, u32 len) {
    const u32 lane = (u32)lane_id();
    const u32 whole = len & ~15u;
    for (u32 i = 16 * lane; i < whole; i += 16 * 64) {
        u32x4 v;
        __builtin_memcpy(&v, src + i, 16);
        __builtin_memcpy(dst + i, &v, 16);
    }
    if (lane < (len & 15u)) dst[whole + lane] = src[whole + lane];
}

/* what gz_compose_body writes behind fragment f's name, in front of the line's end (the whole wave calls it) -> where the line ends.
   Nothing here; csrc/bam_comments.h has the form that writes a BAM record's fields as a comment */
struct GzNoNote {
    __device__ __forceinline__ u8* operator()(u32, int, u8* d) const { return d; }
};
/* a wave per record; comp holds hdr->total bytes (the caller sized it after k_gz_layout: comp_cap is checked all the same) */
template <class Src, class Note = GzNoNote>
__device__ __forceinline__ void gz_compose_body(const Src& src, const fpl_read_result* __restrict__ res, u32 n_rec,
                                                const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap, const Note& note = Note()) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    for (u32 i = wave; i < n_rec; i += n_waves) { /* wave-uniform */
        const u64 o0 = rec_off[i], o1 = rec_off[i + 1];
        if (o1 == o0 || o1 > comp_cap) continue;
        const GzRec g = src.rec_wave(i);
        const fpl_read_result r = res[i];
        u8* d = comp + o0;
        for (int f = 0; f < r.n_frag && f < 2; f++) {
            if (r.code[f] != FPL_PASS_FILTER) continue;
            const u32 pl = gz_prefix_len(r.kind[f], g.name_len);
            const u32 fl = r.frag_len[f], fs = r.frag_start[f];
            if (g.name_len) {
                if (lane == 0) d[0] = g.lead;
                if (lane < pl) {
                    const char* pf = pl == 22 ? "split-by-adapter-left-" : "split-by-adapter-right-";
                    d[1 + lane] = (u8)pf[lane];
                }
                gz_wave_copy(d + 1 + pl, g.name_rest, g.name_len - 1);
            }
            d = note(i, f, d + g.name_len + pl);
            gz_wave_copy(d + 1, g.seq + fs, fl);
            u8* d2 = d + 1 + fl + 1;
            if (g.strand) gz_wave_copy(d2, g.strand, g.strand_len); /* (wave-uniform) */
            else if (lane == 0) d2[0] = '+';
            u8* d3 = d2 + g.strand_len + 1;
            gz_wave_copy(d3, g.qual + fs, fl);
            if (lane == 0) {
                d[0] = '\n';
                d2[-1] = '\n';
                d3[-1] = '\n';
                d3[fl] = '\n';
            }
            d = d3 + fl + 1;
        }
    }
}
__global__ void __launch_bounds__(256)
k_gz_compose(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
             const fpl_read_result* __restrict__ res, u32 n_rec, const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    gz_compose_body(GzTextSrc{text, line, nl_pos}, res, n_rec, rec_off, comp, comp_cap);
}
__global__ void __launch_bounds__(256)
k_gz_compose_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                 const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, const u64* __restrict__ rec_off,
                 u8* __restrict__ comp, u64 comp_cap) {
    gz_compose_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, rec_off, comp, comp_cap);
}

/* ---- the fragment forms (fpl_set_fragment_output): the output reads of a --break / --mask batch ----
   The layout's lane and the compose's wave is ordered fragment j of the batch's list (frag_index.h); rec_off has an entry per
   fragment plus one.  The bytes are format_range's with a fragment list (host/format.cpp): the name's first byte, "r<break_no>-"
   when break_no != 0, the split prefix by kind, the rest of the name; the bases with every region of the fragment shown as N;
   the '+' line and the qualities as they are.  A fragment whose code is not FPL_PASS_FILTER, whose read is dropped or whose
   entry nobody claimed writes nothing. */
struct GzFragList {
    const fpl_fragment* frags;
    const fpl_region* regs;
    const u32* order;
    const FragIndex* fi;
};
__device__ __forceinline__ u32 gz_break_digits(u32 break_no) { /* (16 bits: 1 - 5 digits) */
    return break_no >= 10000 ? 5u : (break_no >= 1000 ? 4u : (break_no >= 100 ? 3u : (break_no >= 10 ? 2u : 1u)));
}
/* what a fragment's name line holds between the name's first byte and the rest of it: "r<i>-" and the prefix -- written whether
   the name is empty or not, as format_range does */
__device__ __forceinline__ u32 gz_frag_tag_len(const fpl_fragment& f, u32& pl) {
    pl = f.kind == 1 ? 22u : (f.kind == 2 ? 23u : 0u);
    return pl + (f.break_no ? 2u + gz_break_digits(f.break_no) : 0u);
}
/* ordered fragment j: its list entry, and whether it is written at all */
__device__ __forceinline__ bool gz_frag_take(const GzFragList& fl, const fpl_read_result* __restrict__ res, u32 n_rec, u32 j, u32 n,
                                             fpl_fragment& f) {
    const u32 e = frag_entry(fl.order, j, n);
    if (e == FI_NONE) return false;
    f = fl.frags[e];
    return f.code == FPL_PASS_FILTER && f.read < n_rec && !res[f.read].dropped;
}
template <class Src>
struct GzFragItem {
    Src src;
    const fpl_read_result* res;
    u32 n_rec, n;
    GzFragList fl;
    struct State {
        GzRec g;
        fpl_fragment f;
        bool take;
    };
    __device__ __forceinline__ State load(u32 j) const {
        State s = {};
        s.take = gz_frag_take(fl, res, n_rec, j, n, s.f);
        if (s.take) s.g = src.rec(s.f.read);
        return s;
    }
    __device__ __forceinline__ void lens(const State& s, u64& a, u64& b) const {
        u32 pl;
        a = (u64)s.g.name_len + gz_frag_tag_len(s.f, pl) + 1 + (u64)s.f.len + 1;
        b = (u64)s.g.strand_len + 1 + (u64)s.f.len + 1;
    }
    __device__ __forceinline__ u64 len(const State& s) const {
        if (!s.take) return 0;
        u64 a, b;
        lens(s, a, b);
        return a + b;
    }
    template <class F>
    __device__ __forceinline__ void cuts(const State& s, u64 o, F&& emit) const {
        if (!s.take) return;
        u64 a, b;
        lens(s, a, b);
        gz_frag_cuts(o, a, b, s.f.len, emit);
    }
};
/* (a status of the index is a status of the layout: bit 2, and nothing behind it runs) */
template <class Src>
__device__ __forceinline__ void gz_layout_frag_body(const Src& src, const fpl_read_result* __restrict__ res, u32 n_rec, const GzFragList& fl,
                                                    u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap,
                                                    GzHeader* __restrict__ hdr) {
    const u32 n = frag_index_len(fl.fi);
    gz_layout_scan(GzFragItem<Src>{src, res, n_rec, n, fl}, n, rec_off, blk_start, blk_cap, hdr);
    if (threadIdx.x == 0 && fl.fi->status) hdr->status |= 4u;
}
__global__ void __launch_bounds__(1024)
k_gz_layout_frag(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
                 const fpl_read_result* __restrict__ res, u32 n_rec, GzFragList fl, u64* __restrict__ rec_off, u64* __restrict__ blk_start,
                 u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_frag_body(GzTextSrc{text, line, nl_pos}, res, n_rec, fl, rec_off, blk_start, blk_cap, hdr);
}
__global__ void __launch_bounds__(1024)
k_gz_layout_frag_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                     const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, GzFragList fl,
                     u64* __restrict__ rec_off, u64* __restrict__ blk_start, u32 blk_cap, GzHeader* __restrict__ hdr) {
    gz_layout_frag_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, fl, rec_off, blk_start, blk_cap, hdr);
}

/* len bytes of one value, the wave together */
__device__ __forceinline__ void gz_wave_fill(u8* __restrict__ dst, u8 byte, u32 len) {
    const u32 lane = (u32)lane_id();
    const u32 whole = len & ~15u;
    const u32 w = 0x01010101u * byte;
    const u32x4 v = {w, w, w, w};
    for (u32 i = 16 * lane; i < whole; i += 16 * 64) __builtin_memcpy(dst + i, &v, 16);
    if (lane < (len & 15u)) dst[whole + lane] = byte;
}
/* the bases [start, start + len) of a read at d with the fragment's regions shown as N (frag_clip_region: append_masked's
   clipping).  Written as DISJOINT pieces, a copy for every unmasked stretch and a fill for every region, in the regions' order
   (ascending): a copy of the whole line with the N stored over it would have two lanes of one wave store to one byte, and
   program order says nothing about which of the two lands last. */
__device__ __forceinline__ void gz_wave_masked(u8* __restrict__ d, const u8* __restrict__ bases, u32 start, u32 len,
                                               const fpl_region* __restrict__ regs, u32 n_regs) {
    u32 pos = 0; /* bytes of the fragment written so far */
    for (u32 k = 0; k < n_regs; k++) { /* wave-uniform */
        u32 a, l;
        if (!frag_clip_region(regs[k], start, len, a, l)) continue;
        u32 e = a + l;
        if (a < pos) a = pos; /* (the list is ascending and disjoint; one that is not still gives disjoint pieces) */
        if (e <= a) continue;
        if (a > pos) gz_wave_copy(d + pos, bases + start + pos, a - pos);
        gz_wave_fill(d + a, (u8)'N', e - a);
        pos = e;
    }
    if (pos < len) gz_wave_copy(d + pos, bases + start + pos, len - pos);
}
/* a wave per ordered fragment; comp holds hdr->total bytes */
template <class Src>
__device__ __forceinline__ void gz_compose_frag_body(const Src& src, const fpl_read_result* __restrict__ res, u32 n_rec, const GzFragList& fl,
                                                     const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const u32 lane = (u32)lane_id();
    const u32 n = frag_index_len(fl.fi);
    for (u32 j = wave; j < n; j += n_waves) { /* wave-uniform */
        const u64 o0 = rec_off[j], o1 = rec_off[j + 1];
        if (o1 == o0 || o1 > comp_cap) continue;
        fpl_fragment f;
        if (!gz_frag_take(fl, res, n_rec, j, n, f)) continue; /* (the layout gave it bytes: it is taken) */
        const GzRec g = src.rec_wave(f.read);
        u8* d = comp + o0;
        u32 pl;
        const u32 tl = gz_frag_tag_len(f, pl);
        if (lane == 0) {
            u8* t = d + (g.name_len ? 1 : 0);
            if (g.name_len) d[0] = g.lead;
            if (f.break_no) {
                const u32 nd = gz_break_digits(f.break_no);
                u32 v = f.break_no;
                t[0] = 'r';
                for (u32 k = nd; k > 0; k--, v /= 10) t[k] = (u8)('0' + v % 10);
                t[1 + nd] = '-';
            }
        }
        if (lane < pl) {
            const char* pf = pl == 22 ? "split-by-adapter-left-" : "split-by-adapter-right-";
            d[(g.name_len ? 1 : 0) + (tl - pl) + lane] = (u8)pf[lane];
        }
        if (g.name_len > 1) gz_wave_copy(d + 1 + tl, g.name_rest, g.name_len - 1);
        d += g.name_len + tl;
        gz_wave_masked(d + 1, g.seq, f.start, f.len, fl.regs + f.region_first, f.region_count);
        u8* d2 = d + 1 + f.len + 1;
        if (g.strand) gz_wave_copy(d2, g.strand, g.strand_len); /* (wave-uniform) */
        else if (lane == 0) d2[0] = '+';
        u8* d3 = d2 + g.strand_len + 1;
        gz_wave_copy(d3, g.qual + f.start, f.len);
        if (lane == 0) {
            d[0] = '\n';
            d2[-1] = '\n';
            d3[-1] = '\n';
            d3[f.len] = '\n';
        }
    }
}
__global__ void __launch_bounds__(256)
k_gz_compose_frag(const u8* __restrict__ text, const u32* __restrict__ line, const u32* __restrict__ nl_pos,
                  const fpl_read_result* __restrict__ res, u32 n_rec, GzFragList fl, const u64* __restrict__ rec_off, u8* __restrict__ comp,
                  u64 comp_cap) {
    gz_compose_frag_body(GzTextSrc{text, line, nl_pos}, res, n_rec, fl, rec_off, comp, comp_cap);
}
__global__ void __launch_bounds__(256)
k_gz_compose_frag_bam(const u8* __restrict__ bam, const uint64_t* __restrict__ rec_start, const u8* __restrict__ seq, const u8* __restrict__ qual,
                      const uint64_t* __restrict__ off, const fpl_read_result* __restrict__ res, u32 n_rec, GzFragList fl,
                      const u64* __restrict__ rec_off, u8* __restrict__ comp, u64 comp_cap) {
    gz_compose_frag_body(GzBamSrc{bam, rec_start, seq, qual, off}, res, n_rec, fl, rec_off, comp, comp_cap);
}

/* ---- code lengths: the whole workgroup; everything in LDS ---- */
struct GzCodeScratch {
    u32 key[GZ_NSYM + 3];  /* counts in ascending order, then the algorithm's work array */
    u16 sym[GZ_NSYM + 3];  /* the symbol at each rank */
    u32 cnt[17];           /* symbols per length */
    u32 n;                 /* symbols in use */
};
/* len[s] for s < nsym: a prefix code of at most maxbits bits for the symbols whose freq is not 0 (complete when two or more are
   in use; one symbol gets length 1).  Called by every thread of the workgroup. */
__device__ inline void gz_code_lengths(const u32* freq, int nsym, int maxbits, u8* len, GzCodeScratch* S) {
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    /* rank by (count, symbol): a counting sort, one or two symbols a thread */
    for (int s = tid; s < nsym; s += nthr) {
        const u32 f = freq[s];
        u32 rank = 0, used = 0;
        for (int t = 0; t < nsym; t++) {
            const u32 ft = freq[t];
            if (ft) {
                used++;
                if (f && (ft < f || (ft == f && t < s))) rank++;
            }
        }
        len[s] = 0;
        if (f) {
            S->key[rank] = f;
            S->sym[rank] = (u16)s;
        }
        if (s == 0) S->n = used;
    }
    __syncthreads();
    if (tid == 0) {
        const int n = (int)S->n;
        u32* A = S->key;
        if (n == 1) {
            A[0] = 1;
        } else if (n >= 2) {
            /* Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": A[] ascending counts -> code lengths */
            A[0] += A[1];
            int root = 0, leaf = 2;
            for (int next = 1; next < n - 1; next++) {
                if (leaf >= n || A[root] < A[leaf]) {
                    A[next] = A[root];
                    A[root++] = (u32)next;
                } else {
                    A[next] = A[leaf++];
                }
                if (leaf >= n || (root < next && A[root] < A[leaf])) {
                    A[next] += A[root];
                    A[root++] = (u32)next;
                } else {
                    A[next] += A[leaf++];
                }
            }
            A[n - 2] = 0;
            for (int next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
            int avbl = 1, used = 0, dpth = 0;
            root = n - 2;
            int next = n - 1;
            while (avbl > 0) {
                while (root >= 0 && (int)A[root] == dpth) {
                    used++;
                    root--;
                }
                while (avbl > used) {
                    A[next--] = (u32)dpth;
                    avbl--;
                }
                avbl = 2 * used;
                dpth++;
                used = 0;
            }
        }
        /* counts per length, lengths above the limit folded into it, then the Kraft sum brought back to exactly 2^maxbits: every
           step takes one code off the longest length and splits the deepest shorter one in two */
        for (int l = 0; l <= 16; l++) S->cnt[l] = 0;
        for (int k = 0; k < n; k++) S->cnt[min((int)A[k], maxbits)]++;
        if (n >= 2) {
            u32 total = 0;
            for (int l = maxbits; l > 0; l--) total += S->cnt[l] << (maxbits - l);
            while (total != (1u << maxbits)) {
                S->cnt[maxbits]--;
                for (int l = maxbits - 1; l > 0; l--)
                    if (S->cnt[l]) {
                        S->cnt[l]--;
                        S->cnt[l + 1] += 2;
                        break;
                    }
                total--;
            }
        }
        /* the rarest symbols get the longest codes */
        int k = 0;
        for (int l = maxbits; l >= 1; l--)
            for (u32 c = 0; c < S->cnt[l]; c++) len[S->sym[k++]] = (u8)l;
    }
    __syncthreads();
}

/* thread-private bit writer into a zeroed LDS word array that other threads write too */
struct GzBits {
    u32* w;
    u32 pos;
    __device__ __forceinline__ void put(u32 val, u32 nbits) { /* nbits <= 16 */
        if (nbits == 0) return;
        const u32 i = pos >> 5, s = pos & 31u;
        atomicOr(&w[i], val << s);
        if (s + nbits > 32) atomicOr(&w[i + 1], val >> (32 - s));
        pos += nbits;
    }
};
__device__ __forceinline__ u32 gz_rev(u32 code, u32 len) { return len ? brev32(code) >> (32 - len) : 0u; }

constexpr u32 GZ_OUT_WORDS = (GZ_B + GZ_SLACK + 3) / 4 + 2;

/* a workgroup per deflate block.  tmp: block b's bytes at blk_start[b] + GZ_SLACK * b, blk_size[b] of them;
   blk_crc[b]: the block's share of the member's raw CRC remainder.  BGZF: the share of its BGZF block's remainder (the block's
   bytes shifted to the end of its stripe), and a dynamic header that declares TWO distance codes of length 1 -- a complete set,
   which every inflater takes; the member form's single code is what k_bgzf_inflate refuses. */
template <bool BGZF>
__device__ __forceinline__ void gz_block_body(const u8* __restrict__ comp, const u64* __restrict__ blk_start, const GzHeader* __restrict__ hdr,
                                              u8* __restrict__ tmp, u32* __restrict__ blk_size, u32* __restrict__ blk_crc) {
    __shared__ u32 in_w[GZ_B / 4 + 4];
    __shared__ u32 out_w[GZ_OUT_WORDS];
    __shared__ u32 hist[GZ_NSYM + 3];
    __shared__ u8 len[GZ_NSYM + 3];
    __shared__ u16 code[GZ_NSYM + 3]; /* bit-reversed: as it goes into the stream */
    __shared__ u32 crc_tab[256];
    __shared__ GzCodeScratch scratch;
    __shared__ u8 cl_sym[GZ_NSYM + 8], cl_extra[GZ_NSYM + 8];
    __shared__ u32 cl_freq[19];
    __shared__ u8 cl_len[19 + 1];
    __shared__ u32 wsum[GZ_THREADS / 64];
    __shared__ u32 n_hdr_bits, use_stored, out_size, n_cl;
    const u32 tid = threadIdx.x;
    u8* in = (u8*)in_w;
    const u32 n_blocks = hdr->n_blocks;
    const u64 total = hdr->total;
    crc_tab[tid] = gz_crc_table_entry(tid);
    /* x^(8 * GZ_STRETCH * (threads behind this one)): what this thread's stretch of a block is shifted by (the block's bytes are
       taken as ENDING at the end of the last thread's stretch: zero bytes in front change no remainder) */
    const u32 my_shift = gz_xpow8((u64)GZ_STRETCH * (GZ_THREADS - 1 - tid));
    for (u32 b = blockIdx.x; b < n_blocks; b += gridDim.x) { /* block-uniform */
        __syncthreads();
        const u64 s0 = blk_start[b];
        const u32 n = (u32)(blk_start[b + 1] - s0); /* 1 .. GZ_B */
        const u8* src = comp + s0;
        /* the bytes, coalesced */
        for (u32 i = 16 * tid; i + 16 <= n; i += 16 * GZ_THREADS) {
            u32x4 v;
            __builtin_memcpy(&v, src + i, 16);
            in_w[i / 4] = v.x, in_w[i / 4 + 1] = v.y, in_w[i / 4 + 2] = v.z, in_w[i / 4 + 3] = v.w;
        }
        if (tid < (n & 15u)) in[(n & ~15u) + tid] = src[(n & ~15u) + tid];
        for (u32 i = tid; i < GZ_NSYM; i += GZ_THREADS) hist[i] = i == 256 ? 1u : 0u;
        for (u32 i = tid; i < GZ_OUT_WORDS; i += GZ_THREADS) out_w[i] = 0;
        __syncthreads();
        /* histogram of this thread's symbols; CRC of its stretch of the end-aligned block */
        const u32 a0 = min(n, tid * GZ_STRETCH), a1 = min(n, (tid + 1) * GZ_STRETCH);
        for (u32 i = a0; i < a1; i++) atomicAdd(&hist[in[i]], 1u);
        {
            const u32 pad = GZ_B - n;
            const u32 c0 = tid * GZ_STRETCH > pad ? tid * GZ_STRETCH - pad : 0u;
            const u32 c1 = (tid + 1) * GZ_STRETCH > pad ? (tid + 1) * GZ_STRETCH - pad : 0u;
            u32 c = 0;
            for (u32 i = c0; i < c1; i++) c = crc_tab[(c ^ in[i]) & 0xFFu] ^ (c >> 8);
            c = c ? gz_mulmod(c, my_shift) : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) c ^= shfl_xor_u32(c, d);
            if (lane_id() == 0) wsum[wave_in_block()] = c;
        }
        __syncthreads();
        if (tid == 64) { /* (beside thread 0's serial work below) */
            u32 c = 0;
            for (int k = 0; k < GZ_THREADS / 64; k++) c ^= wsum[k];
            u64 end = total;
            if (BGZF) end = gz_stripe_end(s0, total);
            blk_crc[b] = gz_mulmod(c, gz_xpow8(end - (s0 + n)));
        }
        gz_code_lengths(hist, GZ_NSYM, 15, len, &scratch);
        /* canonical codes: symbols of one length in symbol order */
        if (tid == 0) {
            u32 next = 0;
            scratch.cnt[0] = 0;
            for (int l = 1; l <= 15; l++) { /* cnt[l] := first code of length l */
                const u32 c = scratch.cnt[l];
                scratch.cnt[l] = next;
                next = (next + c) << 1;
            }
        }
        __syncthreads();
        for (u32 s = tid; s < GZ_NSYM; s += GZ_THREADS) {
            const u32 l = len[s];
            u32 rank = 0;
            for (u32 t = 0; t < s; t++) rank += len[t] == l;
            code[s] = (u16)(l ? gz_rev(scratch.cnt[l] + rank, l) : 0u);
        }
        __syncthreads();
        /* the header: run-length symbols over the 257 literal lengths and the distance lengths (one 1; BGZF: two) */
        if (tid == 0) {
            u32 m = 0;
            for (int i = 0; i < 19; i++) cl_freq[i] = 0;
            for (u32 i = 0; i < GZ_NSYM + (BGZF ? 2u : 1u);) {
                const u32 v = i < GZ_NSYM ? len[i] : 1u;
                if (v != 0) {
                    cl_sym[m] = (u8)v, cl_extra[m] = 0, m++, i++;
                    cl_freq[v]++;
                    continue;
                }
                u32 run = 1;
                while (i + run < GZ_NSYM && len[i + run] == 0) run++;
                i += run;
                while (run >= 11) {
                    const u32 t = min(run, 138u);
                    cl_sym[m] = 18, cl_extra[m] = (u8)(t - 11), m++;
                    cl_freq[18]++;
                    run -= t;
                }
                if (run >= 3) {
                    cl_sym[m] = 17, cl_extra[m] = (u8)(run - 3), m++;
                    cl_freq[17]++;
                    run = 0;
                }
                for (; run; run--) {
                    cl_sym[m] = 0, cl_extra[m] = 0, m++;
                    cl_freq[0]++;
                }
            }
            n_cl = m;
        }
        __syncthreads();
        gz_code_lengths(cl_freq, 19, 7, cl_len, &scratch);
        if (tid == 0) {
            /* literal bits (end-of-block included) */
            u32 body = 0;
            for (u32 s = 0; s < GZ_NSYM; s++) body += hist[s] * len[s];
            u32 first[8], next = 0, cl_code[19];
            for (int l = 1; l <= 7; l++) {
                first[l] = next;
                next = (next + scratch.cnt[l]) << 1;
            }
            for (int s = 0; s < 19; s++) {
                const u32 l = cl_len[s];
                cl_code[s] = l ? gz_rev(first[l]++, l) : 0u;
            }
            const u8 order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            u32 hclen = 19;
            while (hclen > 4 && cl_len[order[hclen - 1]] == 0) hclen--;
            GzBits bw = {out_w, 0};
            bw.put(0, 1);  /* BFINAL */
            bw.put(2, 2);  /* BTYPE: dynamic */
            bw.put(0, 5);  /* HLIT: 257 codes */
            bw.put(BGZF ? 1 : 0, 5);  /* HDIST: 1 code; BGZF: 2 */
            bw.put(hclen - 4, 4);
            for (u32 i = 0; i < hclen; i++) bw.put(cl_len[order[i]], 3);
            const u32 m = n_cl;
            for (u32 i = 0; i < m; i++) {
                const u32 s = cl_sym[i];
                bw.put(cl_code[s], cl_len[s]);
                if (s == 17) bw.put(cl_extra[i], 3);
                if (s == 18) bw.put(cl_extra[i], 7);
            }
            const u32 hdr_bits = bw.pos;
            /* end of block sits in `body`; then the empty stored block: 3 header bits, up to the byte, 00 00 FF FF */
            const u32 end_bits = hdr_bits + body + 3;
            const u32 dyn_bytes = (end_bits + 7) / 8 + 4;
            n_hdr_bits = hdr_bits;
            use_stored = dyn_bytes >= n + GZ_SLACK;
            out_size = use_stored ? n + GZ_SLACK : dyn_bytes;
            if (!use_stored) {
                bw.pos = hdr_bits + body - len[256];
                bw.put(code[256], len[256]);
                bw.pos = (end_bits + 7) / 8 * 8 + 16;
                bw.put(0xFFFFu, 16);
            }
        }
        __syncthreads();
        u8* dst = tmp + s0 + (u64)GZ_SLACK * b;
        const u32 size = out_size;
        if (use_stored) {
            if (tid == 0) {
                dst[0] = 0;
                dst[1] = (u8)(n & 0xFF), dst[2] = (u8)(n >> 8);
                dst[3] = (u8)(~n & 0xFF), dst[4] = (u8)((~n >> 8) & 0xFF);
            }
            for (u32 i = tid; i < n; i += GZ_THREADS) dst[GZ_SLACK + i] = in[i];
        } else {
            /* where this thread's codes go */
            u32 bits = 0;
            for (u32 i = a0; i < a1; i++) bits += len[in[i]];
            const u32 incl = wave_scan_incl_u32(bits);
            if (lane_id() == 63) wsum[wave_in_block()] = incl;
            __syncthreads();
            u32 pos = n_hdr_bits + incl - bits;
            for (int k = 0; k < wave_in_block(); k++) pos += wsum[k];
            if (bits) {
                u32 w = pos >> 5;
                u32 have = pos & 31u; /* low bits of the first word are somebody else's */
                u64 acc = 0;
                bool first = true;
                for (u32 i = a0; i < a1; i++) {
                    const u32 s = in[i];
                    acc |= (u64)code[s] << have;
                    have += len[s];
                    if (have >= 32) {
                        if (first) atomicOr(&out_w[w], (u32)acc);
                        else out_w[w] = (u32)acc; /* (all 32 bits are this thread's) */
                        first = false;
                        w++;
                        acc >>= 32;
                        have -= 32;
                    }
                }
                if (have) atomicOr(&out_w[w], (u32)acc);
            }
            __syncthreads();
            const u8* ob = (const u8*)out_w;
            for (u32 i = 16 * tid; i + 16 <= size; i += 16 * GZ_THREADS) {
                u32x4 v;
                v.x = out_w[i / 4], v.y = out_w[i / 4 + 1], v.z = out_w[i / 4 + 2], v.w = out_w[i / 4 + 3];
                __builtin_memcpy(dst + i, &v, 16);
            }
            if (tid < (size & 15u)) dst[(size & ~15u) + tid] = ob[(size & ~15u) + tid];
        }
        if (tid == 0) blk_size[b] = size;
    }
}
__global__ void __launch_bounds__(GZ_THREADS)
k_gz_block(const u8* __restrict__ comp, const u64* __restrict__ blk_start, const GzHeader* __restrict__ hdr, u8* __restrict__ tmp,
           u32* __restrict__ blk_size, u32* __restrict__ blk_crc) {
    gz_block_body<false>(comp, blk_start, hdr, tmp, blk_size, blk_crc);
}
__global__ void __launch_bounds__(GZ_THREADS)
k_gz_block_bgzf(const u8* __restrict__ comp, const u64* __restrict__ blk_start, const GzHeader* __restrict__ hdr, u8* __restrict__ tmp,
                u32* __restrict__ blk_size, u32* __restrict__ blk_crc) {
    gz_block_body<true>(comp, blk_start, hdr, tmp, blk_size, blk_crc);
}

/* one block: blk_off[b] = bytes of the member in front of block b's; header, final block, trailer; hdr->gz_len, hdr->crc */
__global__ void __launch_bounds__(1024)
k_gz_finish(const u32* __restrict__ blk_size, const u32* __restrict__ blk_crc, u64* __restrict__ blk_off, GzHeader* __restrict__ hdr,
            u8* __restrict__ out, u64 out_cap) {
    __shared__ u64 wsum[16];
    __shared__ u32 wcrc[16];
    __shared__ u64 carry;
    const u32 n_blocks = hdr->n_blocks;
    if (threadIdx.x == 0) carry = 10;
    u32 crc = 0;
    __syncthreads();
    for (u32 base = 0; base < n_blocks; base += 1024) { /* block-uniform */
        const u32 i = base + threadIdx.x;
        const u64 v = i < n_blocks ? blk_size[i] : 0u;
        if (i < n_blocks) crc ^= blk_crc[i];
        const u64 incl = gz_scan_incl_u64(v);
        if (lane_id() == 63) wsum[wave_in_block()] = incl;
        __syncthreads();
        u64 run = carry + incl - v;
        for (int k = 0; k < wave_in_block(); k++) run += wsum[k];
        if (i < n_blocks) blk_off[i] = run;
        __syncthreads();
        if (threadIdx.x == 1023) carry = run + v;
        __syncthreads();
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) crc ^= shfl_xor_u32(crc, d);
    if (lane_id() == 0) wcrc[wave_in_block()] = crc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 total = hdr->total;
        if (total == 0 || hdr->status) {
            hdr->gz_len = 0;
            return;
        }
        u32 raw = 0;
        for (int k = 0; k < 16; k++) raw ^= wcrc[k];
        /* the register starts as all ones: that is 0xFFFFFFFF * x^(8 total) on top of the remainder of the bytes */
        const u32 c = raw ^ gz_mulmod(0xFFFFFFFFu, gz_xpow8(total)) ^ 0xFFFFFFFFu;
        const u64 end = carry;
        hdr->crc = c;
        hdr->gz_len = end + 13;
        if (end + 13 > out_cap) {
            hdr->status = 1;
            hdr->gz_len = 0;
            return;
        }
        const u8 head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff}; /* deflate, no flags, no time, unknown system */
        for (int k = 0; k < 10; k++) out[k] = head[k];
        u8* t = out + end;
        t[0] = 1, t[1] = 0, t[2] = 0, t[3] = 0xff, t[4] = 0xff; /* BFINAL, stored, 0 bytes */
        for (int k = 0; k < 4; k++) t[5 + k] = (u8)(c >> (8 * k));
        for (int k = 0; k < 4; k++) t[9 + k] = (u8)((u32)total >> (8 * k));
    }
}

/* The BGZF form of the finish.  One block: the running sum of the deflate blocks' sizes as above; a deflate block's place is the
   sum in front of it plus the frames in front of it and its own stripe's header: blk_off[b] = sum + 18 + 31 * (blk_start[b] /
   GZ_STRIPE).  hdr->crc stays the CRC-32 of the whole composed text: every block's remainder stands at the end of its stripe
   (k_gz_block_bgzf) and is shifted on to the end of the text here.  Every thread takes a run of consecutive blocks and
   carries ONE remainder through it, multiplied by x^(8 * the next stripe's bytes) whenever the run enters the next stripe; at
   the end of the run what is left to the end of the text is a whole number m of stripes and the last stripe's length, and
   x^(8 * GZ_STRIPE * 2^j) for the bits j of m comes from a table of 32 entries.  (A gz_xpow8 per block, each a chain of some
   sixty gz_mulmod, was 22 ms for the 122 000 blocks of a 1 Gbase batch; the table per block still 5.)  hdr->gz_len = the
   BGZF blocks together. */
__global__ void __launch_bounds__(1024)
k_gz_finish_bgzf(const u64* __restrict__ blk_start, const u32* __restrict__ blk_size, const u32* __restrict__ blk_crc,
                 u64* __restrict__ blk_off, GzHeader* __restrict__ hdr, u64 out_cap) {
    __shared__ u64 wsum[16];
    __shared__ u32 wcrc[16];
    __shared__ u64 carry;
    __shared__ u32 pw[32], last_pw;
    const u32 n_blocks = hdr->n_blocks;
    const u64 total = hdr->total;
    const u64 n_stripes = (total + GZ_STRIPE - 1) / GZ_STRIPE;
    if (threadIdx.x == 0) carry = 0;
    if (threadIdx.x < 32) { /* pw[j] = x^(8 * GZ_STRIPE * 2^j) */
        u32 r = gz_xpow8(GZ_STRIPE);
        for (u32 j = 0; j < threadIdx.x; j++) r = gz_mulmod(r, r);
        pw[threadIdx.x] = r;
    }
    if (threadIdx.x == 32) last_pw = n_stripes ? gz_xpow8(total - (n_stripes - 1) * GZ_STRIPE) : 0u; /* x^(8 * the last stripe's bytes) */
    u32 crc = 0;
    __syncthreads();
    {
        const u32 per = (n_blocks + 1023) / 1024;
        const u32 b0 = min(n_blocks, threadIdx.x * per), b1 = n_blocks - b0 < per ? n_blocks : b0 + per;
        u64 cur = b0 < b1 ? blk_start[b0] / GZ_STRIPE : 0u; /* the stripe crc stands at the end of */
        /* (eight blocks' loads at a time: a lane's run is its own stretch of memory, so a load of one element per lane is 64
           cache lines, and 240 of them one after the other were most of this kernel's 5 ms on a 1 Gbase batch) */
        for (u32 i0 = b0; i0 < b1; i0 += 8) {
            u64 st[8];
            u32 cr[8];
#pragma unroll
            for (u32 k = 0; k < 8; k++) {
                const u32 i = i0 + k < b1 ? i0 + k : b1 - 1;
                st[k] = blk_start[i];
                cr[k] = blk_crc[i];
            }
#pragma unroll
            for (u32 k = 0; k < 8; k++) {
                if (i0 + k >= b1) break;
                const u64 stripe = st[k] / GZ_STRIPE;
                for (; cur < stripe; cur++) /* (every stripe has a block: one step at most) */
                    crc = crc ? gz_mulmod(crc, cur + 2 == n_stripes ? last_pw : pw[0]) : 0u;
                crc ^= cr[k];
            }
        }
        if (crc && cur + 1 < n_stripes) { /* (n_stripes <= n_blocks < 2^32: m has at most 32 bits) */
            u32 f = last_pw;
            u64 m = n_stripes - 2 - cur;
            for (int j = 0; m && j < 32; j++, m >>= 1)
                if (m & 1ull) f = gz_mulmod(f, pw[j]);
            crc = gz_mulmod(crc, f);
        }
    }
    for (u32 base = 0; base < n_blocks; base += 1024) { /* block-uniform */
        const u32 i = base + threadIdx.x;
        u64 v = 0, stripe = 0;
        if (i < n_blocks) { /* (both loads under one branch: in flight together) */
            const u32 sz = blk_size[i];
            const u64 at = blk_start[i];
            v = sz, stripe = at / GZ_STRIPE;
        }
        const u64 incl = gz_scan_incl_u64(v);
        if (lane_id() == 63) wsum[wave_in_block()] = incl;
        __syncthreads();
        u64 run = carry + incl - v;
        for (int k = 0; k < wave_in_block(); k++) run += wsum[k];
        if (i < n_blocks) blk_off[i] = run + GZ_BGZF_HEAD + (u64)GZ_BGZF_EXTRA * stripe;
        __syncthreads();
        if (threadIdx.x == 1023) carry = run + v;
        __syncthreads();
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) crc ^= shfl_xor_u32(crc, d);
    if (lane_id() == 0) wcrc[wave_in_block()] = crc;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (total == 0 || hdr->status) {
            hdr->gz_len = 0;
            return;
        }
        u32 raw = 0;
        for (int k = 0; k < 16; k++) raw ^= wcrc[k];
        hdr->crc = raw ^ gz_mulmod(0xFFFFFFFFu, gz_xpow8(total)) ^ 0xFFFFFFFFu;
        const u64 len = carry + (u64)GZ_BGZF_EXTRA * ((total + GZ_STRIPE - 1) / GZ_STRIPE);
        hdr->gz_len = len;
        if (len > out_cap) {
            hdr->status = 1;
            hdr->gz_len = 0;
        }
    }
}

/* A thread per stripe, behind k_gz_finish_bgzf: the stripe's deflate blocks are those whose start lies in it (a search in
   blk_start: the stripe's first byte is a multiple of GZ_B, so it IS a start); their remainders XORed are the raw remainder of
   the stripe's bytes, the all-ones term of its length makes the CRC-32.  Writes the 18-byte header with BSIZE in front of the
   stripe's first deflate block and, behind its last, the final empty stored block, CRC-32 and ISIZE.  A block over 65 536 bytes
   (the bound beside GZ_STRIPE says there is none) is a status, not a file. */
__global__ void __launch_bounds__(256)
k_gz_frame(const u64* __restrict__ blk_start, const u32* __restrict__ blk_size, const u32* __restrict__ blk_crc,
           const u64* __restrict__ blk_off, GzHeader* __restrict__ hdr, u8* __restrict__ out, u64 out_cap) {
    if (hdr->gz_len == 0) return; /* (nothing to write, or the finish found the output too small) */
    const u32 n_blocks = hdr->n_blocks;
    const u64 total = hdr->total;
    const u64 n_stripes = (total + GZ_STRIPE - 1) / GZ_STRIPE;
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < n_stripes; k += (u64)gridDim.x * blockDim.x) {
        const u64 s = k * GZ_STRIPE, e = gz_stripe_end(s, total);
        /* first block that starts at or behind s, and at or behind e */
        u32 lo = 0, hi = n_blocks;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2;
            if (blk_start[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        const u32 b0 = lo;
        u32 b1 = b0, raw = 0;
        while (b1 < n_blocks && blk_start[b1] < e) raw ^= blk_crc[b1++];
        if (b1 == b0) continue; /* (cannot be: s is a block start) */
        const u64 begin = blk_off[b0] - GZ_BGZF_HEAD;
        const u64 tail = blk_off[b1 - 1] + blk_size[b1 - 1];
        const u64 bytes = tail + 13 - begin;
        if (bytes > GZ_BGZF_MAX) {
            atomicOr(&hdr->status, 2u);
            continue;
        }
        if (tail + 13 > out_cap) continue;
        const u32 isize = (u32)(e - s);
        const u32 c = raw ^ gz_mulmod(0xFFFFFFFFu, gz_xpow8(isize)) ^ 0xFFFFFFFFu;
        const u8 head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        u8* h = out + begin;
        for (int i = 0; i < 16; i++) h[i] = head[i];
        h[16] = (u8)((bytes - 1) & 0xFF), h[17] = (u8)((bytes - 1) >> 8);
        u8* t = out + tail;
        t[0] = 1, t[1] = 0, t[2] = 0, t[3] = 0xff, t[4] = 0xff; /* BFINAL, stored, 0 bytes */
        for (int i = 0; i < 4; i++) t[5 + i] = (u8)(c >> (8 * i));
        for (int i = 0; i < 4; i++) t[9 + i] = (u8)(isize >> (8 * i));
    }
}

/* (either form: blk_off says where a block's bytes go) */
__global__ void __launch_bounds__(GZ_THREADS)
k_gz_compact(const u8* __restrict__ tmp, const u64* __restrict__ blk_start, const u32* __restrict__ blk_size,
             const u64* __restrict__ blk_off, const GzHeader* __restrict__ hdr, u8* __restrict__ out, u64 out_cap) {
    const u32 n_blocks = hdr->n_blocks;
    if (hdr->gz_len == 0) return;
    for (u32 b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const u8* src = tmp + blk_start[b] + (u64)GZ_SLACK * b;
        const u32 size = blk_size[b];
        if (blk_off[b] + size > out_cap) continue;
        u8* dst = out + blk_off[b];
        const u32 whole = size & ~15u;
        for (u32 i = 16 * threadIdx.x; i < whole; i += 16 * GZ_THREADS) {
            u32x4 v;
            __builtin_memcpy(&v, src + i, 16);
            __builtin_memcpy(dst + i, &v, 16);
        }
        if (threadIdx.x < (size & 15u)) dst[whole + threadIdx.x] = src[whole + threadIdx.x];
    }
}

}  // namespace fpl
#endif
