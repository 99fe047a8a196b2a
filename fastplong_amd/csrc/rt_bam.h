/* rt_bam.h -- BAM in: records the host found (fpl_process_bam_async, fpl_decode_bam; bam_decode.h), and a BAM's BGZF blocks whose
   records the device finds itself -- a staged kind of rt_slots.h (bgzf_inflate.h, bam_walk.h) -- with the tail between two
   submissions and the calls that bring a refused stretch back.  (--break / --mask: fpl_set_bam_gzip is refused until
   fpl_set_fragment_output is on; the BGZF kind stays refused.) */
#pragma once

int fpl_set_bam_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    if (on && ctx->hcfg.defer && !ctx->frag_out) return FPL_ERR_STATE; /* (--break / --mask write from fragment lists: fpl_set_fragment_output first) */
    ctx->bam_gzip = on != 0;
    return FPL_OK;
}

/* ---- BAM records in (ABI v8): csrc/bam_decode.h ---- */
/* what the decode kernel will read of every record lies inside [0, n_bytes): the fixed fields, the name, the CIGAR, the bases and
   the qualities; l_seq agrees with the CSR offsets.  (The host walked the records already -- this is the library's own bounds
   check, 24 bytes per record, so that no caller can make the kernel read outside the upload.) */
static int bam_check(const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off, u32 n_reads, u32* max_len) {
    u32 ml = 0;
    for (u32 i = 0; i < n_reads; i++) {
        if (!read_len_ok(off, i, ml)) return FPL_ERR_ARG;
        const uint64_t rs = rec_start[i];
        if (rs > n_bytes || n_bytes - rs < 36) return FPL_ERR_ARG;
        const uint8_t* r = bam + rs;
        const uint64_t l_name = r[12], n_cigar = (uint64_t)r[16] | ((uint64_t)r[17] << 8);
        uint32_t l_seq;
        memcpy(&l_seq, r + 20, 4);
        if (l_seq > 0x7FFFFFFFu || (uint64_t)l_seq != off[i + 1] - off[i]) return FPL_ERR_ARG;
        const uint64_t need = 36 + l_name + 4 * n_cigar + ((uint64_t)l_seq + 1) / 2 + l_seq;
        if (n_bytes - rs < need) return FPL_ERR_ARG;
    }
    if (max_len) *max_len = ml;
    return FPL_OK;
}

/* enqueue the decode of a batch whose records, record starts and offsets are on the device (stream st) */
static void bam_launch(const u8* d_bam, const uint64_t* d_rec, const uint64_t* d_off, u32 n_reads, uint64_t o_begin, uint64_t o_end,
                       u8* d_seq, u8* d_qual, hipStream_t st) {
    u64 word0, n_words;
    bam_words(o_begin, o_end, word0, n_words);
    if (!n_words) return;
    const u64 blocks = (n_words + BAM_THREADS - 1) / BAM_THREADS;
    hipLaunchKernelGGL(k_bam_decode, dim3((u32)blocks), dim3(BAM_THREADS), 0, st, d_bam, d_rec, d_off, n_reads, word0, n_words, d_seq,
                       d_qual);
}

int fpl_process_bam_async(fpl_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                          uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out, fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    if (n_reads && (!bam || !rec_start || !off || !results)) return FPL_ERR_ARG;
    /* (a gzip batch may leave the decoded arrays on the device: both NULL or neither) */
    if (n_reads && (!seq_out || !qual_out) && !(ctx->bam_gzip && !seq_out && !qual_out)) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(slot_begin(ctx, BatchKind::BAM, ctx->bam_gzip, slp));
    u32 max_len = 0;
    if (n_reads && bam_check(bam, n_bytes, rec_start, off, n_reads, &max_len) != FPL_OK) {
        ctx->err = "fpl_process_bam_async: a record does not lie inside the bytes given, or its l_seq disagrees with the offsets";
        return FPL_ERR_ARG;
    }
    fpl_ctx::Slot& sl = *slp;
    sl.n_reads = n_reads;
    sl.user_results = results;
    if (n_reads == 0) return slot_commit(ctx, sl, FPL_OK);
    fpl_ctx::Slot::Bam& b = sl.bam;
    const uint64_t o_begin = off[0], o_end = off[n_reads];
    b.o_begin = o_begin;
    b.bases = o_end - o_begin;
    b.bytes = n_bytes;
    b.seq_out = seq_out;
    b.qual_out = qual_out;
    FPL_TRY(ensure_host_streams(ctx));
    FPL_TRY(ensure_slot(ctx, sl, n_reads, o_end + 16)); /* (the decode writes whole 16-byte words) */
    if (!b.d_bam.holds(n_bytes + BAM_PAD)) FPL_HIP(regrow(b.d_bam.want(grown(n_bytes, BAM_PAD))));
    FPL_HIP(b.d_rec.grow(n_reads, 16));
    auto enqueue = [&]() -> int {
        /* the upload on the copy stream, the decode on the parse stream behind it (the next batch's upload goes out meanwhile), the
           per-read kernels behind the decode; the records, bases and qualities come back on the way-back stream */
        FPL_HIP(hipMemcpyAsync(b.d_bam.ptr, bam, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipMemcpyAsync(b.d_rec.ptr, rec_start, sizeof(uint64_t) * (size_t)n_reads, hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipMemcpyAsync(sl.d_off.ptr, off, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        FPL_HIP(hipStreamWaitEvent(ctx->s_parse, sl.ev_h2d, 0));
        bam_launch(b.d_bam.ptr, b.d_rec.ptr, sl.d_off.ptr, n_reads, o_begin, o_end, sl.d_seq.ptr, sl.d_qual.ptr, ctx->s_parse);
        FPL_HIP(hipGetLastError());
        FPL_HIP(hipEventRecord(sl.ev_parsed, ctx->s_parse));
        return submit_tail(ctx, sl, sl.ev_parsed, n_reads, o_end, max_len);
    };
    return slot_commit(ctx, sl, enqueue());
}

int fpl_decode_bam(int32_t device, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off, uint32_t n_reads,
                   uint8_t* seq_out, uint8_t* qual_out) {
    if (n_reads == 0) return FPL_OK;
    if (!bam || !rec_start || !off || !seq_out || !qual_out || device < 0) return FPL_ERR_ARG;
    if (bam_check(bam, n_bytes, rec_start, off, n_reads, nullptr) != FPL_OK) return FPL_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return FPL_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FPL_ERR_HIP;
    const uint64_t o_begin = off[0], o_end = off[n_reads];
    DevBuf<u8> d_bam, d_seq, d_qual;
    DevBuf<uint64_t> d_rec, d_off;
    const size_t out_bytes = (size_t)((o_end + 15) & ~15ull);
    if (d_bam.alloc(n_bytes + BAM_PAD) != hipSuccess || d_rec.alloc(n_reads) != hipSuccess || d_off.alloc((size_t)n_reads + 1) != hipSuccess ||
        d_seq.alloc(out_bytes + 16) != hipSuccess || d_qual.alloc(out_bytes + 16) != hipSuccess)
        return FPL_ERR_HIP;
    if (hipMemcpy(d_bam.ptr, bam, n_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_rec.ptr, rec_start, sizeof(uint64_t) * n_reads, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_off.ptr, off, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice) != hipSuccess)
        return FPL_ERR_HIP;
    bam_launch(d_bam.ptr, d_rec.ptr, d_off.ptr, n_reads, o_begin, o_end, d_seq.ptr, d_qual.ptr, 0);
    if (hipGetLastError() != hipSuccess) return FPL_ERR_HIP;
    if (o_end > o_begin && (hipMemcpy(seq_out + o_begin, d_seq.ptr + o_begin, o_end - o_begin, hipMemcpyDeviceToHost) != hipSuccess ||
                            hipMemcpy(qual_out + o_begin, d_qual.ptr + o_begin, o_end - o_begin, hipMemcpyDeviceToHost) != hipSuccess))
        return FPL_ERR_HIP;
    return FPL_OK;
}

/* ---- BGZF blocks in, records out: bgzf_inflate.h -> bam_walk.h -> bam_decode.h -> the per-read kernels ---- */
/* a batch of either kind that carries the tail (BGZF BAM, BGZF text) is in flight */
static bool bgzf_in_flight(const fpl_ctx* ctx) {
    for (u32 k = ctx->waited; k != ctx->submitted; k++)
        if (bgzf_kind(ctx->slot[k % FPL_MAX_IN_FLIGHT].kind)) return true;
    return false;
}
/* k_bgzf_inflate's grid: a wave per block; as many workgroups as the device keeps resident (the tables' LDS bounds them), the rest
   off the counter */
static inline u32 bgzf_grid(u32 n_blocks, u32 n_cu) {
    const u32 per_cu = std::max<u32>(1, std::min<u32>(8, (u32)(160u * 1024 / (sizeof(BgzfWaveLds) * (BGZF_THREADS / WAVE) + 1024))));
    return std::min<u32>((n_blocks + BGZF_THREADS / WAVE - 1) / (BGZF_THREADS / WAVE), n_cu * per_cu);
}
/* room for a submission's names: a quarter of [tail room | inflated bytes] and 1 MiB, never more than all of it (a name is part of
   its record).  Records whose names take more than that are FPL_BAMW_TOO_MANY, as more than a record per 64 bytes is. */
static inline uint64_t bam_names_cap(uint64_t hi) { return std::min<uint64_t>(hi, hi / 4 + (1u << 20)); }
/* the walk's state and the tail buffer, made on first use (all zero: no tail, nothing refused) */
static int ensure_bam_tail(fpl_ctx* ctx) {
    if (!ctx->d_bamw_state.ptr) {
        FPL_HIP(ctx->d_bamw_state.alloc(1));
        FPL_HIP(hipMemset(ctx->d_bamw_state.ptr, 0, sizeof(BamWalkState)));
    }
    if (!ctx->d_bam_tail.ptr) FPL_HIP(ctx->d_bam_tail.alloc((size_t)std::max<uint64_t>(ctx->bam_tail_cap, 1)));
    return FPL_OK;
}

/* every range of a block table, before anything is enqueued: the payload inside the compressed bytes, the sizes BGZF allows, and the
   output either in order and without gaps from 0, 32 bits in all (out_bytes == nullptr; *total: their sum), or anywhere inside
   [0, *out_bytes) */
static bool bgzf_blocks_ok(const fpl_bgzf_block* blocks, uint32_t n_blocks, uint64_t comp_bytes, const uint64_t* out_bytes, uint64_t* total) {
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_blocks; i++) {
        const fpl_bgzf_block& d = blocks[i];
        if (d.comp_len > BGZF_MAX_COMP || d.isize > BGZF_MAX_ISIZE || d.comp_off > comp_bytes || comp_bytes - d.comp_off < d.comp_len) return false;
        if (out_bytes ? d.out_off > *out_bytes || *out_bytes - d.out_off < d.isize : d.out_off != sum) return false;
        sum += d.isize;
        if (!out_bytes && sum > 0xFFFFFFF0ull) return false;
    }
    if (total) *total = sum;
    return true;
}
/* the inflate of a block table that is on the device, on stream st: the kernel's work counter at zero, then the kernel */
static hipError_t bgzf_inflate_enqueue(const u8* d_comp, fpl_bgzf_block* d_blocks, u32 n_blocks, u8* d_out, u32* d_next, u32 n_cu, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(d_next, 0, sizeof(u32), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(bgzf_grid(n_blocks, n_cu)), dim3(BGZF_THREADS), 0, st, d_comp, d_blocks, n_blocks, d_out, d_next);
    return hipSuccess;
}

int fpl_process_bgzf_bam_async(fpl_ctx* ctx, const uint8_t* comp, uint64_t comp_bytes, const fpl_bgzf_block* blocks, uint32_t n_blocks,
                               uint64_t skip) {
    if (!ctx || (n_blocks && !blocks) || (comp_bytes && !comp)) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(slot_begin(ctx, BatchKind::BGZF, ctx->bam_gzip, slp));
    if (!ctx->bam_fresh && ctx->tail_kind != BatchKind::BGZF) {
        ctx->err = "fpl_process_bgzf_bam_async: the context holds the tail of BGZF text submissions";
        return FPL_ERR_STATE;
    }
    if (skip && !ctx->bam_fresh) {
        ctx->err = "fpl_process_bgzf_bam_async: skip is valid only while the context holds no tail";
        return FPL_ERR_ARG;
    }
    uint64_t total = 0;
    if (!bgzf_blocks_ok(blocks, n_blocks, comp_bytes, nullptr, &total)) return FPL_ERR_ARG;
    BamWalkJob j;
    if (!bam_walk_plan(j, ctx->bam_tail_cap, total, skip, ctx->bam_seg_bytes)) return FPL_ERR_ARG;
    fpl_ctx::Slot& sl = *slp;
    fpl_ctx::Slot::Bam& b = sl.bam;
    b.o_begin = b.bases = 0;
    b.seq_out = b.qual_out = nullptr;
    FPL_TRY(ensure_host_streams(ctx));
    FPL_TRY(ensure_bam_tail(ctx));
    const u32 rec_cap = bam_walk_rec_cap(total);
    const uint64_t hi = j.tail_cap + total;
    b.bytes = hi;
    if (!b.d_whdr.ptr) {
        FPL_HIP(b.d_whdr.alloc(1));
        FPL_HIP(b.h_whdr.alloc(1));
        FPL_HIP(b.d_next.alloc(1));
    }
    if (!b.d_bam.holds(hi + BAM_PAD)) FPL_HIP(regrow(b.d_bam.want(grown(hi, BAM_PAD))));
    FPL_HIP(b.d_names.grow((size_t)bam_names_cap(hi) + 1, 4096));
    if (!sl.d_results.holds(rec_cap)) {
        const size_t cap = grown(rec_cap, 16);
        FPL_HIP(regrow(sl.d_off.want(cap + 1), sl.d_results.want(cap)));
    }
    if (!b.d_name_off.holds((size_t)rec_cap + 1)) {
        const size_t cap = grown(rec_cap, 16);
        FPL_HIP(regrow(b.d_rec.want(cap + 1), b.d_name_off.want(cap + 1)));
    }
    FPL_HIP(b.d_rec.grow((size_t)rec_cap + 1, 16)); /* (a slot fpl_process_bam_async sized before) */
    FPL_HIP(b.d_comp.grow((size_t)comp_bytes + 1, 4096));
    FPL_HIP(b.d_blocks.grow((size_t)n_blocks + 1, 64));
    if (!b.d_cand.holds(j.n_seg)) {
        const size_t cap = grown(j.n_seg, 64);
        FPL_HIP(regrow(b.d_cand.want(cap), b.d_segs.want(cap), b.d_bases.want(cap)));
    }
    FPL_HIP(b.d_lists.grow((size_t)j.n_seg * j.per_seg, 4096));
    j.buf = b.d_bam.ptr;
    j.rec_cap = rec_cap;
    j.st = ctx->d_bamw_state.ptr;
    j.tail_buf = ctx->d_bam_tail.ptr;
    j.blocks = b.d_blocks.ptr;
    j.n_blocks = n_blocks;
    j.cand = b.d_cand.ptr;
    j.segs = b.d_segs.ptr;
    j.lists = b.d_lists.ptr;
    j.bases = b.d_bases.ptr;
    j.hdr = b.d_whdr.ptr;
    j.rec_start = b.d_rec.ptr;
    j.off = sl.d_off.ptr;
    j.name_off = b.d_name_off.ptr;
    j.names = b.d_names.ptr;
    j.names_cap = bam_names_cap(hi);
    auto enqueue = [&]() -> int {
        /* the upload on the copy stream; inflate and walk on the parse stream behind it, and behind the walk of the submission
           before -- that order carries the tail; only the header comes back */
        if (comp_bytes) FPL_HIP(hipMemcpyAsync(b.d_comp.ptr, comp, comp_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        if (n_blocks) FPL_HIP(hipMemcpyAsync(b.d_blocks.ptr, blocks, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        hipStream_t st = ctx->s_parse;
        FPL_HIP(hipStreamWaitEvent(st, sl.ev_h2d, 0));
        if (n_blocks) FPL_HIP(bgzf_inflate_enqueue(b.d_comp.ptr, b.d_blocks.ptr, n_blocks, b.d_bam.ptr + j.tail_cap, b.d_next.ptr, ctx->n_cu, st));
        bam_walk_enqueue(j, st);
        FPL_HIP(hipGetLastError());
        FPL_HIP(hipMemcpyAsync(b.h_whdr.ptr, b.d_whdr.ptr, sizeof(fpl_bam_window), hipMemcpyDeviceToHost, st));
        FPL_HIP(hipEventRecord(sl.ev_parsed, st));
        return FPL_OK;
    };
    const int r = slot_commit(ctx, sl, enqueue(), 1);
    if (r == FPL_OK) {
        ctx->bam_fresh = false;
        ctx->tail_kind = BatchKind::BGZF;
    }
    return r;
}

/* stage 2 of a BGZF batch (slot_continue): the header is in -- the decode, the per-read kernels, the way back of the records and the names */
static int bgzf_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out) {
    fpl_ctx::Slot::Bam& b = sl.bam;
    const fpl_bam_window h = *b.h_whdr.ptr;
    if (h.status != FPL_BAMW_OK || h.n_reads == 0) return FPL_OK; /* nothing to run: the wait reports */
    const u32 n = h.n_reads;
    b.o_begin = 0;
    b.bases = h.n_bases;
    b.seq_out = seq_out;
    b.qual_out = qual_out;
    FPL_TRY(ensure_slot(ctx, sl, n, h.n_bases + 16)); /* (the decode writes whole 16-byte words; d_off / d_results hold rec_cap already) */
    FPL_HIP(b.h_names.grow((size_t)h.name_bytes + 1, 4096));
    FPL_HIP(b.h_name_off.grow((size_t)n + 1, 1024));
    FPL_HIP(hipStreamWaitEvent(ctx->stream, sl.ev_parsed, 0));
    bam_launch(b.d_bam.ptr, b.d_rec.ptr, sl.d_off.ptr, n, 0, h.n_bases, sl.d_seq.ptr, sl.d_qual.ptr, ctx->stream);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipEventRecord(sl.ev_parsed, ctx->stream)); /* (from here on: the bases are decoded, as for a BAM batch) */
    FPL_HIP(hipMemcpyAsync(b.h_names.ptr, b.d_names.ptr, (size_t)h.name_bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
    FPL_HIP(hipMemcpyAsync(b.h_name_off.ptr, b.d_name_off.ptr, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->s_d2h));
    return submit_tail(ctx, sl, sl.ev_parsed, n, h.n_bases, h.max_read_len);
}

int fpl_peek_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl;
    FPL_TRY(peek_pending(ctx, BatchKind::BGZF, sl, out, sizeof(*out)));
    *out = *sl->bam.h_whdr.ptr;
    return FPL_OK;
}

int fpl_start_bgzf_bam(fpl_ctx* ctx, uint8_t* seq_out, uint8_t* qual_out) {
    if (!ctx || (!seq_out) != (!qual_out)) return FPL_ERR_ARG;
    return start_pending(ctx, BatchKind::BGZF, seq_out, qual_out);
}

int fpl_wait_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out, const fpl_read_result** results, const uint8_t** names, const uint64_t** name_off,
                      const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out || (!gz) != (!gz_len)) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(wait_front(ctx, kind_bit(BatchKind::BGZF), slp)); /* (the others: fpl_wait, fpl_wait_text) */
    fpl_ctx::Slot& sl = *slp;
    memset(out, 0, sizeof(*out));
    if (results) *results = nullptr;
    if (names) *names = nullptr;
    if (name_off) *name_off = nullptr;
    if (gz) {
        *gz = nullptr;
        *gz_len = 0;
    }
    FPL_TRY(wait_staged(ctx, sl)); /* (stage 2: a no-op when fpl_start_bgzf_bam did it) */
    *out = *sl.bam.h_whdr.ptr;
    if (out->status != FPL_BAMW_OK || sl.n_reads == 0) return FPL_OK;
    FPL_TRY(wait_finish(ctx, sl, gz, gz_len));
    if (results) *results = sl.h_results.ptr;
    if (names) *names = sl.bam.h_names.ptr;
    if (name_off) *name_off = sl.bam.h_name_off.ptr;
    return FPL_OK;
}

/* (the recovery calls, shared by the BGZF BAM and the BGZF text path, run with no batch of either kind in flight: every walk is
   done -- its header was waited for -- and the state is at rest) */
int fpl_bam_tail_get(fpl_ctx* ctx, uint8_t* buf, uint64_t cap, uint64_t* len) {
    if (!ctx || !len) return FPL_ERR_ARG;
    *len = 0;
    if (bgzf_in_flight(ctx)) return FPL_ERR_STATE;
    if (!ctx->d_bamw_state.ptr) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    BamWalkState st;
    FPL_HIP(hipMemcpy(&st, ctx->d_bamw_state.ptr, sizeof(st), hipMemcpyDeviceToHost));
    const uint64_t n = std::min<uint64_t>(st.tail_len, ctx->bam_tail_cap);
    *len = n;
    if (n > cap || (n && !buf)) return FPL_ERR_ARG;
    if (n) FPL_HIP(hipMemcpy(buf, ctx->d_bam_tail.ptr, (size_t)n, hipMemcpyDeviceToHost));
    return FPL_OK;
}
static int bam_state_update(fpl_ctx* ctx, bool set_tail, uint64_t tail_len) {
    FPL_TRY(ensure_bam_tail(ctx));
    BamWalkState st;
    FPL_HIP(hipMemcpy(&st, ctx->d_bamw_state.ptr, sizeof(st), hipMemcpyDeviceToHost));
    st.refused = 0;
    if (set_tail) {
        st.tail_len = (u32)tail_len;
        if (tail_len == 0) st.rec_base = 0;
    }
    FPL_HIP(hipMemcpy(ctx->d_bamw_state.ptr, &st, sizeof(st), hipMemcpyHostToDevice));
    ctx->bam_fresh = st.tail_len == 0; /* (a refused first stretch left none: it is submitted again with its skip) */
    return FPL_OK;
}
int fpl_bam_tail_set(fpl_ctx* ctx, const uint8_t* bytes, uint64_t len) {
    if (!ctx || (len && !bytes) || len > ctx->bam_tail_cap) return FPL_ERR_ARG;
    if (bgzf_in_flight(ctx)) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_TRY(bam_state_update(ctx, true, len));
    if (len) FPL_HIP(hipMemcpy(ctx->d_bam_tail.ptr, bytes, (size_t)len, hipMemcpyHostToDevice));
    return FPL_OK;
}
int fpl_resume_bgzf_bam(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    if (bgzf_in_flight(ctx)) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    return bam_state_update(ctx, false, 0);
}
int fpl_reserve_bam_tail(fpl_ctx* ctx, uint64_t bytes) {
    if (!ctx || bytes > (1ull << 30)) return FPL_ERR_ARG;
    if (bgzf_in_flight(ctx)) return FPL_ERR_STATE;
    if (!ctx->d_bam_tail.ptr) { /* before the first use: exactly what was asked for */
        ctx->bam_tail_cap = bytes;
        return FPL_OK;
    }
    if (bytes <= ctx->bam_tail_cap) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    DevBuf<u8> nw;
    FPL_HIP(nw.alloc((size_t)bytes));
    if (ctx->bam_tail_cap) FPL_HIP(hipMemcpy(nw.ptr, ctx->d_bam_tail.ptr, (size_t)ctx->bam_tail_cap, hipMemcpyDeviceToDevice));
    ctx->d_bam_tail.swap(nw); /* (the old block goes with nw) */
    ctx->bam_tail_cap = bytes;
    return FPL_OK;
}
