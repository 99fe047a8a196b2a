/* rt_text.h -- FASTQ text in (ABI v7; text_parse.h): a staged kind of rt_slots.h.  Stage 1 uploads and parses a chunk, stage 2 runs
   the per-read kernels on what the parse found. */
#pragma once

static int ensure_text_slot(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint64_t n_bytes) {
    fpl_ctx::Slot::Text& t = sl.text;
    FPL_TRY(ensure_slot(ctx, sl, (u32)(n_bytes / 64 + 16), n_bytes / 2 + 64, false));
    if (!t.d_hdr.ptr) {
        FPL_HIP(t.d_hdr.alloc(1));
        FPL_HIP(t.h_hdr.alloc(1));
    }
    if (!t.d_text.holds(n_bytes + 16)) {
        const size_t cap = grown(n_bytes, 4096), rc = cap / 64 + 16;
        FPL_HIP(regrow(t.d_text.want(cap + 16), t.d_nl.want(4 * rc), t.d_blk.want(cap / TP_BLOCK_BYTES + 2), t.d_line.want(4 * rc),
                       t.d_len.want(rc)));
    }
    return FPL_OK;
}

/* stage 2 of a text batch (slot_continue): the header is in -- enqueue the per-read kernels and the way back of the records and line starts */
static int text_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl) {
    const TextHeader h = *sl.text.h_hdr.ptr;
    if (h.status != 0 || h.n_records == 0) return FPL_OK; /* nothing to run: fpl_wait_text reports */
    const u32 n = h.n_records;
    if (!sl.text.h_line.holds(4 * (size_t)n)) FPL_HIP(regrow(sl.text.h_line.want(4 * grown(n, 16))));
    FPL_HIP(sl.h_results.grow(n, 1024));
    return submit_tail(ctx, sl, sl.ev_parsed, n, h.n_bases, h.max_len);
}
int fpl_process_text_async(fpl_ctx* ctx, const uint8_t* text, uint64_t n_bytes) {
    if (!ctx || (n_bytes && !text)) return FPL_ERR_ARG;
    if (n_bytes > 0xFFFFFFF0ull) return FPL_ERR_ARG; /* (line positions are 32 bits wide: cut the file in smaller chunks) */
    fpl_ctx::Slot* slp;
    FPL_TRY(slot_begin(ctx, BatchKind::Text, ctx->text_gzip, slp));
    fpl_ctx::Slot& sl = *slp;
    fpl_ctx::Slot::Text& t = sl.text;
    t.bytes = n_bytes;
    FPL_TRY(ensure_host_streams(ctx));
    FPL_TRY(ensure_text_slot(ctx, sl, n_bytes));
    if (n_bytes == 0) {
        memset(t.h_hdr.ptr, 0, sizeof(TextHeader));
        t.h_hdr.ptr->bad_record = ~0ull;
        return slot_commit(ctx, sl, FPL_OK, 2); /* (nothing to enqueue) */
    }
    auto enqueue = [&]() -> int {
        /* the upload on the copy stream, the parse on a stream of its own behind it: the NEXT chunk's upload starts the moment this
           one's is done (with the parse on the copy stream the link sat idle for 140 us between two uploads of 590) */
        u8* const d_text = t.d_text.ptr;
        u32 *const d_nl = t.d_nl.ptr, *const d_blk = t.d_blk.ptr, *const d_line = t.d_line.ptr, *const d_len = t.d_len.ptr;
        TextHeader* const d_hdr = t.d_hdr.ptr;
        FPL_HIP(hipMemcpyAsync(d_text, text, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        hipStream_t st = ctx->s_parse;
        FPL_HIP(hipStreamWaitEvent(st, sl.ev_h2d, 0));
        FPL_HIP(hipMemsetAsync(d_hdr, 0, sizeof(TextHeader), st));
        FPL_HIP(hipMemsetAsync(&d_hdr->bad_record, 0xFF, sizeof(u64), st));
        const u32 nblk = (u32)((n_bytes + TP_BLOCK_BYTES - 1) / TP_BLOCK_BYTES);
        const u32 rec_cap = (u32)(n_bytes / 64 + 16);
        hipLaunchKernelGGL(k_text_count, dim3(nblk), dim3(TP_THREADS), 0, st, (const u8*)d_text, (u64)n_bytes, d_blk, d_hdr);
        hipLaunchKernelGGL(k_text_scan, dim3(1), dim3(1024), 0, st, d_blk, nblk, d_hdr);
        hipLaunchKernelGGL(k_text_fill, dim3(nblk), dim3(TP_THREADS), 0, st, (const u8*)d_text, (u64)n_bytes, (const u32*)d_blk, d_nl,
                           4 * rec_cap);
        const u32 rblk = std::min<u32>(std::max<u32>(1u, (rec_cap + 255u) / 256u), 4u * ctx->n_cu);
        hipLaunchKernelGGL(k_text_records, dim3(rblk), dim3(256), 0, st, (const u8*)d_text, (u64)n_bytes, (const u32*)d_nl, rec_cap,
                           d_hdr, d_line, d_len);
        hipLaunchKernelGGL(k_text_offsets, dim3(1), dim3(1024), 0, st, (const u32*)d_len, rec_cap, d_hdr, sl.d_off.ptr);
        hipLaunchKernelGGL(k_text_gather, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)d_text, (const u32*)d_line,
                           (const u32*)d_len, (const uint64_t*)sl.d_off.ptr, (const TextHeader*)d_hdr, rec_cap, sl.d_seq.ptr, sl.d_qual.ptr);
        FPL_HIP(hipGetLastError());
        FPL_HIP(hipMemcpyAsync(t.h_hdr.ptr, d_hdr, sizeof(TextHeader), hipMemcpyDeviceToHost, st));
        FPL_HIP(hipEventRecord(sl.ev_parsed, st));
        return FPL_OK;
    };
    return slot_commit(ctx, sl, enqueue(), 1);
}

static void text_info(const fpl_ctx::Slot& sl, fpl_text_result* out) {
    const TextHeader& h = *sl.text.h_hdr.ptr;
    memset(out, 0, sizeof(*out));
    out->n_lines = h.n_lines;
    out->bad_record = h.bad_record;
    out->status = (h.status & 1u) ? FPL_TEXT_IRREGULAR : (h.status & 2u) ? FPL_TEXT_TOO_MANY : FPL_TEXT_OK;
    if (out->status == FPL_TEXT_OK) {
        out->n_reads = h.n_records;
        out->n_bases = h.n_bases;
        out->max_read_len = h.max_len;
    }
}

int fpl_peek_text(fpl_ctx* ctx, fpl_text_result* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl;
    FPL_TRY(peek_pending(ctx, BatchKind::Text, sl, out, sizeof(*out)));
    text_info(*sl, out);
    return FPL_OK;
}

int fpl_start_text(fpl_ctx* ctx) { return ctx ? start_pending(ctx, BatchKind::Text, nullptr, nullptr) : FPL_ERR_ARG; }

int fpl_cancel_text(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl;
    FPL_TRY(pending_begin(ctx, BatchKind::Text, sl, nullptr, 0, false));
    if (sl->rc == FPL_OK) FPL_HIP(hipEventSynchronize(sl->ev_parsed)); /* (its copy and parse read the caller's text) */
    sl->cancelled = true;
    sl->n_reads = 0;
    return FPL_OK;
}

int fpl_set_text_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->text_gzip = on != 0;
    return FPL_OK;
}

int fpl_set_gzip_framing(fpl_ctx* ctx, int framing) {
    if (!ctx || (framing != FPL_GZIP_MEMBER && framing != FPL_GZIP_BGZF)) return FPL_ERR_ARG;
    ctx->gzip_bgzf = framing == FPL_GZIP_BGZF; /* (read by slot_begin: the next submission's slot) */
    return FPL_OK;
}

int fpl_set_gzip_records(fpl_ctx* ctx, int records) {
    if (!ctx || (records != FPL_GZIP_FASTQ && records != FPL_GZIP_BAM)) return FPL_ERR_ARG;
    if (records == FPL_GZIP_BAM && ctx->hcfg.defer && ctx->frag_out) return FPL_ERR_STATE; /* (the record form stays with the host in fragment mode) */
    ctx->gzip_records = records == FPL_GZIP_BAM; /* (read by slot_begin, like the framing) */
    return FPL_OK;
}

int fpl_set_bam_tags(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    if (on && ctx->hcfg.defer && ctx->frag_out) return FPL_ERR_STATE; /* (as the record form) */
    ctx->bam_tags = on != 0; /* (read by slot_begin, like the framing; a slot that holds no BAM records ignores it) */
    return FPL_OK;
}

int fpl_set_bam_mods(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->bam_mods = on != 0; /* (read by slot_begin; without fpl_set_bam_tags it changes nothing) */
    return FPL_OK;
}

int fpl_set_bam_comments(fpl_ctx* ctx, const char* tags, int n_tags) {
    if (!ctx || (n_tags > 0 && !tags)) return FPL_ERR_ARG;
    bamcomment::Selection s;
    if (!bamcomment::make_selection(tags, n_tags, s)) return FPL_ERR_ARG;
    if (s.n != 0 && ctx->hcfg.defer && ctx->frag_out) return FPL_ERR_STATE; /* (as the record form) */
    ctx->bam_comments = s; /* (read by slot_begin, like the framing; a slot whose gzip bytes are not the FASTQ text of BAM records ignores it) */
    return FPL_OK;
}

int fpl_set_bam_moves(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->bam_moves = on != 0; /* (read by slot_begin; without fpl_set_bam_tags it changes nothing) */
    return FPL_OK;
}

static int wait_text(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                     const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(wait_front(ctx, kind_bit(BatchKind::Text), slp)); /* (a CSR or BAM batch: fpl_wait) */
    fpl_ctx::Slot& sl = *slp;
    memset(out, 0, sizeof(*out));
    if (results) *results = nullptr;
    if (line_starts) *line_starts = nullptr;
    FPL_TRY(wait_staged(ctx, sl)); /* (stage 2: a no-op when fpl_start_text did it) */
    if (sl.cancelled) {
        out->status = FPL_TEXT_CANCELLED;
        out->bad_record = ~0ull;
        return FPL_OK;
    }
    text_info(sl, out);
    if (out->status != FPL_TEXT_OK || sl.n_reads == 0) return FPL_OK;
    FPL_TRY(wait_finish(ctx, sl, gz, gz_len));
    if (results) *results = sl.h_results.ptr;
    if (line_starts) *line_starts = sl.text.h_line.ptr;
    return FPL_OK;
}
int fpl_wait_text(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts) {
    return wait_text(ctx, out, results, line_starts, nullptr, nullptr);
}
int fpl_wait_text_gz(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                     const uint8_t** gz, uint64_t* gz_len) {
    if (!gz || !gz_len) return FPL_ERR_ARG;
    *gz = nullptr;
    *gz_len = 0;
    return wait_text(ctx, out, results, line_starts, gz, gz_len);
}
