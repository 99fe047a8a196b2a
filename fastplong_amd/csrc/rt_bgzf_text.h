/* rt_bgzf_text.h -- a FASTQ's BGZF blocks in, records out (text_walk.h): a staged kind of rt_slots.h whose text is inflated,
   cut at a record's end and parsed on the device.  The tail between two submissions, its capacity, the refusal flag and the
   recovery calls are rt_bam.h's. */
#pragma once

int fpl_process_bgzf_text_async(fpl_ctx* ctx, const uint8_t* comp, uint64_t comp_bytes, const fpl_bgzf_block* blocks, uint32_t n_blocks) {
    if (!ctx || (n_blocks && !blocks) || (comp_bytes && !comp)) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(slot_begin(ctx, BatchKind::BGZFText, ctx->text_gzip, slp));
    if (!ctx->bam_fresh && ctx->tail_kind != BatchKind::BGZFText) {
        ctx->err = "fpl_process_bgzf_text_async: the context holds the tail of BGZF BAM submissions";
        return FPL_ERR_STATE;
    }
    uint64_t total = 0;
    if (!bgzf_blocks_ok(blocks, n_blocks, comp_bytes, nullptr, &total)) return FPL_ERR_ARG;
    TextWalkJob j;
    if (!text_walk_plan(j, ctx->bam_tail_cap, total)) return FPL_ERR_ARG;
    fpl_ctx::Slot& sl = *slp;
    fpl_ctx::Slot::Text& t = sl.text;
    fpl_ctx::Slot::Bam& b = sl.bam;
    const uint64_t hi = j.tail_cap + total;
    t.bytes = hi; /* (what the gzip layout's bound is made of) */
    b.o_begin = b.bases = 0;
    b.seq_out = b.qual_out = nullptr;
    FPL_TRY(ensure_host_streams(ctx));
    FPL_TRY(ensure_bam_tail(ctx));
    FPL_TRY(ensure_text_slot(ctx, sl, hi)); /* (d_off / d_results / d_nl / d_line / d_len hold rec_cap and more) */
    if (!t.d_whdr.ptr) {
        FPL_HIP(t.d_whdr.alloc(1));
        FPL_HIP(t.h_whdr.alloc(1));
        FPL_HIP(t.d_ws.alloc(1));
    }
    if (!b.d_next.ptr) FPL_HIP(b.d_next.alloc(1));
    FPL_HIP(t.d_nlen.grow(j.rec_cap, 16));
    FPL_HIP(b.d_name_off.grow((size_t)j.rec_cap + 1, 16));
    FPL_HIP(b.d_names.grow((size_t)bam_names_cap(hi) + 1, 4096));
    FPL_HIP(b.d_comp.grow((size_t)comp_bytes + 1, 4096));
    FPL_HIP(b.d_blocks.grow((size_t)n_blocks + 1, 64));
    j.buf = t.d_text.ptr;
    j.st = ctx->d_bamw_state.ptr;
    j.tail_buf = ctx->d_bam_tail.ptr;
    j.blocks = b.d_blocks.ptr;
    j.n_blocks = n_blocks;
    j.blk = t.d_blk.ptr;
    j.nl_pos = t.d_nl.ptr;
    j.line = t.d_line.ptr;
    j.len = t.d_len.ptr;
    j.nlen = t.d_nlen.ptr;
    j.ws = t.d_ws.ptr;
    j.hdr = t.d_whdr.ptr;
    j.off = sl.d_off.ptr;
    j.name_off = b.d_name_off.ptr;
    j.names = b.d_names.ptr;
    j.names_cap = bam_names_cap(hi);
    j.seq = sl.d_seq.ptr;
    j.qual = sl.d_qual.ptr;
    j.seq_cap = hi / 2 + 64; /* (what ensure_text_slot sized them for: a regular record has as many qualities as bases) */
    auto enqueue = [&]() -> int {
        /* the upload on the copy stream; inflate and walk on the parse stream behind it, and behind the walk of the submission
           before -- that order carries the tail; only the header comes back */
        if (comp_bytes) FPL_HIP(hipMemcpyAsync(b.d_comp.ptr, comp, comp_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        if (n_blocks) FPL_HIP(hipMemcpyAsync(b.d_blocks.ptr, blocks, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        hipStream_t st = ctx->s_parse;
        FPL_HIP(hipStreamWaitEvent(st, sl.ev_h2d, 0));
        if (n_blocks) FPL_HIP(bgzf_inflate_enqueue(b.d_comp.ptr, b.d_blocks.ptr, n_blocks, t.d_text.ptr + j.tail_cap, b.d_next.ptr, ctx->n_cu, st));
        text_walk_enqueue(j, 8 * ctx->n_cu, st);
        FPL_HIP(hipGetLastError());
        FPL_HIP(hipMemcpyAsync(t.h_whdr.ptr, t.d_whdr.ptr, sizeof(fpl_text_window), hipMemcpyDeviceToHost, st));
        FPL_HIP(hipEventRecord(sl.ev_parsed, st));
        return FPL_OK;
    };
    const int r = slot_commit(ctx, sl, enqueue(), 1);
    if (r == FPL_OK) {
        ctx->bam_fresh = false;
        ctx->tail_kind = BatchKind::BGZFText;
    }
    return r;
}

/* stage 2 of a BGZF text batch (slot_continue): the header is in -- the per-read kernels on the slot's CSR arrays, the way back of
   the names and, where the caller gave arrays, of the bases and qualities */
static int bgzf_text_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out) {
    fpl_ctx::Slot::Bam& b = sl.bam;
    const fpl_text_window h = *sl.text.h_whdr.ptr;
    if (h.status != FPL_TXTW_OK || h.n_reads == 0) return FPL_OK; /* nothing to run: the wait reports */
    const u32 n = h.n_reads;
    FPL_HIP(sl.h_results.grow(n, 1024));
    FPL_HIP(b.h_names.grow((size_t)h.name_bytes + 1, 4096));
    FPL_HIP(b.h_name_off.grow((size_t)n + 1, 1024));
    FPL_HIP(hipStreamWaitEvent(ctx->s_d2h, sl.ev_parsed, 0));
    if (h.name_bytes) FPL_HIP(hipMemcpyAsync(b.h_names.ptr, b.d_names.ptr, (size_t)h.name_bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
    FPL_HIP(hipMemcpyAsync(b.h_name_off.ptr, b.d_name_off.ptr, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->s_d2h));
    if (seq_out && h.n_bases) {
        FPL_HIP(hipMemcpyAsync(seq_out, sl.d_seq.ptr, (size_t)h.n_bases, hipMemcpyDeviceToHost, ctx->s_d2h));
        FPL_HIP(hipMemcpyAsync(qual_out, sl.d_qual.ptr, (size_t)h.n_bases, hipMemcpyDeviceToHost, ctx->s_d2h));
    }
    return submit_tail(ctx, sl, sl.ev_parsed, n, h.n_bases, h.max_read_len); /* (its ev_done, on the way-back stream, is behind these copies) */
}

int fpl_peek_bgzf_text(fpl_ctx* ctx, fpl_text_window* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl;
    FPL_TRY(peek_pending(ctx, BatchKind::BGZFText, sl, out, sizeof(*out)));
    *out = *sl->text.h_whdr.ptr;
    return FPL_OK;
}

int fpl_start_bgzf_text(fpl_ctx* ctx, uint8_t* seq_out, uint8_t* qual_out) {
    if (!ctx || (!seq_out) != (!qual_out)) return FPL_ERR_ARG;
    return start_pending(ctx, BatchKind::BGZFText, seq_out, qual_out);
}

int fpl_wait_bgzf_text(fpl_ctx* ctx, fpl_text_window* out, const fpl_read_result** results, const uint8_t** names, const uint64_t** name_off,
                       const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out || (!gz) != (!gz_len)) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(wait_front(ctx, kind_bit(BatchKind::BGZFText), slp)); /* (the others: fpl_wait, fpl_wait_text, fpl_wait_bgzf_bam) */
    fpl_ctx::Slot& sl = *slp;
    memset(out, 0, sizeof(*out));
    if (results) *results = nullptr;
    if (names) *names = nullptr;
    if (name_off) *name_off = nullptr;
    if (gz) {
        *gz = nullptr;
        *gz_len = 0;
    }
    FPL_TRY(wait_staged(ctx, sl)); /* (stage 2: a no-op when fpl_start_bgzf_text did it) */
    *out = *sl.text.h_whdr.ptr;
    if (out->status != FPL_TXTW_OK || sl.n_reads == 0) return FPL_OK;
    FPL_TRY(wait_finish(ctx, sl, gz, gz_len));
    if (results) *results = sl.h_results.ptr;
    if (names) *names = sl.bam.h_names.ptr;
    if (name_off) *name_off = sl.bam.h_name_off.ptr;
    return FPL_OK;
}
