/* rt_batch.h -- one batch whose reads are on the device: the workspaces it needs (every ensure_*), fpl_process_batch_device (the
   per-read kernels, pipeline.h) and fpl_emit_batch_device (emit.h). */
#pragma once

/* (every ensure_*: a group sized by one number grows together behind one device-wide wait, with a quarter of headroom) */
static int ensure_scratch(fpl_ctx* ctx, u32 n_reads, uint64_t n_bytes, u32 max_read_len) {
    const size_t slabs = stats_scratch_slabs(n_reads, n_bytes, max_read_len, ctx->n_cu, ctx->tune);
    if (ctx->d_stats_scratch.holds(slabs * (size_t)FS_SLAB)) return FPL_OK;
    const size_t cap = grown(slabs, 0);
    FPL_HIP(regrow(ctx->d_stats_scratch.want(cap * (size_t)FS_SLAB),
                   ctx->d_stats_flags.want(2 * cap + 64))); /* slab flags + tile flags: tiles <= slabs, whatever the shape */
    return FPL_OK;
}

/* slabs of the post-only pass when it has a stream of its own: FS_EXTRA_BLOCKS per cycle tile */
static int ensure_extra_scratch(fpl_ctx* ctx, u32 n_reads, u32 max_read_len, bool sorted) {
    if (!ctx->overlap || ctx->hcfg.defer) return FPL_OK;
    /* only the sorted pass forks the post-only pass onto the side stream; a batch that takes the plain walk needs none of this */
    if (!sorted) return FPL_OK;
    const u32 n_tiles = cdiv(max_read_len ? max_read_len : 1, FS_T);
    const size_t slabs = (size_t)stats_extra_blocks(n_reads, ctx->tune) * n_tiles;
    if (ctx->d_extra_scratch.holds(slabs * (size_t)FS_SLAB)) return FPL_OK;
    const size_t cap = grown(slabs, 0);
    FPL_HIP(regrow(ctx->d_extra_scratch.want(cap * (size_t)FS_SLAB), ctx->d_extra_flags.want(2 * cap + 64))); /* (slab flags + tile flags) */
    return FPL_OK;
}

static int ensure_sort_ws(fpl_ctx* ctx, u32 n_reads, uint64_t n_bytes) {
    const u32 per = stats_items_per_slice(n_reads, n_reads ? (u32)(n_bytes / n_reads) : 0, ctx->n_cu, ctx->tune);
    FPL_HIP(ctx->d_sort_ws.grow(sort_ws_words(stats_sorted_max_slices(n_reads, per, ctx->tune), n_reads), 0));
    return FPL_OK;
}

/* the fragment / region / piece lists of k_break_mask: capacities grow (25 % headroom) and never shrink -- when one list is too
   small all are made anew, none below what it had --, so that a run whose batches differ a little in size does not reallocate
   -- and wait for the device -- on every batch */
static int ensure_break_mask(fpl_ctx* ctx, u32 n_reads, uint64_t n_bytes) {
    if (!ctx->hcfg.defer) return FPL_OK;
    if (!ctx->d_bm_counts.ptr) FPL_HIP(ctx->d_bm_counts.alloc(4));
    u32 need_f = 0, need_r = 0, need_i = 0;
    break_mask_caps(n_reads, n_bytes, ctx->hcfg.brk, ctx->hcfg.brk_w, ctx->hcfg.msk, ctx->hcfg.msk_w, need_f, need_r, need_i);
    if (ctx->d_bm_frags.holds(need_f) && need_r <= ctx->d_bm_regs.cap && need_i <= ctx->d_frag_cyc.cap) return FPL_OK;
    const size_t frag_cap = std::max(ctx->d_bm_frags.cap, grown(need_f, 64, 0x7FFFFFF0u));
    const size_t reg_cap = std::max(ctx->d_bm_regs.cap, grown(need_r, 64, 0x7FFFFFF0u));
    const size_t item_cap = std::max(ctx->d_frag_cyc.cap, grown(need_i, 64, 0x7FFFFFF0u));
    FPL_HIP(regrow(ctx->d_bm_frags.want(frag_cap), ctx->d_bm_regs.want(reg_cap), ctx->d_frag_off.want(item_cap),
                   ctx->d_frag_len.want(item_cap), ctx->d_frag_cyc.want(item_cap)));
    return FPL_OK;
}

static int ensure_workspace(fpl_ctx* ctx, u32 n_reads) {
    if (ctx->d_state.holds(n_reads)) return FPL_OK;
    /* 25 % headroom, as the other workspaces: a host that cuts its input by BYTES hands in batches whose read counts wander by a few
       per cent, and every new record used to cost a device-wide wait, a dozen hipFree and as many hipMalloc -- 3 to 9 ms each, five or
       six times in the first 60 ms of a run (rocprofv3 timeline of the CLI, tools/cli_timeline.sh) */
    const size_t cap = grown(n_reads, 1024);
    if (ctx->hcfg.defer) /* (with --break / --mask the item list is sized by ensure_break_mask) */
        FPL_HIP(regrow(ctx->d_state.want(cap), ctx->d_state2.want(cap), ctx->d_wins.want(cap), ctx->d_recs.want(cap), ctx->d_redo.want(cap),
                       ctx->d_st_off.want(cap), ctx->d_st_len.want(cap), ctx->d_st_e.want(cap)));
    else
        FPL_HIP(regrow(ctx->d_state.want(cap), ctx->d_state2.want(cap), ctx->d_wins.want(cap), ctx->d_recs.want(cap), ctx->d_redo.want(cap),
                       ctx->d_st_off.want(cap), ctx->d_st_len.want(cap), ctx->d_st_e.want(cap), ctx->d_frag_off.want(2 * cap),
                       ctx->d_frag_len.want(2 * cap)));
    return FPL_OK;
}

int fpl_process_batch_device(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off,
                             uint32_t n_reads, uint64_t n_bytes, uint32_t max_read_len, fpl_read_result* d_results,
                             void* stream_v) {
    if (!ctx) return FPL_ERR_ARG;
    if (n_reads && (!d_seq || !d_qual || !d_off || !d_results)) return FPL_ERR_ARG;
    if (n_reads > 0x7FFFFFFFu / 2) return FPL_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_v;
    FPL_HIP(hipSetDevice(ctx->device));
    if (max_read_len > ctx->C) {
        /* (a quarter more than asked for: the longest read so far is a record that keeps being broken by a little, and every
           growth waits for the device and moves the counters) */
        const uint64_t want = (uint64_t)max_read_len + max_read_len / 4;
        FPL_TRY(fpl_reserve_cycles(ctx, want > 0x7FFFFFFFull ? max_read_len : (u32)want));
    }
    /* which statistics pass the batch takes: asked ONCE -- the side stream's slabs, the launch sequence and the form counters all
       follow this one answer (a drift between separate askings would size the slabs for one form and launch the other) */
    const bool sorted_form = n_reads && stats_takes_sorted(n_reads, n_bytes, max_read_len, ctx->n_cu, ctx->tune, ctx->hcfg.defer != 0);
    if (n_reads) {
        FPL_TRY(ensure_workspace(ctx, n_reads));
        FPL_TRY(ensure_scratch(ctx, n_reads, n_bytes, max_read_len));
        FPL_TRY(ensure_extra_scratch(ctx, n_reads, max_read_len, sorted_form));
        FPL_TRY(ensure_sort_ws(ctx, n_reads, n_bytes));
        FPL_TRY(ensure_break_mask(ctx, n_reads, n_bytes));
    }
    /* which of the two ReadState[] / work-counter sets this batch takes, and whether its end trims start ahead of the main stream */
    const int par = (int)(ctx->batch_no & 1);
    u32* const work_ctr = ctx->d_work_ctr.ptr + par * WORK_CTR_WORDS;
    hipEvent_t inputs_ev = ctx->next_inputs_event;
    ctx->next_inputs_event = nullptr;
    const bool ahead = n_reads && ctx->trim_ahead && ctx->overlap && !ctx->dbg && !ctx->hcfg.defer && ctx->batch_no > 0 &&
                       (inputs_ev || ctx->inputs_ready) && trim_worth_ahead(n_reads, ctx->tune);
    if (n_reads) {
        if (ahead) {
            /* the set was last used two batches ago; the trims also wait for this batch's inputs when an event says when they are in */
            FPL_HIP(hipStreamWaitEvent(ctx->s_trim, ctx->ev_batch_done[par], 0));
            if (ctx->ahead_gate) FPL_HIP(hipStreamWaitEvent(ctx->s_trim, ctx->ev_stats_done[par ^ 1], 0)); /* (the batch before this one) */
            if (inputs_ev) FPL_HIP(hipStreamWaitEvent(ctx->s_trim, inputs_ev, 0));
            FPL_HIP(hipMemsetAsync(work_ctr, 0, WORK_CTR_WORDS * sizeof(u32), ctx->s_trim));
        } else {
            FPL_HIP(hipMemsetAsync(work_ctr, 0, WORK_CTR_WORDS * sizeof(u32), stream));
        }
    }
    if (ctx->hcfg.defer && ctx->d_bm_counts.ptr) FPL_HIP(hipMemsetAsync(ctx->d_bm_counts.ptr, 0, 4 * sizeof(u32), stream));
    BatchArgs a;
    a.seq = d_seq;
    a.qual = d_qual;
    a.off = d_off;
    a.n_reads = n_reads;
    a.n_bytes = n_bytes;
    a.max_read_len = max_read_len;
    a.cfg = ctx->d_cfg.ptr;
    a.ads = ctx->d_ads.ptr;
    a.state = par ? ctx->d_state2.ptr : ctx->d_state.ptr;
    if (ctx->trim_ahead && ctx->overlap) a.ev_stats_done = ctx->ev_stats_done[par].h;
    if (ahead) {
        a.trim_stream = ctx->s_trim;
        a.ev_trim_done = ctx->ev_trim_done.h;
    }
    a.results = d_results;
    a.frag_off = ctx->d_frag_off.ptr;
    a.frag_len = ctx->d_frag_len.ptr;
    a.frag_cyc = ctx->d_frag_cyc.ptr;
    a.bm = BmLists{ctx->d_bm_frags.ptr, ctx->d_bm_regs.ptr, (u32)ctx->d_bm_frags.cap, (u32)ctx->d_bm_regs.cap, (u32)ctx->d_frag_cyc.cap,
                     ctx->d_bm_counts.ptr};
    a.defer = ctx->hcfg.defer != 0;
    a.trim_mode = ctx->hcfg.trim_mode;
    a.n_fasta = ctx->hcfg.n_fasta;
    a.scan_short = ctx->hcfg.scan_short != 0;
    a.counters = ctx->d_counters.ptr;
    a.C = ctx->C;
    a.work_ctr = work_ctr;
    a.recs = ctx->d_recs.ptr;
    a.wins = ctx->d_wins.ptr;
    a.redo = ctx->d_redo.ptr;
    a.sort_ws = ctx->d_sort_ws.ptr;
    a.st_off = ctx->d_st_off.ptr;
    a.st_len = ctx->d_st_len.ptr;
    a.st_e = ctx->d_st_e.ptr;
    a.stats_scratch = ctx->d_stats_scratch.ptr;
    a.stats_flags = ctx->d_stats_flags.ptr;
    if (ctx->overlap && ctx->d_extra_scratch.ptr) {
        a.extra_scratch = ctx->d_extra_scratch.ptr;
        a.extra_flags = ctx->d_extra_flags.ptr;
        a.aux = ctx->s_aux;
        a.ev_fork = ctx->ev_fork.h;
        a.ev_join = ctx->ev_join.h;
    }
    a.n_cu = ctx->n_cu;
    a.sorted_form = sorted_form ? 1 : 0;
    a.dbg = ctx->dbg;
    if ((a.dbg & 0xA000) && !ctx->probe_primed) { /* (profiling only: the first batch of a back-only / scan-only context runs whole) */
        a.dbg &= ~0xB000;
        ctx->probe_primed = true;
    }
    a.tune = ctx->tune;
    if (n_reads) { /* which forms this batch takes (the same predicates enqueue_batch asks) */
        ctx->forms[0]++;
        ctx->forms[1] += n_reads;
        ctx->forms[2] += trim_takes_batched(n_reads, a.trim_mode, a.tune) ? 1 : 0;
        ctx->forms[3] += sorted_form ? 1 : 0;
        if (n_reads > ctx->forms[4]) ctx->forms[4] = n_reads;
        ctx->forms[5] += ahead ? 1 : 0;
    }
    const bool timing = ctx->timing != 0;
    const int slot = ctx->ev_calls % fpl_ctx::EV_RING;
    hipError_t ev_err = hipSuccess;
    enqueue_batch(a, stream, [&](int i) {
        if (timing) {
            hipError_t e = hipEventRecord(ctx->ev[slot][i], stream);
            if (e != hipSuccess) ev_err = e;
        }
    });
    FPL_HIP(hipGetLastError());
    FPL_HIP(ev_err);
    if (n_reads) {
        FPL_HIP(hipEventRecord(ctx->ev_batch_done[par], stream));
        ctx->batch_no++;
    }
    if (timing) ctx->ev_calls++;
    return FPL_OK;
}

/* fpl_set_fragment_output: the order of the last batch's fragment list (csrc/frag_index.h), enqueued on `st` behind the kernels
   that wrote the list.  Sized by the list's capacity: how many fragments there are only the device knows. */
static int frag_index(fpl_ctx* ctx, u32 n_reads, hipStream_t st) {
    if (!ctx->d_bm_frags.ptr || !ctx->d_bm_counts.ptr) { /* (no batch has run yet) */
        ctx->err = "fragment output: the context has no fragment list yet";
        return FPL_ERR_STATE;
    }
    const size_t frag_cap = ctx->d_bm_frags.cap;
    if (!ctx->d_fi.ptr) FPL_HIP(ctx->d_fi.alloc(1));
    if (!ctx->d_fi_cnt.holds((size_t)n_reads + 1)) {
        const size_t cap = grown((size_t)n_reads + 1, 1024);
        FPL_HIP(regrow(ctx->d_fi_cnt.want(cap), ctx->d_fi_first.want(cap)));
    }
    if (!ctx->d_fi_order.holds(frag_cap)) FPL_HIP(regrow(ctx->d_fi_order.want(frag_cap)));
    FPL_HIP(hipMemsetAsync(ctx->d_fi.ptr, 0, sizeof(FragIndex), st));
    FPL_HIP(hipMemsetAsync(ctx->d_fi_cnt.ptr, 0, sizeof(u32) * ((size_t)n_reads + 1), st));
    FPL_HIP(hipMemsetAsync(ctx->d_fi_order.ptr, 0xFF, sizeof(u32) * frag_cap, st));
    const dim3 grid(frag_index_blocks(frag_cap, ctx->n_cu));
    hipLaunchKernelGGL(k_frag_count, grid, dim3(FI_THREADS), 0, st, (const fpl_fragment*)ctx->d_bm_frags.ptr, (const u32*)ctx->d_bm_counts.ptr,
                       (u32)frag_cap, n_reads, ctx->d_fi_cnt.ptr, ctx->d_fi.ptr);
    hipLaunchKernelGGL(k_frag_first, dim3(1), dim3(FI_SCAN), 0, st, (const u32*)ctx->d_fi_cnt.ptr, n_reads, (const u32*)ctx->d_bm_counts.ptr,
                       ctx->d_fi_first.ptr, ctx->d_fi.ptr);
    hipLaunchKernelGGL(k_frag_place, grid, dim3(FI_THREADS), 0, st, (const fpl_fragment*)ctx->d_bm_frags.ptr, (const u32*)ctx->d_fi_cnt.ptr,
                       (const u32*)ctx->d_fi_first.ptr, n_reads, ctx->d_fi_order.ptr, ctx->d_fi.ptr);
    FPL_HIP(hipGetLastError());
    return FPL_OK;
}

int fpl_set_fragment_output(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    if (!ctx->hcfg.defer) return FPL_OK; /* (without --break / --mask there is no fragment list: nothing changes) */
    if (ctx->submitted != ctx->waited) return FPL_ERR_STATE;
    /* the record form, tags and comments stay with the host in fragment mode: a context that has one of them on keeps it, and
       this switch stays off */
    if (on && (ctx->gzip_records || ctx->bam_tags || ctx->bam_comments.n != 0)) return FPL_ERR_STATE;
    ctx->frag_out = on != 0;
    return FPL_OK;
}

int fpl_set_emit_break_no(fpl_ctx* ctx, uint16_t* d_break_no) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->d_emit_break_no = d_break_no;
    return FPL_OK;
}

/* fpl_emit_batch_device with fpl_set_fragment_output: the output reads are the ordered fragments of the context's last batch */
static int emit_fragments(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint32_t n_reads,
                          const fpl_read_result* d_results, uint8_t* d_seq_out, uint8_t* d_qual_out, uint64_t out_cap_bytes,
                          uint64_t* d_off_out, uint32_t out_cap_reads, uint32_t* d_src, uint8_t* d_kind, fpl_emit_info* d_info,
                          hipStream_t stream);

/* the layout's block sums grow together; the list of sources on its own (it follows the capacity the caller gives) */
static int ensure_emit(fpl_ctx* ctx, u32 nblk, size_t n_from) {
    if (!ctx->d_emit_cnt.holds(nblk)) {
        const size_t cap = grown(nblk, 64);
        FPL_HIP(regrow(ctx->d_emit_cnt.want(cap), ctx->d_emit_max.want(cap), ctx->d_emit_bytes.want(cap)));
    }
    FPL_HIP(ctx->d_emit_from.grow(n_from, 1024));
    return FPL_OK;
}

int fpl_emit_batch_device(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint32_t n_reads,
                          const fpl_read_result* d_results, uint8_t* d_seq_out, uint8_t* d_qual_out, uint64_t out_cap_bytes,
                          uint64_t* d_off_out, uint32_t out_cap_reads, uint32_t* d_src, uint8_t* d_kind, fpl_emit_info* d_info,
                          void* stream_v) {
    if (!ctx || !d_info) return FPL_ERR_ARG;
    if (n_reads && (!d_seq || !d_qual || !d_off || !d_results || !d_seq_out || !d_qual_out || !d_off_out)) return FPL_ERR_ARG;
    if (n_reads > (1u << 30)) return FPL_ERR_ARG;
    if (ctx->hcfg.defer && !ctx->frag_out) {
        ctx->err = "fpl_emit_batch_device: with break_enabled / mask_enabled the output reads are the fragment list's (fpl_get_fragments, or fpl_set_fragment_output)";
        return FPL_ERR_STATE;
    }
    hipStream_t stream = (hipStream_t)stream_v;
    FPL_HIP(hipSetDevice(ctx->device));
    if (ctx->hcfg.defer && n_reads)
        return emit_fragments(ctx, d_seq, d_qual, d_off, n_reads, d_results, d_seq_out, d_qual_out, out_cap_bytes, d_off_out, out_cap_reads,
                              d_src, d_kind, d_info, stream);
    if (!n_reads) {
        FPL_HIP(hipMemsetAsync(d_info, 0, sizeof(fpl_emit_info), stream));
        if (d_off_out) FPL_HIP(hipMemsetAsync(d_off_out, 0, sizeof(uint64_t), stream));
        return FPL_OK;
    }
    const u32 nblk = cdiv(n_reads, (u32)EM_LAYOUT_READS);
    /* (the fill runs only when the output reads fit the caller's capacity, and a read gives two at the most) */
    const size_t n_from = (size_t)std::min<uint64_t>(2ull * n_reads, out_cap_reads);
    FPL_TRY(ensure_emit(ctx, nblk, n_from ? n_from : 1));
    hipLaunchKernelGGL(k_emit_count, dim3(nblk), dim3(EM_LAYOUT_READS), 0, stream, d_off, d_results, n_reads, ctx->d_emit_cnt.ptr,
                       ctx->d_emit_bytes.ptr, ctx->d_emit_max.ptr);
    hipLaunchKernelGGL(k_emit_scan, dim3(1), dim3(EM_SCAN_BLOCKS), 0, stream, ctx->d_emit_cnt.ptr, ctx->d_emit_bytes.ptr,
                       (const u32*)ctx->d_emit_max.ptr, nblk, (u64)out_cap_bytes, out_cap_reads, d_off_out, d_info);
    hipLaunchKernelGGL(k_emit_fill, dim3(nblk), dim3(EM_LAYOUT_READS), 0, stream, d_off, d_results, n_reads, (const u32*)ctx->d_emit_cnt.ptr,
                       (const u64*)ctx->d_emit_bytes.ptr, (const fpl_emit_info*)d_info, d_off_out, d_src, d_kind, ctx->d_emit_from.ptr);
    /* the output's size is known on the device only: a grid for the most the capacity admits, whose waves walk the tiles there are */
    hipLaunchKernelGGL(k_emit_gather, dim3(emit_gather_blocks(out_cap_bytes, ctx->n_cu)), dim3(EM_GATHER_THREADS), 0, stream,
                       (const u8*)d_seq, (const u8*)d_qual, (const uint64_t*)d_off_out, (const EmitFrom*)ctx->d_emit_from.ptr,
                       (const fpl_emit_info*)d_info, d_seq_out, d_qual_out);
    FPL_HIP(hipGetLastError());
    return FPL_OK;
}

static int emit_fragments(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint32_t n_reads,
                          const fpl_read_result* d_results, uint8_t* d_seq_out, uint8_t* d_qual_out, uint64_t out_cap_bytes,
                          uint64_t* d_off_out, uint32_t out_cap_reads, uint32_t* d_src, uint8_t* d_kind, fpl_emit_info* d_info,
                          hipStream_t stream) {
    FPL_TRY(frag_index(ctx, n_reads, stream));
    const size_t frag_cap = ctx->d_bm_frags.cap;
    const u32 nblk = cdiv((u32)frag_cap, (u32)EM_LAYOUT_READS); /* (a block per EM_LAYOUT_READS fragments the list has ROOM for) */
    const size_t n_from = (size_t)std::min<uint64_t>(frag_cap, out_cap_reads);
    FPL_TRY(ensure_emit(ctx, nblk, n_from ? n_from : 1));
    FPL_HIP(ctx->d_emit_ent.grow(n_from ? n_from : 1, 1024));
    const fpl_fragment* frags = ctx->d_bm_frags.ptr;
    const u32* order = ctx->d_fi_order.ptr;
    const FragIndex* fi = ctx->d_fi.ptr;
    hipLaunchKernelGGL(k_emit_count_frag, dim3(nblk), dim3(EM_LAYOUT_READS), 0, stream, d_off, d_results, n_reads, frags, order, fi,
                       ctx->d_emit_cnt.ptr, ctx->d_emit_bytes.ptr, ctx->d_emit_max.ptr);
    hipLaunchKernelGGL(k_emit_scan, dim3(1), dim3(EM_SCAN_BLOCKS), 0, stream, ctx->d_emit_cnt.ptr, ctx->d_emit_bytes.ptr,
                       (const u32*)ctx->d_emit_max.ptr, nblk, (u64)out_cap_bytes, out_cap_reads, d_off_out, d_info);
    hipLaunchKernelGGL(k_emit_fill_frag, dim3(nblk), dim3(EM_LAYOUT_READS), 0, stream, d_off, d_results, n_reads, frags, order, fi,
                       (const u32*)ctx->d_emit_cnt.ptr, (const u64*)ctx->d_emit_bytes.ptr, d_info, d_off_out, d_src, d_kind,
                       ctx->d_emit_break_no, ctx->d_emit_from.ptr, ctx->d_emit_ent.ptr);
    hipLaunchKernelGGL(k_emit_gather, dim3(emit_gather_blocks(out_cap_bytes, ctx->n_cu)), dim3(EM_GATHER_THREADS), 0, stream,
                       (const u8*)d_seq, (const u8*)d_qual, (const uint64_t*)d_off_out, (const EmitFrom*)ctx->d_emit_from.ptr,
                       (const fpl_emit_info*)d_info, d_seq_out, d_qual_out);
    if (ctx->hcfg.msk) /* (without --mask no fragment has a region) */
        hipLaunchKernelGGL(k_emit_mask, dim3(std::max<u32>(1u, std::min<u32>((u32)((n_from + 3) / 4), 8u * ctx->n_cu))), dim3(EM_GATHER_THREADS), 0,
                           stream, frags, (const fpl_region*)ctx->d_bm_regs.ptr, (const u32*)ctx->d_emit_ent.ptr, (const uint64_t*)d_off_out,
                           (const fpl_emit_info*)d_info, d_seq_out);
    FPL_HIP(hipGetLastError());
    return FPL_OK;
}
