/* rt_slots.h -- the asynchronous path's queue of FPL_MAX_IN_FLIGHT slots, written once for all five kinds: a submission takes the
   next slot (slot_begin) and counts once its work is enqueued (slot_commit); a staged kind -- text, BGZF, BGZF text -- enqueues stage 1 there
   and stage 2 (slot_continue) on its start call or in its wait; the waits collect in the order of submission (wait_front,
   wait_staged, wait_finish).  Around them what every kind shares: the slot's staging, the second half of a submission
   (submit_tail), the gzip member of a batch -- and the CSR kind itself. */
#pragma once

static int ensure_host_streams(fpl_ctx* ctx) {
    if (ctx->stream) return FPL_OK;
    FPL_HIP(ctx->stream.create());
    FPL_HIP(ctx->s_h2d.create());
    FPL_HIP(ctx->s_d2h.create());
    FPL_HIP(ctx->s_parse.create());
    return FPL_OK;
}

/* device staging of one slot for a batch of this size, and the page-locked copy of its records.
   host_results: false for a text slot -- its device arrays are sized by the most records its bytes COULD hold (one per 64 bytes),
   the page-locked host copy of the records by what the chunk turns out to have (text_continue): locking 19 MB of pages per slot
   for the 1 900 records of a 32 MB chunk of long reads was 3 ms of the link standing still, three times at the start of a run */
static int ensure_slot(fpl_ctx* ctx, fpl_ctx::Slot& sl, u32 n_reads, uint64_t n_bytes, bool host_results = true) {
    if (!sl.d_seq.holds(n_bytes)) {
        const size_t cap = grown(n_bytes, 64);
        FPL_HIP(regrow(sl.d_seq.want(cap), sl.d_qual.want(cap)));
    }
    if (!sl.d_results.holds(n_reads)) {
        const size_t cap = grown(n_reads, 16);
        FPL_HIP(regrow(sl.d_off.want(cap + 1), sl.d_results.want(cap)));
    }
    if (host_results) FPL_HIP(sl.h_results.grow(n_reads, 1024));
    return FPL_OK;
}

/* ---- gzip members of a text batch (ABI v9) and of a BAM batch (ABI v10): csrc/gz_emit.h ---- */
/* the fragment lists of the batch as the gzip kernels take them (fpl_set_fragment_output) */
static GzFragList gz_frag_list(const fpl_ctx* ctx) {
    return GzFragList{ctx->d_bm_frags.ptr, ctx->d_bm_regs.ptr, ctx->d_fi_order.ptr, ctx->d_fi.ptr};
}
/* the layout of a --break / --mask batch: the index over its fragment list, then a lane per ordered fragment.  rec_off and the
   block arrays are sized by the list's CAPACITY (break_mask_caps: the host knows it without a wait) */
static int gz_layout_frag(fpl_ctx* ctx, fpl_ctx::Slot& sl, u32 n) {
    fpl_ctx::Slot::Gzip& g = sl.gzip;
    const bool bam = bam_records(sl.kind);
    hipStream_t st = ctx->stream;
    FPL_TRY(frag_index(ctx, n, st));
    const size_t frag_cap = ctx->d_bm_frags.cap;
    const uint64_t bases = bam ? sl.bam.bases : sl.text.bytes / 2;
    const uint64_t blk_want = gz_frag_blocks_bound(bases, frag_cap) + 1;
    if (blk_want > 0xFFFFFFF0ull) return FPL_ERR_ARG;
    FPL_HIP(g.d_rec_off.grow(frag_cap + 1, 4096 / sizeof(u64)));
    if (!g.d_blk_start.holds(blk_want)) {
        const size_t cap = grown(blk_want, 64, 0xFFFFFFF0u);
        FPL_HIP(regrow(g.d_blk_start.want(cap), g.d_blk_off.want(cap), g.d_blk_size.want(cap), g.d_blk_crc.want(cap)));
    }
    const u32 blk_cap = (u32)g.d_blk_start.cap;
    if (bam)
        hipLaunchKernelGGL(k_gz_layout_frag_bam, dim3(1), dim3(1024), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, gz_frag_list(ctx), g.d_rec_off.ptr, g.d_blk_start.ptr, blk_cap - 1,
                           g.d_hdr.ptr);
    else
        hipLaunchKernelGGL(k_gz_layout_frag, dim3(1), dim3(1024), 0, st, (const u8*)sl.text.d_text.ptr, (const u32*)sl.text.d_line.ptr,
                           (const u32*)sl.text.d_nl.ptr, (const fpl_read_result*)sl.d_results.ptr, n, gz_frag_list(ctx), g.d_rec_off.ptr,
                           g.d_blk_start.ptr, blk_cap - 1, g.d_hdr.ptr);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipMemcpyAsync(g.h_hdr.ptr, g.d_hdr.ptr, sizeof(GzHeader), hipMemcpyDeviceToHost, st));
    FPL_HIP(hipEventRecord(g.ev, st));
    return FPL_OK;
}
/* behind the per-read kernels of the batch, on their stream: where every record's output and every deflate block starts */
static int gz_layout(fpl_ctx* ctx, fpl_ctx::Slot& sl, u32 n) {
    fpl_ctx::Slot::Gzip& g = sl.gzip;
    const bool bam = bam_records(sl.kind);
    if (!g.d_hdr.ptr) {
        FPL_HIP(g.d_hdr.alloc(1));
        FPL_HIP(g.h_hdr.alloc(1));
    }
    const bool tags = g.tags && g.records && bam; /* fpl_set_bam_tags: only where the bytes are BAM records of BAM records */
    const bool notes = g.notes.n != 0 && !g.records && bam; /* fpl_set_bam_comments: only where the bytes are the FASTQ text of BAM records */
    const uint64_t blk_want = (g.records ? (bam ? bamout_bam_blocks_bound(sl.bam.bases, n) + (tags ? bamtag_extra_bound(sl.bam.bytes) / GZ_B + 1 : 0)
                                                : bamout_blocks_bound(sl.text.bytes, n))
                                         : (bam ? gz_bam_blocks_bound(sl.bam.bases, n) + (notes ? bamcomment_extra_bound(sl.bam.bytes) / GZ_B + 1 : 0)
                                                : gz_blocks_bound(sl.text.bytes, n))) + 1;
    if (sl.frag) return gz_layout_frag(ctx, sl, n);
    if (blk_want > 0xFFFFFFF0ull) return FPL_ERR_ARG;
    FPL_HIP(g.d_rec_off.grow((size_t)n + 1, 4096 / sizeof(u64)));
    if (!g.d_blk_start.holds(blk_want)) {
        const size_t cap = grown(blk_want, 64, 0xFFFFFFF0u); /* (the kernels take it as 32 bits) */
        FPL_HIP(regrow(g.d_blk_start.want(cap), g.d_blk_off.want(cap), g.d_blk_size.want(cap), g.d_blk_crc.want(cap)));
    }
    const u32 blk_cap = (u32)g.d_blk_start.cap;
    hipStream_t st = ctx->stream;
    if (tags) { /* a lane per record walks its aux region, then the layout with the lengths it found */
        if (!ctx->d_tag_counters.ptr) {
            FPL_HIP(ctx->d_tag_counters.alloc(4));
            FPL_HIP(hipMemsetAsync(ctx->d_tag_counters.ptr, 0, 4 * sizeof(unsigned long long), st));
        }
        FPL_HIP(g.d_tag_info.grow(n, 4096 / sizeof(BamTagInfo)));
        if (g.mods || g.moves) { /* the same walk notes the MM / ML / MN fields, the mv and ts fields or both; a wave per candidate record plans its fragments' fields */
            const dim3 lanes(std::max<u32>(1u, std::min<u32>((n + 255) / 256, 8u * ctx->n_cu))), waves(std::max<u32>(1u, std::min<u32>((n + 3) / 4, 8u * ctx->n_cu)));
            const u32 fragment_mode = (u32)(ctx->hcfg.defer ? 1 : 0);
            if (g.mods) {
                if (!ctx->d_mod_counters.ptr) {
                    FPL_HIP(ctx->d_mod_counters.alloc(BAMMOD_COUNTERS));
                    FPL_HIP(hipMemsetAsync(ctx->d_mod_counters.ptr, 0, BAMMOD_COUNTERS * sizeof(unsigned long long), st));
                }
                FPL_HIP(g.d_mod_info.grow(n, 4096 / sizeof(BamModInfo)));
                FPL_HIP(g.d_mod_cand.grow(n, 1024));
                FPL_HIP(g.d_mod_plan.grow(n, 16));
                FPL_HIP(hipMemsetAsync(ctx->d_mod_counters.ptr + 4, 0, sizeof(unsigned long long), st));
            }
            if (g.moves) {
                if (!ctx->d_move_counters.ptr) {
                    FPL_HIP(ctx->d_move_counters.alloc(BAMMOVE_COUNTERS));
                    FPL_HIP(hipMemsetAsync(ctx->d_move_counters.ptr, 0, BAMMOVE_COUNTERS * sizeof(unsigned long long), st));
                }
                FPL_HIP(g.d_move_info.grow(n, 4096 / sizeof(BamMoveInfo)));
                FPL_HIP(g.d_move_cand.grow(n, 1024));
                FPL_HIP(g.d_move_plan.grow(n, 4096 / sizeof(BamMovePlan)));
                FPL_HIP(hipMemsetAsync(ctx->d_move_counters.ptr + 4, 0, sizeof(unsigned long long), st));
            }
            /* (without fpl_set_bam_mods the buffers of its walk are nullptr: k_bam_tags_moves leaves them alone) */
            BamModInfo* const minfo = g.mods ? g.d_mod_info.ptr : nullptr;
            u32* const mcand = g.mods ? g.d_mod_cand.ptr : nullptr;
            unsigned long long* const mcount = g.mods ? ctx->d_mod_counters.ptr : nullptr;
            if (g.moves)
                hipLaunchKernelGGL(k_bam_tags_moves, lanes, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                                   (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, ctx->d_tag_counters.ptr, minfo, mcand, mcount,
                                   g.d_move_info.ptr, g.d_move_cand.ptr, ctx->d_move_counters.ptr);
            else
                hipLaunchKernelGGL(k_bam_tags_mods, lanes, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                                   (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, ctx->d_tag_counters.ptr, minfo, mcand, mcount);
            if (g.mods)
                hipLaunchKernelGGL(k_bam_mods_plan, waves, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                                   (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, (const BamModInfo*)g.d_mod_info.ptr,
                                   (const u32*)g.d_mod_cand.ptr, g.d_mod_plan.ptr, ctx->d_tag_counters.ptr, ctx->d_mod_counters.ptr);
            if (g.moves) /* (behind the other plan: it adds to the lengths that one wrote) */
                hipLaunchKernelGGL(k_bam_moves_plan, waves, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                                   (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, (const BamMoveInfo*)g.d_move_info.ptr,
                                   (const u32*)g.d_move_cand.ptr, g.d_move_plan.ptr, ctx->d_tag_counters.ptr, ctx->d_move_counters.ptr);
        } else {
            hipLaunchKernelGGL(k_bam_tags, dim3(std::max<u32>(1u, std::min<u32>((n + 255) / 256, 8u * ctx->n_cu))), dim3(256), 0, st,
                               (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr, (const fpl_read_result*)sl.d_results.ptr, n,
                               (u32)(ctx->hcfg.defer ? 1 : 0), g.d_tag_info.ptr, ctx->d_tag_counters.ptr);
        }
        hipLaunchKernelGGL(k_bamout_layout_bam_tags, dim3(1), dim3(1024), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr, g.d_rec_off.ptr, g.d_blk_start.ptr,
                           blk_cap - 1, g.d_hdr.ptr);
    } else if (notes) {
        /* the walk and the plan of the tagged record form say which bytes either fragment's record would carry (their counts go
           into a block nobody reads); the tails write those bytes out, a wave per record measures their text, then the layout */
        if (!ctx->d_note_counters.ptr) {
            FPL_HIP(ctx->d_note_counters.alloc(4));
            FPL_HIP(hipMemsetAsync(ctx->d_note_counters.ptr, 0, 4 * sizeof(unsigned long long), st));
            FPL_HIP(ctx->d_note_work.alloc(4 + BAMMOD_COUNTERS));
        }
        FPL_HIP(hipMemsetAsync(ctx->d_note_work.ptr, 0, (4 + BAMMOD_COUNTERS) * sizeof(unsigned long long), st));
        FPL_HIP(g.d_tag_info.grow(n, 4096 / sizeof(BamTagInfo)));
        FPL_HIP(g.d_mod_info.grow(n, 4096 / sizeof(BamModInfo)));
        FPL_HIP(g.d_mod_cand.grow(n, 1024));
        FPL_HIP(g.d_mod_plan.grow(n, 16));
        FPL_HIP(g.d_note_len.grow(2 * (size_t)n, 4096 / sizeof(u64)));
        for (auto& t : g.d_note_tags) FPL_HIP(t.grow((size_t)sl.bam.bytes + BAM_PAD, 4096));
        const dim3 lanes(std::max<u32>(1u, std::min<u32>((n + 255) / 256, 8u * ctx->n_cu))), waves(std::max<u32>(1u, std::min<u32>((n + 3) / 4, 8u * ctx->n_cu)));
        const u32 fragment_mode = (u32)(ctx->hcfg.defer ? 1 : 0);
        hipLaunchKernelGGL(k_bam_tags_mods, lanes, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, ctx->d_note_work.ptr, g.d_mod_info.ptr,
                           g.d_mod_cand.ptr, ctx->d_note_work.ptr + 4);
        hipLaunchKernelGGL(k_bam_mods_plan, waves, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, fragment_mode, g.d_tag_info.ptr, (const BamModInfo*)g.d_mod_info.ptr,
                           (const u32*)g.d_mod_cand.ptr, g.d_mod_plan.ptr, ctx->d_note_work.ptr, ctx->d_note_work.ptr + 4);
        hipLaunchKernelGGL(k_bam_comment_tags, waves, dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (u64)sl.bam.bytes, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr, (const BamModInfo*)g.d_mod_info.ptr,
                           (const BamModPlan*)g.d_mod_plan.ptr, g.d_note_tags[0].ptr, g.d_note_tags[1].ptr);
        hipLaunchKernelGGL(k_bam_comment_len, waves, dim3(256), 0, st, (const u8*)g.d_note_tags[0].ptr, (const u8*)g.d_note_tags[1].ptr, (u64)sl.bam.bytes,
                           (const uint64_t*)sl.bam.d_rec.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr, g.notes, g.d_note_len.ptr, ctx->d_note_counters.ptr);
        hipLaunchKernelGGL(k_gz_layout_bam_comments, dim3(1), dim3(1024), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr, (const fpl_read_result*)sl.d_results.ptr, n,
                           (const u64*)g.d_note_len.ptr, g.d_rec_off.ptr, g.d_blk_start.ptr, blk_cap - 1, g.d_hdr.ptr);
    } else if (bam)
        hipLaunchKernelGGL(g.records ? k_bamout_layout_bam : k_gz_layout_bam, dim3(1), dim3(1024), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, g.d_rec_off.ptr, g.d_blk_start.ptr, blk_cap - 1, g.d_hdr.ptr);
    else
        hipLaunchKernelGGL(g.records ? k_bamout_layout : k_gz_layout, dim3(1), dim3(1024), 0, st, (const u8*)sl.text.d_text.ptr, (const u32*)sl.text.d_line.ptr,
                           (const u32*)sl.text.d_nl.ptr, (const fpl_read_result*)sl.d_results.ptr, n, g.d_rec_off.ptr, g.d_blk_start.ptr,
                           blk_cap - 1, g.d_hdr.ptr);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipMemcpyAsync(g.h_hdr.ptr, g.d_hdr.ptr, sizeof(GzHeader), hipMemcpyDeviceToHost, st));
    FPL_HIP(hipEventRecord(g.ev, st));
    return FPL_OK;
}
/* the layout is in: buffers of the sizes it found, the other kernels, the member's way back.  *gz / *gz_len: see the header */
static int gz_emit(fpl_ctx* ctx, fpl_ctx::Slot& sl, const uint8_t** gz, uint64_t* gz_len) {
    fpl_ctx::Slot::Gzip& g = sl.gzip;
    FPL_HIP(hipEventSynchronize(g.ev));
    const GzHeader h = *g.h_hdr.ptr;
    if (h.status & 4u) { /* (the fragment forms: frag_index.h found the lists overflowed, or not to index) */
        ctx->err = "break/mask lists overflowed their capacity";
        return FPL_ERR_CAPACITY;
    }
    if (h.status) {
        ctx->err = "gzip layout: more deflate blocks than the bound allows";
        return FPL_ERR_STATE;
    }
    if (h.total == 0) return FPL_OK;
    const u32 n = sl.n_reads;
    const uint64_t out_want = gz_out_bound(h.total, h.n_blocks, g.bgzf);
    FPL_HIP(g.d_comp.grow(h.total + 16, 4096));
    FPL_HIP(g.d_tmp.grow(out_want + 16, 4096));
    FPL_HIP(g.d_out.grow(out_want + 16, 4096));
    hipStream_t st = ctx->stream;
    /* (g.records: the bytes are BAM records, csrc/bam_emit.h; the block kernels below do not care) */
    if (sl.frag && bam_records(sl.kind))
        hipLaunchKernelGGL(k_gz_compose_frag_bam, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, gz_frag_list(ctx), (const u64*)g.d_rec_off.ptr, g.d_comp.ptr,
                           (u64)h.total);
    else if (sl.frag)
        hipLaunchKernelGGL(k_gz_compose_frag, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.text.d_text.ptr,
                           (const u32*)sl.text.d_line.ptr, (const u32*)sl.text.d_nl.ptr, (const fpl_read_result*)sl.d_results.ptr, n,
                           gz_frag_list(ctx), (const u64*)g.d_rec_off.ptr, g.d_comp.ptr, (u64)h.total);
    else if (g.tags && g.moves && g.records && bam_records(sl.kind))
        hipLaunchKernelGGL(k_bamout_compose_bam_moves, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr,
                           (const BamModInfo*)(g.mods ? g.d_mod_info.ptr : nullptr), (const BamModPlan*)(g.mods ? g.d_mod_plan.ptr : nullptr),
                           (const BamMoveInfo*)g.d_move_info.ptr, (const BamMovePlan*)g.d_move_plan.ptr, (const u64*)g.d_rec_off.ptr, g.d_comp.ptr,
                           (u64)h.total);
    else if (g.tags && g.mods && g.records && bam_records(sl.kind))
        hipLaunchKernelGGL(k_bamout_compose_bam_mods, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr, (const BamModInfo*)g.d_mod_info.ptr,
                           (const BamModPlan*)g.d_mod_plan.ptr, (const u64*)g.d_rec_off.ptr, g.d_comp.ptr, (u64)h.total);
    else if (g.tags && g.records && bam_records(sl.kind))
        hipLaunchKernelGGL(k_bamout_compose_bam_tags, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const BamTagInfo*)g.d_tag_info.ptr, (const u64*)g.d_rec_off.ptr,
                           g.d_comp.ptr, (u64)h.total);
    else if (g.notes.n != 0 && !g.records && bam_records(sl.kind))
        hipLaunchKernelGGL(k_gz_compose_bam_comments, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr, (const fpl_read_result*)sl.d_results.ptr, n,
                           (const BamTagInfo*)g.d_tag_info.ptr, (const u8*)g.d_note_tags[0].ptr, (const u8*)g.d_note_tags[1].ptr,
                           (const u64*)g.d_note_len.ptr, g.notes, (const u64*)g.d_rec_off.ptr, g.d_comp.ptr, (u64)h.total);
    else if (bam_records(sl.kind))
        hipLaunchKernelGGL(g.records ? k_bamout_compose_bam : k_gz_compose_bam, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const u64*)g.d_rec_off.ptr, g.d_comp.ptr, (u64)h.total);
    else
        hipLaunchKernelGGL(g.records ? k_bamout_compose : k_gz_compose, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.text.d_text.ptr, (const u32*)sl.text.d_line.ptr,
                           (const u32*)sl.text.d_nl.ptr, (const fpl_read_result*)sl.d_results.ptr, n, (const u64*)g.d_rec_off.ptr,
                           g.d_comp.ptr, (u64)h.total);
    const u32 grid = std::max<u32>(1u, std::min<u32>(h.n_blocks, 8u * ctx->n_cu));
    if (g.bgzf) {
        /* the BGZF form: the same blocks with a complete distance code, placed behind their stripes' headers, then the frames */
        const u32 n_stripes = (u32)gz_bgzf_blocks(h.total);
        hipLaunchKernelGGL(k_gz_block_bgzf, dim3(grid), dim3(GZ_THREADS), 0, st, (const u8*)g.d_comp.ptr, (const u64*)g.d_blk_start.ptr,
                           (const GzHeader*)g.d_hdr.ptr, g.d_tmp.ptr, g.d_blk_size.ptr, g.d_blk_crc.ptr);
        hipLaunchKernelGGL(k_gz_finish_bgzf, dim3(1), dim3(1024), 0, st, (const u64*)g.d_blk_start.ptr, (const u32*)g.d_blk_size.ptr,
                           (const u32*)g.d_blk_crc.ptr, (u64*)g.d_blk_off.ptr, g.d_hdr.ptr, (u64)out_want);
        hipLaunchKernelGGL(k_gz_frame, dim3((n_stripes + 255) / 256), dim3(256), 0, st, (const u64*)g.d_blk_start.ptr,
                           (const u32*)g.d_blk_size.ptr, (const u32*)g.d_blk_crc.ptr, (const u64*)g.d_blk_off.ptr, g.d_hdr.ptr,
                           g.d_out.ptr, (u64)out_want);
    } else {
        hipLaunchKernelGGL(k_gz_block, dim3(grid), dim3(GZ_THREADS), 0, st, (const u8*)g.d_comp.ptr, (const u64*)g.d_blk_start.ptr,
                           (const GzHeader*)g.d_hdr.ptr, g.d_tmp.ptr, g.d_blk_size.ptr, g.d_blk_crc.ptr);
        hipLaunchKernelGGL(k_gz_finish, dim3(1), dim3(1024), 0, st, (const u32*)g.d_blk_size.ptr, (const u32*)g.d_blk_crc.ptr,
                           (u64*)g.d_blk_off.ptr, g.d_hdr.ptr, g.d_out.ptr, (u64)out_want);
    }
    hipLaunchKernelGGL(k_gz_compact, dim3(grid), dim3(GZ_THREADS), 0, st, (const u8*)g.d_tmp.ptr, (const u64*)g.d_blk_start.ptr,
                       (const u32*)g.d_blk_size.ptr, (const u64*)g.d_blk_off.ptr, (const GzHeader*)g.d_hdr.ptr, g.d_out.ptr, (u64)out_want);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipMemcpyAsync(g.h_hdr.ptr, g.d_hdr.ptr, sizeof(GzHeader), hipMemcpyDeviceToHost, st));
    FPL_HIP(hipEventRecord(g.ev, st));
    FPL_HIP(g.h_out.grow(out_want, 4096)); /* (beside the kernels) */
    FPL_HIP(hipEventSynchronize(g.ev));
    const GzHeader h2 = *g.h_hdr.ptr;
    if (h2.status || h2.gz_len == 0 || h2.gz_len > out_want) {
        ctx->err = g.bgzf ? "BGZF blocks: the kernels report a size outside the bound" : "gzip member: the kernels report a size outside the bound";
        return FPL_ERR_STATE;
    }
    /* (the kernels are done: the member goes back on the copy stream, beside the next batch's kernels) */
    FPL_HIP(hipMemcpyAsync(g.h_out.ptr, g.d_out.ptr, h2.gz_len, hipMemcpyDeviceToHost, ctx->s_d2h));
    FPL_HIP(hipEventRecord(g.ev, ctx->s_d2h));
    FPL_HIP(hipEventSynchronize(g.ev));
    *gz = g.h_out.ptr;
    *gz_len = h2.gz_len;
    ctx->gz_batches++;
    return FPL_OK;
}

/* The second half of every submission, behind whatever brings the reads to the device as CSR arrays (`inputs` says when they
   are in): the per-read kernels on the compute stream, then the records' way back on a stream of their own, so that they do not
   queue behind the next batch's input copies.  A BAM batch sends its decoded bases back in front of the records, as soon as the
   decode is done; a text batch its line starts behind them; a gzip batch has its layout enqueued behind the kernels. */
static int submit_tail(fpl_ctx* ctx, fpl_ctx::Slot& sl, hipEvent_t inputs, u32 n, uint64_t n_bytes, u32 max_len) {
    FPL_HIP(hipStreamWaitEvent(ctx->stream, inputs, 0));
    ctx->next_inputs_event = inputs; /* (the end trims may start as soon as the inputs are in: beside the batch before) */
    const int rd = fpl_process_batch_device(ctx, sl.d_seq.ptr, sl.d_qual.ptr, sl.d_off.ptr, n, n_bytes, max_len, sl.d_results.ptr, ctx->stream);
    ctx->next_inputs_event = nullptr;
    if (rd != FPL_OK) return rd;
    FPL_HIP(hipEventRecord(sl.ev_kern, ctx->stream));
    if (bam_records(sl.kind)) {
        const fpl_ctx::Slot::Bam& b = sl.bam;
        FPL_HIP(hipStreamWaitEvent(ctx->s_d2h, sl.ev_parsed, 0));
        if (b.bases && b.seq_out) {
            FPL_HIP(hipMemcpyAsync(b.seq_out + b.o_begin, sl.d_seq.ptr + b.o_begin, b.bases, hipMemcpyDeviceToHost, ctx->s_d2h));
            FPL_HIP(hipMemcpyAsync(b.qual_out + b.o_begin, sl.d_qual.ptr + b.o_begin, b.bases, hipMemcpyDeviceToHost, ctx->s_d2h));
        }
    }
    FPL_HIP(hipStreamWaitEvent(ctx->s_d2h, sl.ev_kern, 0));
    FPL_HIP(hipMemcpyAsync(sl.h_results.ptr, sl.d_results.ptr, sizeof(fpl_read_result) * (size_t)n, hipMemcpyDeviceToHost, ctx->s_d2h));
    if (sl.kind == BatchKind::Text)
        FPL_HIP(hipMemcpyAsync(sl.text.h_line.ptr, sl.text.d_line.ptr, sizeof(u32) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->s_d2h));
    FPL_HIP(hipEventRecord(sl.ev_done, ctx->s_d2h));
    if (sl.gz) FPL_TRY(gz_layout(ctx, sl, n)); /* (on the compute stream) */
    sl.n_reads = n; /* (a staged slot's: what its wait hands over) */
    return FPL_OK;
}
/* after an enqueue error: "nothing is in flight" is what the caller reads into it, and it recycles the host arrays at once.  Copies
   or kernels that did get enqueued before the failing call may still read them (and the slot): wait them out first. */
static void drain(fpl_ctx* ctx) {
    for (hipStream_t st : {ctx->s_h2d.h, ctx->s_parse.h, ctx->stream.h, ctx->s_d2h.h})
        if (st) (void)hipStreamSynchronize(st);
}
/* the offsets of read i rise and it is no longer than 2^31 - 1; max_len follows the longest read */
static inline bool read_len_ok(const uint64_t* off, u32 i, u32& max_len) {
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x7FFFFFFFull) return false;
    max_len = std::max(max_len, (u32)(off[i + 1] - off[i]));
    return true;
}

/* ---- the slot protocol ---- */
/* A submission, behind its own argument checks: room in the queue, the device, --break / --mask (the fragment lists of the batch
   in flight live in buffers the next batch's kernels reuse, and they are read batch by batch: a CSR or BAM batch is let in while
   nothing is in flight, a text batch under the same rule once fpl_set_fragment_output is on, the resident kinds never); then the next slot, reset for `kind`.  Nothing counts before slot_commit. */
static int slot_begin(fpl_ctx* ctx, BatchKind kind, bool gz, fpl_ctx::Slot*& out) {
    if (ctx->submitted - ctx->waited >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    const bool staged = staged_kind(kind);
    /* (fpl_set_fragment_output lets a text batch in under the rule of the CSR and BAM kinds: the lists are sized in its stage 2,
       once the parse has said how many reads there are -- fpl_process_batch_device.  The resident kinds stay out.) */
    const bool refused = staged && !(ctx->frag_out && kind == BatchKind::Text);
    if (ctx->hcfg.defer && (refused || ctx->submitted != ctx->waited)) return FPL_ERR_STATE;
    /* (the slot's previous batch has been waited for -- FPL_MAX_IN_FLIGHT slots, FIFO -- so its buffers are free) */
    fpl_ctx::Slot& sl = ctx->slot[ctx->submitted % FPL_MAX_IN_FLIGHT];
    sl.kind = kind;
    sl.gz = gz;
    sl.frag = ctx->hcfg.defer && ctx->frag_out;
    sl.gzip.records = ctx->gzip_records;
    sl.gzip.tags = ctx->bam_tags;
    sl.gzip.mods = ctx->bam_tags && ctx->bam_mods;
    sl.gzip.moves = ctx->bam_tags && ctx->bam_moves;
    sl.gzip.notes = ctx->bam_comments;
    sl.gzip.bgzf = ctx->gzip_bgzf || sl.gzip.records; /* BAM records are BGZF whatever the framing says (here and not in gz_layout: a staged kind's layout runs in its start call or its wait) */
    sl.n_reads = 0;
    sl.user_results = nullptr;
    sl.rc = FPL_OK;
    sl.stage = 0;
    sl.cancelled = false;
    out = &sl;
    return FPL_OK;
}
/* the end of a submission.  enqueue_rc: what its enqueue gave (FPL_OK also where there was nothing to enqueue); stage: 1 when the
   slot waits for its stage 2 */
static int slot_commit(fpl_ctx* ctx, fpl_ctx::Slot& sl, int enqueue_rc, int stage = 0) {
    if (enqueue_rc != FPL_OK) {
        drain(ctx);
        return enqueue_rc;
    }
    sl.stage = stage;
    ctx->submitted++;
    return FPL_OK;
}

/* the oldest batch of `kind` in flight that is neither started nor cancelled: what its peek / start / cancel calls act on */
static fpl_ctx::Slot* pending(fpl_ctx* ctx, BatchKind kind) {
    for (u32 k = ctx->waited; k != ctx->submitted; k++) {
        fpl_ctx::Slot& sl = ctx->slot[k % FPL_MAX_IN_FLIGHT];
        if (sl.kind == kind && sl.stage == 1 && !sl.cancelled) return &sl;
    }
    return nullptr;
}
/* what those calls begin with: the pending slot (none: FPL_ERR_STATE, and the caller's record stays as it is), the record cleared,
   the slot's enqueue error if it has one (report_rc; a cancel goes on regardless), the device */
static int pending_begin(fpl_ctx* ctx, BatchKind kind, fpl_ctx::Slot*& sl, void* out = nullptr, size_t out_bytes = 0, bool report_rc = true) {
    sl = pending(ctx, kind);
    if (!sl) return FPL_ERR_STATE;
    if (out) memset(out, 0, out_bytes);
    if (report_rc && sl->rc != FPL_OK) return sl->rc;
    FPL_HIP(hipSetDevice(ctx->device));
    return FPL_OK;
}
/* fpl_peek_*: the pending slot with its header in */
static int peek_pending(fpl_ctx* ctx, BatchKind kind, fpl_ctx::Slot*& sl, void* out, size_t out_bytes) {
    FPL_TRY(pending_begin(ctx, kind, sl, out, out_bytes));
    FPL_HIP(hipEventSynchronize(sl->ev_parsed));
    return FPL_OK;
}

/* Stage 2 of a staged batch: the header is in -- enqueue what it sizes (rt_text.h, rt_bam.h, rt_bgzf_text.h; all leave n_reads at 0 where there is
   nothing to run: the wait reports).  A no-op for a slot whose stage 2 ran. */
/* (called by the start calls and the waits only: a submission never waits for a parse, so the next chunk's copy goes out behind this
   one's at once -- no round trip to the host between two chunks on the link -- and a batch that has only been peeked at is in no counter) */
static int text_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl);
static int bgzf_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out);
static int bgzf_text_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out);
static int slot_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out) {
    if (sl.stage != 1) return FPL_OK;
    sl.stage = 2;
    FPL_HIP(hipEventSynchronize(sl.ev_parsed));
    sl.n_reads = 0;
    if (sl.kind == BatchKind::Text) return text_continue(ctx, sl);
    return sl.kind == BatchKind::BGZF ? bgzf_continue(ctx, sl, seq_out, qual_out) : bgzf_text_continue(ctx, sl, seq_out, qual_out);
}
/* fpl_start_*: stage 2 of the pending slot, ahead of its wait; an error here is what that wait reports */
static int start_pending(fpl_ctx* ctx, BatchKind kind, uint8_t* seq_out, uint8_t* qual_out) {
    fpl_ctx::Slot* sl;
    FPL_TRY(pending_begin(ctx, kind, sl));
    const int r = slot_continue(ctx, *sl, seq_out, qual_out);
    if (r != FPL_OK) sl->rc = r;
    return r;
}

/* what every wait begins with: something is in flight and the oldest slot is of a kind this wait collects (`kinds`: kind_bit of
   each) -- else FPL_ERR_STATE, and nothing has been touched */
static constexpr unsigned kind_bit(BatchKind k) { return 1u << (unsigned)k; }
static int wait_front(fpl_ctx* ctx, unsigned kinds, fpl_ctx::Slot*& sl) {
    if (ctx->submitted == ctx->waited) return FPL_ERR_STATE;
    sl = &ctx->slot[ctx->waited % FPL_MAX_IN_FLIGHT];
    return (kinds & kind_bit(sl->kind)) ? FPL_OK : FPL_ERR_STATE;
}
/* a staged kind's wait, once its out-pointers are cleared: stage 2 unless a start call ran it (or a cancel took it out), and the
   slot leaves the queue.  Returns the slot's enqueue error: nothing was enqueued behind the failure */
static int wait_staged(fpl_ctx* ctx, fpl_ctx::Slot& sl) {
    FPL_HIP(hipSetDevice(ctx->device));
    if (!sl.cancelled && sl.rc == FPL_OK) {
        const int r = slot_continue(ctx, sl, nullptr, nullptr);
        if (r != FPL_OK) sl.rc = r;
    }
    ctx->waited++;
    return sl.cancelled ? FPL_OK : sl.rc;
}
/* what every wait ends with, for a slot that ran reads: the gzip member where the caller asks for one and the batch has one -- it
   is made before the records are handed over --, then the records' way back is done */
static int wait_finish(fpl_ctx* ctx, fpl_ctx::Slot& sl, const uint8_t** gz, uint64_t* gz_len) {
    if (gz && sl.gz) FPL_TRY(gz_emit(ctx, sl, gz, gz_len));
    FPL_HIP(hipEventSynchronize(sl.ev_done));
    return FPL_OK;
}

int fpl_in_flight(const fpl_ctx* ctx) { return ctx ? (int)(ctx->submitted - ctx->waited) : 0; }

/* ---- the CSR kind; its waits collect BAM batches too ---- */
/* gz != nullptr: fpl_wait_bam_gz */
static int wait_batch(fpl_ctx* ctx, const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx) return FPL_ERR_ARG;
    fpl_ctx::Slot* slp;
    FPL_TRY(wait_front(ctx, kind_bit(BatchKind::CSR) | kind_bit(BatchKind::BAM), slp)); /* (the others: fpl_wait_text, fpl_wait_bgzf_bam, fpl_wait_bgzf_text) */
    fpl_ctx::Slot& sl = *slp;
    ctx->waited++;
    if (sl.rc != FPL_OK) return sl.rc; /* nothing was enqueued behind the failure */
    if (sl.n_reads == 0) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_TRY(wait_finish(ctx, sl, gz, gz_len));
    memcpy(sl.user_results, sl.h_results.ptr, sizeof(fpl_read_result) * (size_t)sl.n_reads);
    return FPL_OK;
}
int fpl_wait(fpl_ctx* ctx) { return wait_batch(ctx, nullptr, nullptr); }
int fpl_wait_bam_gz(fpl_ctx* ctx, const uint8_t** gz, uint64_t* gz_len) {
    if (!gz || !gz_len) return FPL_ERR_ARG;
    *gz = nullptr;
    *gz_len = 0;
    return wait_batch(ctx, gz, gz_len);
}

int fpl_process_batch_async(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off,
                            uint32_t n_reads, fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    if (n_reads && (!seq || !qual || !off || !results)) return FPL_ERR_ARG;
    /* (a text batch in flight keeps waiting for ITS wait: the kernels of this batch go first -- the order of the kernels is free,
       the slots are collected in the order of submission) */
    fpl_ctx::Slot* slp;
    FPL_TRY(slot_begin(ctx, BatchKind::CSR, false, slp));
    fpl_ctx::Slot& sl = *slp;
    sl.n_reads = n_reads;
    sl.user_results = results;
    if (n_reads == 0) return slot_commit(ctx, sl, FPL_OK);
    const uint64_t n_bytes = off[n_reads];
    u32 max_len = 0;
    for (u32 i = 0; i < n_reads; i++)
        if (!read_len_ok(off, i, max_len)) return FPL_ERR_ARG;
    FPL_TRY(ensure_host_streams(ctx));
    FPL_TRY(ensure_slot(ctx, sl, n_reads, n_bytes));
    auto enqueue = [&]() -> int {
        if (n_bytes) {
            FPL_HIP(hipMemcpyAsync(sl.d_seq.ptr, seq, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
            FPL_HIP(hipMemcpyAsync(sl.d_qual.ptr, qual, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        }
        FPL_HIP(hipMemcpyAsync(sl.d_off.ptr, off, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        return submit_tail(ctx, sl, sl.ev_h2d, n_reads, n_bytes, max_len);
    };
    return slot_commit(ctx, sl, enqueue());
}

int fpl_process_batch(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint32_t n_reads,
                      fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    if (ctx->submitted != ctx->waited) return FPL_ERR_STATE; /* (collect the asynchronous batches first) */
    if (n_reads == 0) return FPL_OK;
    FPL_TRY(fpl_process_batch_async(ctx, seq, qual, off, n_reads, results));
    return fpl_wait(ctx);
}
