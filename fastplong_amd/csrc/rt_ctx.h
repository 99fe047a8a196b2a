/* rt_ctx.h -- the context behind the C-ABI: what a slot of the asynchronous path holds, and the error macros of the entry points.
   (One of the host units fpl_hip.hip includes, once each and in its order; none stands alone.) */
#pragma once

/* what a slot holds: a CSR batch (fpl_process_batch_async), a FASTQ text chunk (fpl_process_text_async) or BAM records
   (fpl_process_bam_async), a BAM's BGZF blocks whose records the device finds itself (fpl_process_bgzf_bam_async), or a FASTQ's
   BGZF blocks whose text the device cuts and parses itself (fpl_process_bgzf_text_async).  fpl_wait / fpl_wait_bam_gz collect CSR
   and BAM batches, fpl_wait_text* text batches, fpl_wait_bgzf_bam BGZF batches, fpl_wait_bgzf_text BGZF text batches. */
enum class BatchKind { CSR, Text, BAM, BGZF, BGZFText };
/* the kinds whose submission enqueues stage 1 only (rt_slots.h) */
static inline bool staged_kind(BatchKind k) { return k == BatchKind::Text || k == BatchKind::BGZF || k == BatchKind::BGZFText; }
/* the kinds that carry a tail in the context from one submission to the next */
static inline bool bgzf_kind(BatchKind k) { return k == BatchKind::BGZF || k == BatchKind::BGZFText; }
/* the slot holds BAM records on the device: d_bam, d_rec and the decoded arrays (what the BAM forms of the gzip kernels read) */
static inline bool bam_records(BatchKind k) { return k == BatchKind::BAM || k == BatchKind::BGZF; }

struct fpl_ctx {
    int device = -1;
    u32 n_cu = 256;
    int dbg = 0;
    bool probe_primed = false;
    int n_adapters = 2;
    u32 C = 0;
    DevBuf<DevConfig> d_cfg;
    DevBuf<DevAdapter> d_ads;
    DevBuf<long long> d_counters;
    /* per-batch workspace, grown on demand (ensure_workspace: all sized by the reads of the largest batch so far) */
    DevBuf<ReadState> d_state;
    DevBuf<ScanRec> d_recs;  /* k_scan -> k_resolve */
    DevBuf<ScanWin> d_wins;
    DevBuf<RedoItem> d_redo; /* k_resolve -> k_redo */
    DevBuf<uint64_t> d_frag_off;
    DevBuf<u32> d_frag_len;
    DevBuf<u32> d_work_ctr;
    /* --break / --mask (DevConfig::defer): lists k_break_mask appends to, sized per batch (ensure_break_mask; BmLists) */
    DevConfig hcfg;
    DevBuf<u32> d_frag_cyc;
    DevBuf<fpl_fragment> d_bm_frags;
    DevBuf<fpl_region> d_bm_regs;
    DevBuf<u32> d_bm_counts;
    DevBuf<u32> d_sort_ws;       /* k_stats_sorted: bucket counters and the slice table (words) */
    DevBuf<uint64_t> d_st_off;   /* the reads in sorted order (as many as d_state) */
    DevBuf<u32> d_st_len;
    DevBuf<u32> d_st_e;
    DevBuf<u64> d_stats_scratch; /* slabs of FS_SLAB words; beside them two flag bytes per slab + 64 */
    DevBuf<u8> d_stats_flags;
    DevBuf<u64> d_extra_scratch; /* the post-only pass's own slabs / flags (it runs on s_aux beside the reduce of k_stats_sorted) */
    DevBuf<u8> d_extra_flags;
    /* fpl_emit_batch_device (csrc/emit.h): the layout's per-block sums, and per output read where its bytes come from */
    DevBuf<u32> d_emit_cnt, d_emit_max;
    DevBuf<u64> d_emit_bytes;
    DevBuf<EmitFrom> d_emit_from;
    /* fpl_set_fragment_output: a context with --break / --mask writes its device output forms from the fragment list of its LAST
       batch -- one batch is in flight at a time, so the index over that list (csrc/frag_index.h) is the context's, not a slot's */
    bool frag_out = false;
    DevBuf<u32> d_fi_cnt, d_fi_first; /* per read: its fragments, and where they start in the order (n_reads + 1) */
    DevBuf<u32> d_fi_order;           /* per fragment of the list's capacity: the entry at that place */
    DevBuf<FragIndex> d_fi;
    DevBuf<u32> d_emit_ent;           /* fpl_emit_batch_device: the list entry of every output read (k_emit_mask) */
    uint16_t* d_emit_break_no = nullptr; /* fpl_set_emit_break_no: the caller's array, or none */
    /* The end trims of batch k + 1 beside the kernels of batch k ("trim ahead"): the trim kernel is the first of a batch, needs
       nothing of the batch before, and is bound by memory latency where k_scan / k_stats_sorted are bound by instruction issue
       -- 0.5 ms of a 12.5 ms step when two whole batches run side by side (round 4, tools/overlap_probe.py).  It writes
       ReadState[] and takes its groups off a work counter: both exist twice, batches alternate.  A batch qualifies when its
       inputs are known to be complete on the device before its predecessor is done: the asynchronous path (its own H2D
       event), or a caller's promise (fpl_assume_inputs_ready). */
    DevBuf<ReadState> d_state2;
    Stream s_trim;
    Event ev_trim_done, ev_batch_done[2], ev_stats_done[2];
    int ahead_gate = 0;             /* FPL_TRIM_AHEAD_GATE: 0 the trims of batch k + 1 start as soon as batch k - 1 is done -- beside k_scan of
                                       batch k, two of their blocks per CU (pipeline.h) --, 1 when the statistics kernel
                                       of batch k is done (beside its reduce / post-only tail: the default until round 6) */
    uint64_t batch_no = 0;          /* batches enqueued (parity picks the buffers) */
    bool trim_ahead = true;         /* FPL_NO_TRIM_AHEAD=1 (read in fpl_create) turns it off */
    bool inputs_ready = false;      /* fpl_assume_inputs_ready */
    hipEvent_t next_inputs_event = nullptr; /* (set by the asynchronous path around its call of fpl_process_batch_device) */
    Stream s_aux;                   /* the side stream of a batch (pipeline.h: FPL_FORK / FPL_JOIN) */
    Event ev_fork, ev_join;
    bool overlap = true;            /* FPL_NO_OVERLAP=1 (read in fpl_create): everything on the one stream */
    /* staging for the host-pointer entry points: FPL_MAX_IN_FLIGHT slots, so that the copies of one batch
       overlap the kernels of the previous one */
    struct Slot {
        BatchKind kind = BatchKind::CSR;
        bool gz = false; /* a text or BAM batch whose passing reads also come back as a gzip member (`gzip` below) */
        bool frag = false; /* ... written from the batch's fragment list (fpl_set_fragment_output on a --break / --mask context) */
        /* every kind: the reads as CSR arrays on the device (uploaded, parsed out of the text or decoded from the BAM records),
           their records there and in page-locked memory (the D2H copy never waits for a pageable destination; a text slot
           sizes h_results by the records its chunk really has) */
        DevBuf<u8> d_seq, d_qual;
        DevBuf<uint64_t> d_off;
        DevBuf<fpl_read_result> d_results;
        PinBuf<fpl_read_result> h_results;
        Event ev_h2d, ev_kern, ev_done;
        Event ev_parsed; /* text: the parse is done and the header is in; BAM: the bases are decoded */
        fpl_read_result* user_results = nullptr;
        u32 n_reads = 0;
        int rc = FPL_OK; /* error met while enqueueing, reported by the slot's wait */
        /* the staged kinds (text, BGZF; rt_slots.h): 1 stage 1 enqueued, the header on its way back; 2 stage 2 enqueued (or nothing
           to enqueue); 0 every other slot */
        int stage = 0;
        bool cancelled = false; /* fpl_cancel_text -- never run, reported by its wait */
        /* a TEXT batch: the chunk's bytes, its line breaks, the records' line starts and lengths; stage 1 (copy + parse + the
           header's way back) is enqueued at submission, stage 2 (the per-read kernels, the records' and line starts' way back) once
           the header is in -- by fpl_start_text or by the wait, whichever comes first */
        struct Text {
            uint64_t bytes = 0;
            DevBuf<u8> d_text;      /* the chunk and 16 bytes of padding */
            DevBuf<u32> d_nl, d_blk, d_line, d_len;
            DevBuf<TextHeader> d_hdr;
            PinBuf<TextHeader> h_hdr;
            PinBuf<u32> h_line;     /* four line starts per record */
            /* a BGZF TEXT batch (csrc/text_walk.h): d_text is [room for the tail | the inflated bytes], positions in d_nl / d_line
               are offsets into it -- what the text forms of the gzip kernels read, as for a text batch; the compressed bytes, the
               block table, the names and their offsets are Bam's below.  Stage 1 (upload, inflate, the walk, the header's way
               back) is enqueued at submission, stage 2 (the per-read kernels, the way back of records, names and -- where asked
               for -- bases and qualities) once the header is in, by fpl_start_bgzf_text or by the wait */
            DevBuf<u32> d_nlen;
            DevBuf<TextWalkScratch> d_ws;
            DevBuf<fpl_text_window> d_whdr;
            PinBuf<fpl_text_window> h_whdr;
        } text;
        /* a GZIP batch (fpl_set_text_gzip / fpl_set_bam_gzip; csrc/gz_emit.h).  The layout is enqueued behind the per-read kernels
           (submit_tail); everything behind it is sized by what the layout found and enqueued by the wait (gz_emit).  The BAM forms
           of the layout and compose kernels read d_bam / d_rec / d_seq / d_qual / d_off / d_results of THIS slot: nothing touches
           them before the slot's next submission, which comes after its wait */
        struct Gzip {
            DevBuf<u64> d_rec_off;
            DevBuf<u64> d_blk_start, d_blk_off;
            DevBuf<u32> d_blk_size, d_blk_crc;
            DevBuf<GzHeader> d_hdr;
            PinBuf<GzHeader> h_hdr;
            DevBuf<u8> d_comp; /* the composed text */
            DevBuf<u8> d_tmp;  /* every deflate block in a slot of its own */
            DevBuf<u8> d_out;  /* the member */
            PinBuf<u8> h_out;
            Event ev;
            bool bgzf = false; /* the context's framing when the batch was submitted (fpl_set_gzip_framing) */
            bool records = false; /* ... and its form: BAM records in place of FASTQ text (fpl_set_gzip_records; BGZF always) */
            bool tags = false;    /* ... which carry their input records' auxiliary fields (fpl_set_bam_tags; csrc/bam_tags.h) */
            DevBuf<BamTagInfo> d_tag_info; /* k_bam_tags -> the layout and compose kernels: one per input record */
            bool mods = false;    /* ... with MM / ML / MN re-indexed (fpl_set_bam_mods; csrc/bam_mods.h) */
            DevBuf<BamModInfo> d_mod_info; /* k_bam_tags_mods -> k_bam_mods_plan and the compose kernel: one per input record */
            DevBuf<u32> d_mod_cand;        /* the candidate records */
            DevBuf<BamModPlan> d_mod_plan; /* one per candidate (sized for every record: how many there are only the device knows) */
            bool moves = false;   /* ... with mv and ts re-indexed (fpl_set_bam_moves; csrc/bam_moves.h) */
            DevBuf<BamMoveInfo> d_move_info; /* k_bam_tags_moves -> k_bam_moves_plan and the compose kernel: one per input record */
            DevBuf<u32> d_move_cand;         /* the candidate records */
            DevBuf<BamMovePlan> d_move_plan; /* one per candidate, sized as d_mod_plan is */
            /* ... or FASTQ text whose name lines carry the input records' fields as comments (fpl_set_bam_comments;
               csrc/bam_comments.h): the selection when the batch was submitted (n 0: off) */
            bamcomment::Selection notes = {};
            DevBuf<u8> d_note_tags[2]; /* either fragment's tag bytes, at its record's place: each the size of the record buffer */
            DevBuf<u64> d_note_len;    /* k_bam_comment_len -> the layout and compose kernels: two per input record */
        } gzip;
        /* a BAM batch: the inflated record bytes, where every record starts, and where the decoded bases go on the host (NULL: a
           gzip batch that leaves them on the device) */
        struct Bam {
            uint64_t o_begin = 0, bases = 0;
            uint64_t bytes = 0; /* the extent of the record bytes in d_bam: no record, and no aux region, reaches past it */
            uint8_t *seq_out = nullptr, *qual_out = nullptr;
            DevBuf<u8> d_bam;
            DevBuf<uint64_t> d_rec;
            /* a BGZF batch (csrc/bam_walk.h): d_bam is [room for the tail | the inflated bytes], the walk fills d_rec and d_off.
               Stage 1 (upload, inflate, walk, the header's way back) is enqueued at submission, stage 2 (decode, the per-read
               kernels, the way back of records and names) once the header is in -- by fpl_start_bgzf_bam or by the wait */
            DevBuf<u8> d_comp;
            DevBuf<fpl_bgzf_block> d_blocks;
            DevBuf<u32> d_next;
            DevBuf<u64> d_cand;
            DevBuf<BamSeg> d_segs;
            DevBuf<u32> d_lists;
            DevBuf<BamSegBase> d_bases;
            DevBuf<fpl_bam_window> d_whdr;
            PinBuf<fpl_bam_window> h_whdr;
            DevBuf<u8> d_names;
            DevBuf<uint64_t> d_name_off;
            PinBuf<u8> h_names;
            PinBuf<uint64_t> h_name_off;
        } bam;
    };
    Slot slot[FPL_MAX_IN_FLIGHT];
    u32 submitted = 0, waited = 0; /* batches handed to / collected from the asynchronous path */
    Stream stream;       /* the compute stream of the host-pointer entry points */
    Stream s_h2d, s_d2h; /* copy streams */
    Stream s_parse;      /* the text-parse kernels of a chunk (behind its upload, beside the upload of the next) */
    StatsTune tune; /* FPL_STATS_* tuning hooks, read once in fpl_create */
    /* timing */
    int timing = 0;
    static constexpr int EV_RING = 128;
    Event ev[EV_RING][N_STAGES + 1]; /* (made by fpl_enable_timing) */
    int ev_calls = 0; /* batches recorded since fpl_enable_timing() */
    bool ev_ready = false; /* the whole event ring exists */
    uint64_t forms[6] = {0, 0, 0, 0, 0, 0}; /* fpl_get_batch_forms */
    bool text_gzip = false;    /* fpl_set_text_gzip */
    bool bam_gzip = false;     /* fpl_set_bam_gzip */
    bool gzip_bgzf = false;    /* fpl_set_gzip_framing: what the next gzip batch's slot records */
    bool gzip_records = false; /* fpl_set_gzip_records: the same */
    bool bam_tags = false;     /* fpl_set_bam_tags: the same */
    bool bam_mods = false;     /* fpl_set_bam_mods: the same */
    bamcomment::Selection bam_comments = {}; /* fpl_set_bam_comments: the same (n 0: off) */
    DevBuf<unsigned long long> d_note_counters; /* fpl_get_bam_comment_stats: four counts k_bam_comment_len adds to */
    DevBuf<unsigned long long> d_note_work;     /* what k_bam_tags_mods / k_bam_mods_plan count for such a batch: nobody reads it but they (zeroed per batch) */
    bool bam_moves = false;    /* fpl_set_bam_moves: the same */
    DevBuf<unsigned long long> d_move_counters; /* fpl_get_bam_move_stats: four counts, and the candidates of the batch in flight (csrc/bam_moves.h) */
    DevBuf<unsigned long long> d_mod_counters; /* fpl_get_bam_mod_stats: four counts, and the candidates of the batch in flight (csrc/bam_mods.h) */
    DevBuf<unsigned long long> d_tag_counters; /* fpl_get_bam_tag_stats: four counts k_bam_tags adds to (made with the first tagged batch) */
    /* fpl_process_bgzf_bam_async, fpl_process_bgzf_text_async: the tail between two submissions and the walk's state live on the
       device (csrc/bam_walk.h, csrc/text_walk.h) */
    DevBuf<BamWalkState> d_bamw_state;
    DevBuf<u8> d_bam_tail;
    uint64_t bam_tail_cap = FPL_BAM_TAIL_DEFAULT;
    bool bam_fresh = true;     /* the context holds no tail as far as the host knows (no submission since it last looked): skip is allowed */
    BatchKind tail_kind = BatchKind::BGZF; /* whose tail it is while not fresh: the BGZF kind that submitted last */
    u32 bam_seg_bytes = 0;     /* FPL_BAM_SEG_BYTES (read in fpl_create; 0: BAMW_DEFAULT_SEG) */
    uint64_t gz_batches = 0;   /* fpl_get_gzip_batches */
    std::string err;
};

#define FPL_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);                    \
            return FPL_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

/* a step of the host layer that gives an FPL_* code of its own: an error is the caller's */
#define FPL_TRY(call)                     \
    do {                                  \
        const int r__ = (call);           \
        if (r__ != FPL_OK) return r__;    \
    } while (0)

/* the same for the inflater's call (no context to keep the text in): what is in flight is waited for before the call returns */
#define FPL_HIP_RC(call)                                  \
    do {                                                  \
        if ((call) != hipSuccess) {                       \
            (void)hipStreamSynchronize(inf->stream);      \
            return FPL_ERR_HIP;                           \
        }                                                 \
    } while (0)
