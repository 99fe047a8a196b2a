/*
 * fpl_hip.hip -- the C-ABI of include/fastplong_amd.h on top of the gfx950 kernels.
 * Built by hipcc only (--offload-arch=gfx950); there is no CPU path in this library.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h> /* types only: the library is loaded with dlopen in fpl_allreduce_counters */
#include <dlfcn.h>
#include <sys/mman.h>

#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <thread>
#include <mutex>
#include <string>
#include <vector>

#include "pipeline.h"
#include "buf.h"
#include "text_parse.h"
#include "gz_emit.h"
#include "bam_decode.h"
#include "bgzf_inflate.h"
#include "bam_walk.h"
#include "gzip_inflate.h"
#include "emit.h"

using namespace fpl;

/* what a slot holds: a CSR batch (fpl_process_batch_async), a FASTQ text chunk (fpl_process_text_async) or BAM records
   (fpl_process_bam_async), or a BAM's BGZF blocks whose records the device finds itself (fpl_process_bgzf_bam_async).  fpl_wait /
   fpl_wait_bam_gz collect CSR and BAM batches, fpl_wait_text* text batches, fpl_wait_bgzf_bam BGZF batches. */
enum class BatchKind { CSR, Text, BAM, BGZF };
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
    /* The end trims of batch k + 1 beside the kernels of batch k ("trim ahead"): the trim kernel is the first of a batch, needs
       nothing of the batch before, and is bound by memory latency where k_scan / k_stats_sorted are bound by instruction issue
       -- 0.5 ms of a 12.5 ms step when two whole batches run side by side (round 4, tools/overlap_probe.py).  It writes
       ReadState[] and takes its groups off a work counter: both exist twice, batches alternate.  A batch qualifies when its
       inputs are known to be complete on the device before its predecessor is done: the asynchronous path (its own H2D
       event), or a caller's promise (fpl_assume_inputs_ready). */
    DevBuf<ReadState> d_state2;
    hipStream_t s_trim = nullptr;
    hipEvent_t ev_trim_done = nullptr, ev_batch_done[2] = {nullptr, nullptr}, ev_stats_done[2] = {nullptr, nullptr};
    int ahead_gate = 0;             /* FPL_TRIM_AHEAD_GATE: 0 the trims of batch k + 1 start as soon as batch k - 1 is done -- beside k_scan of
                                       batch k, two of their blocks per CU (pipeline.h) --, 1 when the statistics kernel
                                       of batch k is done (beside its reduce / post-only tail: the default until round 6) */
    uint64_t batch_no = 0;          /* batches enqueued (parity picks the buffers) */
    bool trim_ahead = true;         /* FPL_NO_TRIM_AHEAD=1 (read in fpl_create) turns it off */
    bool inputs_ready = false;      /* fpl_assume_inputs_ready */
    hipEvent_t next_inputs_event = nullptr; /* (set by the asynchronous path around its call of fpl_process_batch_device) */
    hipStream_t s_aux = nullptr;    /* owned: the side stream of a batch (pipeline.h: FPL_FORK / FPL_JOIN) */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap = true;            /* FPL_NO_OVERLAP=1 (read in fpl_create): everything on the one stream */
    /* staging for the host-pointer entry points: FPL_MAX_IN_FLIGHT slots, so that the copies of one batch
       overlap the kernels of the previous one */
    struct Slot {
        BatchKind kind = BatchKind::CSR;
        bool gz = false; /* a text or BAM batch whose passing reads also come back as a gzip member (`gzip` below) */
        /* every kind: the reads as CSR arrays on the device (uploaded, parsed out of the text or decoded from the BAM records),
           their records there and in page-locked memory (the D2H copy never waits for a pageable destination; a text slot
           sizes h_results by the records its chunk really has) */
        DevBuf<u8> d_seq, d_qual;
        DevBuf<uint64_t> d_off;
        DevBuf<fpl_read_result> d_results;
        PinBuf<fpl_read_result> h_results;
        hipEvent_t ev_h2d = nullptr, ev_kern = nullptr, ev_done = nullptr;
        hipEvent_t ev_parsed = nullptr; /* text: the parse is done and the header is in; BAM: the bases are decoded */
        fpl_read_result* user_results = nullptr;
        u32 n_reads = 0;
        int rc = FPL_OK; /* error met while enqueueing, reported by the slot's wait */
        /* a TEXT batch: the chunk's bytes, its line breaks, the records' line starts and lengths; stage 1 (copy + parse + the
           header's way back) is enqueued at submission, stage 2 (the per-read kernels, the records' and line starts' way back) once
           the header is in -- by fpl_start_text or by the wait, whichever comes first */
        struct Text {
            bool cancelled = false; /* fpl_cancel_text -- never run, reported by its wait */
            int stage = 0;          /* 1 parse enqueued, 2 batch enqueued (or nothing to enqueue) */
            uint64_t bytes = 0;
            DevBuf<u8> d_text;      /* the chunk and 16 bytes of padding */
            DevBuf<u32> d_nl, d_blk, d_line, d_len;
            DevBuf<TextHeader> d_hdr;
            PinBuf<TextHeader> h_hdr;
            PinBuf<u32> h_line;     /* four line starts per record */
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
            hipEvent_t ev = nullptr;
        } gzip;
        /* a BAM batch: the inflated record bytes, where every record starts, and where the decoded bases go on the host (NULL: a
           gzip batch that leaves them on the device) */
        struct Bam {
            uint64_t o_begin = 0, bases = 0;
            uint8_t *seq_out = nullptr, *qual_out = nullptr;
            DevBuf<u8> d_bam;
            DevBuf<uint64_t> d_rec;
            /* a BGZF batch (csrc/bam_walk.h): d_bam is [room for the tail | the inflated bytes], the walk fills d_rec and d_off.
               Stage 1 (upload, inflate, walk, the header's way back) is enqueued at submission, stage 2 (decode, the per-read
               kernels, the way back of records and names) once the header is in -- by fpl_start_bgzf_bam or by the wait */
            int stage = 0;
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
    hipStream_t stream = nullptr;  /* owned: the compute stream of the host-pointer entry points */
    hipStream_t s_h2d = nullptr, s_d2h = nullptr; /* owned: copy streams */
    hipStream_t s_parse = nullptr; /* owned: the text-parse kernels of a chunk (behind its upload, beside the upload of the next) */
    StatsTune tune; /* FPL_STATS_* tuning hooks, read once in fpl_create */
    /* timing */
    int timing = 0;
    static constexpr int EV_RING = 128;
    hipEvent_t ev[EV_RING][N_STAGES + 1] = {};
    int ev_calls = 0; /* batches recorded since fpl_enable_timing() */
    bool ev_ready = false; /* the whole event ring exists */
    uint64_t forms[6] = {0, 0, 0, 0, 0, 0}; /* fpl_get_batch_forms */
    bool text_gzip = false;    /* fpl_set_text_gzip */
    bool bam_gzip = false;     /* fpl_set_bam_gzip */
    /* fpl_process_bgzf_bam_async: the tail between two submissions and the walk's state live on the device (csrc/bam_walk.h) */
    DevBuf<BamWalkState> d_bamw_state;
    DevBuf<u8> d_bam_tail;
    uint64_t bam_tail_cap = FPL_BAM_TAIL_DEFAULT;
    bool bam_fresh = true;     /* the context holds no tail as far as the host knows (no submission since it last looked): skip is allowed */
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

/* the same for the inflater's call (no context to keep the text in): what is in flight is waited for before the call returns */
#define FPL_HIP_RC(call)                                  \
    do {                                                  \
        if ((call) != hipSuccess) {                       \
            (void)hipStreamSynchronize(inf->stream);      \
            return FPL_ERR_HIP;                           \
        }                                                 \
    } while (0)

extern "C" {

int fpl_abi_version(void) { return FPL_ABI_VERSION; }

const char* fpl_strerror(int code) {
    switch (code) {
        case FPL_OK: return "ok";
        case FPL_ERR_ARG: return "invalid argument";
        case FPL_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
        case FPL_ERR_HIP: return "HIP runtime error";
        case FPL_ERR_ADAPTER: return "adapter too long or too many adapters";
        case FPL_ERR_CAPACITY: return "read longer than the per-cycle capacity";
        case FPL_ERR_STATE: return "invalid state";
        default: return "unknown error";
    }
}

const char* fpl_last_error(const fpl_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

void fpl_options_default(fpl_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->cut_front_window = o->cut_tail_window = 4;
    o->cut_front_quality = o->cut_tail_quality = 20;
    o->polyx_min_len = 10;
    o->adapter_enabled = 1;
    o->ed_max = 0.25;
    o->trimming_extension = 10;
    o->qual_filter = 1;
    o->qualified_qual = '0';
    o->unqualified_percent_limit = 40;
    o->n_base_limit = 1000000;
    o->n_base_percent_limit = 10;
    o->length_filter = 1;
    o->required_length = 20;
    o->complexity_percent = 30;
    o->break_window = 100; /* src/main.cpp:72-73 */
    o->break_quality = 10;
    o->mask_window = 50;   /* src/main.cpp:67-68 */
    o->mask_quality = 10;
}

static int alloc_counters(fpl_ctx* ctx, u32 C, DevBuf<long long>& out) {
    size_t n = FPL_COUNTERS_LEN(C, ctx->n_adapters);
    FPL_HIP(out.alloc(n));
    FPL_HIP(hipMemset(out.ptr, 0, n * sizeof(long long)));
    return FPL_OK;
}

int fpl_create(fpl_ctx** out, const fpl_options* opt, const char* start_adapter, int32_t start_len,
               const char* end_adapter, int32_t end_len, const fpl_adapter* fasta, int32_t n_fasta,
               int32_t device, uint32_t max_cycles) {
    if (!out || !opt || start_len < 0 || end_len < 0 || n_fasta < 0 || (start_len && !start_adapter) ||
        (end_len && !end_adapter) || (n_fasta && !fasta))
        return FPL_ERR_ARG;
    *out = nullptr;
    if (start_len > FPL_MAX_ADAPTER_LEN || end_len > FPL_MAX_ADAPTER_LEN || 2 + n_fasta > FPL_MAX_ADAPTERS)
        return FPL_ERR_ADAPTER;
    for (int i = 0; i < n_fasta; i++)
        if (fasta[i].len < 0 || fasta[i].len > FPL_MAX_ADAPTER_LEN || (fasta[i].len && !fasta[i].seq)) return FPL_ERR_ADAPTER;
    int ndev = 0;
    /* (a context of the host-pointer path drives five streams -- kernels, two copy streams, two side streams; with the runtime's
       default of four hardware queues per device two of them share one and run in submission order.  The HOST asks for more --
       GPU_MAX_HW_QUEUES=8 in the environment before its first HIP call, as bin/fastplong_amd and bench.py do;
       the library does not touch the process's environment: setenv races with getenv on the host's other threads and does
       nothing once the runtime is up) */
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return FPL_ERR_NO_DEVICE;
    fpl_ctx* ctx = new (std::nothrow) fpl_ctx();
    if (!ctx) return FPL_ERR_ARG;
    ctx->device = device;
    ctx->n_adapters = 2 + n_fasta;
    int rc = [&]() -> int {
        FPL_HIP(hipSetDevice(device));
        hipDeviceProp_t prop;
        FPL_HIP(hipGetDeviceProperties(&prop, device));
        ctx->n_cu = prop.multiProcessorCount > 0 ? (u32)prop.multiProcessorCount : 256;
        /* (the side streams first, the three streams of the host-pointer path when that path is first used -- ensure_host_streams:
           the runtime deals its hardware queues out to the streams in turn, four by default, and two streams that share a queue
           run in submission order, i.e. not beside each other.  A process that only hands over device pointers has the caller's
           stream, s_aux and s_trim: three queues.) */
        FPL_HIP(hipStreamCreateWithFlags(&ctx->s_aux, hipStreamNonBlocking));
        FPL_HIP(hipStreamCreateWithFlags(&ctx->s_trim, hipStreamNonBlocking));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_trim_done, hipEventDisableTiming));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_batch_done[0], hipEventDisableTiming));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_batch_done[1], hipEventDisableTiming));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_stats_done[0], hipEventDisableTiming));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_stats_done[1], hipEventDisableTiming));
        if (const char* e = getenv("FPL_TRIM_AHEAD_GATE")) ctx->ahead_gate = atoi(e);
        if (const char* e = getenv("FPL_NO_TRIM_AHEAD")) ctx->trim_ahead = atoi(e) == 0;
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        FPL_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        if (const char* e = getenv("FPL_NO_OVERLAP")) ctx->overlap = atoi(e) == 0;
        if (const char* e = getenv("FPL_BAM_SEG_BYTES")) { /* (a test hook: small segments; a value the walk cannot use is ignored) */
            const long v = atol(e);
            ctx->bam_seg_bytes = v >= (long)BAMW_MIN_SEG && v <= (1l << 30) ? (u32)v : 0;
        }
        for (auto& sl : ctx->slot) {
            FPL_HIP(hipEventCreateWithFlags(&sl.ev_h2d, hipEventDisableTiming));
            FPL_HIP(hipEventCreateWithFlags(&sl.ev_kern, hipEventDisableTiming));
            FPL_HIP(hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming));
            FPL_HIP(hipEventCreateWithFlags(&sl.ev_parsed, hipEventDisableTiming));
            FPL_HIP(hipEventCreateWithFlags(&sl.gzip.ev, hipEventDisableTiming));
        }
        DevConfig cfg;
        build_config(&cfg, opt, start_len, end_len, n_fasta);
        std::vector<DevAdapter> ads(ctx->n_adapters);
        build_adapter(&ads[0], start_adapter, start_len);
        build_adapter(&ads[1], end_adapter, end_len);
        for (int i = 0; i < n_fasta; i++) build_adapter(&ads[2 + i], fasta[i].seq, fasta[i].len);
        cfg.ham_fast = ads[0].acgt_only && ads[1].acgt_only;
        {
            std::vector<int> lens(2 + n_fasta), acgt(2 + n_fasta);
            for (int i = 0; i < 2 + n_fasta; i++) lens[i] = ads[i].len, acgt[i] = ads[i].acgt_only;
            cfg.trim_mode = trim_mode_of(lens.data(), acgt.data(), 2 + n_fasta);
        }
        cfg.scan_short = cfg.adapter_enabled && cfg.ham_fast && ads[0].len <= 32 && ads[1].len <= 32;
        if (const char* e = getenv("FPL_DEBUG_FLAGS")) cfg.dbg = atoi(e); /* the environment is read here and nowhere else */
        ctx->tune = stats_tune_from_env();
        ctx->dbg = cfg.dbg;
        if ((cfg.brk && cfg.brk_w <= 0) || (cfg.msk && cfg.msk_w <= 0)) {
            ctx->err = "break / mask window size must be positive";
            return FPL_ERR_ARG; /* (the caller below destroys the context) */
        }
        ctx->hcfg = cfg;
        FPL_HIP(ctx->d_cfg.alloc(1));
        FPL_HIP(hipMemcpy(ctx->d_cfg.ptr, &cfg, sizeof(cfg), hipMemcpyHostToDevice));
        FPL_HIP(ctx->d_ads.alloc(ads.size()));
        FPL_HIP(hipMemcpy(ctx->d_ads.ptr, ads.data(), sizeof(DevAdapter) * ads.size(), hipMemcpyHostToDevice));
        FPL_HIP(ctx->d_work_ctr.alloc(2 * WORK_CTR_WORDS)); /* (two sets: batches alternate) */
        ctx->C = max_cycles ? max_cycles : 1;
        int r = alloc_counters(ctx, ctx->C, ctx->d_counters);
        if (r != FPL_OK) return r;
        /* (the ring of timing events -- a thousand of them -- is made when timing is first asked for: a command-line run never does) */
        return FPL_OK;
    }();
    if (rc != FPL_OK) {
        fprintf(stderr, "fpl_create: %s (%s)\n", fpl_strerror(rc), ctx->err.c_str());
        fpl_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return FPL_OK;
}

void fpl_destroy(fpl_ctx* ctx) {
    if (!ctx) return;
    if (ctx->device >= 0) (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    /* (the buffers of the context and of its slots go with the `delete` below) */
    for (auto& sl : ctx->slot) {
        if (sl.gzip.ev) (void)hipEventDestroy(sl.gzip.ev);
        if (sl.ev_parsed) (void)hipEventDestroy(sl.ev_parsed);
        if (sl.ev_h2d) (void)hipEventDestroy(sl.ev_h2d);
        if (sl.ev_kern) (void)hipEventDestroy(sl.ev_kern);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    if (ctx->s_h2d) (void)hipStreamDestroy(ctx->s_h2d);
    if (ctx->s_d2h) (void)hipStreamDestroy(ctx->s_d2h);
    if (ctx->s_parse) (void)hipStreamDestroy(ctx->s_parse);
    if (ctx->s_aux) (void)hipStreamDestroy(ctx->s_aux);
    if (ctx->s_trim) (void)hipStreamDestroy(ctx->s_trim);
    if (ctx->ev_trim_done) (void)hipEventDestroy(ctx->ev_trim_done);
    for (hipEvent_t e : ctx->ev_batch_done)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_stats_done)
        if (e) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    for (int r = 0; r < fpl_ctx::EV_RING; r++)
        for (int i = 0; i <= N_STAGES; i++)
            if (ctx->ev[r][i]) (void)hipEventDestroy(ctx->ev[r][i]);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

uint32_t fpl_max_cycles(const fpl_ctx* ctx) { return ctx ? ctx->C : 0; }
int32_t fpl_n_adapters(const fpl_ctx* ctx) { return ctx ? ctx->n_adapters : 0; }
size_t fpl_counters_len(const fpl_ctx* ctx) { return ctx ? FPL_COUNTERS_LEN(ctx->C, ctx->n_adapters) : 0; }
void* fpl_counters_device_ptr(fpl_ctx* ctx) { return ctx ? ctx->d_counters.ptr : nullptr; }

int fpl_synchronize(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    return FPL_OK;
}

/* cycle-major layout: growing C moves the two Stats tails and appends zero cycles */
int fpl_reserve_cycles(fpl_ctx* ctx, uint32_t max_cycles) {
    if (!ctx) return FPL_ERR_ARG;
    if (max_cycles <= ctx->C) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    DevBuf<long long> nw;
    const u32 Co = ctx->C, Cn = max_cycles;
    int r = alloc_counters(ctx, Cn, nw);
    if (r != FPL_OK) return r;
    for (int k = 0; k < 2; k++) {
        const long long* so = ctx->d_counters.ptr + (size_t)k * FPL_STATS_LEN(Co);
        long long* sn = nw.ptr + (size_t)k * FPL_STATS_LEN(Cn);
        FPL_HIP(hipMemcpy(sn, so, (size_t)Co * FPL_CYC_STRIDE * sizeof(long long), hipMemcpyDeviceToDevice));
        FPL_HIP(hipMemcpy(sn + (size_t)Cn * FPL_CYC_STRIDE, so + (size_t)Co * FPL_CYC_STRIDE,
                          FPL_STATS_TAIL * sizeof(long long), hipMemcpyDeviceToDevice));
    }
    FPL_HIP(hipMemcpy(nw.ptr + FPL_OFF_FR(Cn), ctx->d_counters.ptr + FPL_OFF_FR(Co),
                      (FPL_FR_LEN + FPL_KEYHIST_LEN(ctx->n_adapters)) * sizeof(long long), hipMemcpyDeviceToDevice));
    ctx->d_counters.swap(nw); /* (the old block goes with nw) */
    ctx->C = Cn;
    return FPL_OK;
}

int fpl_get_counters(fpl_ctx* ctx, int64_t* host_buf, size_t n) {
    if (!ctx || !host_buf || n != fpl_counters_len(ctx)) return FPL_ERR_ARG;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    FPL_HIP(hipMemcpy(host_buf, ctx->d_counters.ptr, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FPL_OK;
}

/* RCCL, loaded on first use: a host that never merges across devices does not need the library at all */
namespace {
struct Rccl {
    void* lib = nullptr;
    std::string path; /* what dlopen took */
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string& err) {
        if (lib) return true;
        /* a librccl the process has mapped already (PyTorch-ROCm carries its own under torch/lib, beside its HIP runtime) is THE
           one to use: a second copy would bring a second set of communicator state.  Else the loader's search path, ROCm's
           directory, and the directory of the HIP runtime this library itself resolved to. */
        std::vector<std::string> names;
        if (FILE* maps = fopen("/proc/self/maps", "r")) {
            char line[4096];
            while (fgets(line, sizeof line, maps)) {
                const char* path = strchr(line, '/');
                if (!path || !strstr(path, "librccl.so")) continue;
                std::string s(path);
                while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
                names.push_back(s);
                break;
            }
            fclose(maps);
        }
        names.insert(names.end(), {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"});
        Dl_info hip_at;
        if (dladdr((void*)&hipGetDeviceCount, &hip_at) && hip_at.dli_fname) {
            std::string dir(hip_at.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                names.push_back(dir.substr(0, slash) + "/librccl.so.1");
                names.push_back(dir.substr(0, slash) + "/librccl.so");
            }
        }
        for (const std::string& name : names) {
            lib = dlopen(name.c_str(), RTLD_NOW | RTLD_GLOBAL);
            if (lib) {
                path = name;
                break;
            }
        }
        if (!lib) {
            err = std::string("dlopen(librccl): ") + dlerror();
            return false;
        }
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        AllReduce = (decltype(AllReduce))dlsym(lib, "ncclAllReduce");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !AllReduce) {
            err = "librccl lacks an expected symbol";
            lib = nullptr;
            return false;
        }
        return true;
    }
};
Rccl g_rccl;
}  // namespace

/* communicators made ahead of the merge (fpl_comm_init), kept for the devices they were made for */
namespace {
struct CommCache {
    std::mutex m;
    std::vector<int> devs;
    std::vector<ncclComm_t> comms;
    bool matches(fpl_ctx** ctxs, int n) const {
        if ((int)devs.size() != n || n == 0) return false;
        for (int i = 0; i < n; i++)
            if (devs[(size_t)i] != ctxs[i]->device) return false;
        return true;
    }
    void drop() { /* (caller holds m) */
        for (ncclComm_t c : comms)
            if (c && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c);
        comms.clear();
        devs.clear();
    }
};
CommCache g_comms;
bool rccl_forced() {
    const char* force = getenv("FPL_RCCL_FORCE");
    return force && atoi(force) > 0;
}
int check_merge_args(fpl_ctx** ctxs, int32_t n) {
    if (!ctxs || n < 1) return FPL_ERR_ARG;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i] || ctxs[i]->n_adapters != ctxs[0]->n_adapters) return FPL_ERR_ARG;
        for (int j = 0; j < i; j++)
            if (ctxs[j]->device == ctxs[i]->device) return FPL_ERR_ARG; /* one context per device */
    }
    return FPL_OK;
}
}  // namespace

int fpl_comm_init(fpl_ctx** ctxs, int32_t n) {
    if (!ctxs && n == 0) { /* give the kept communicators back */
        std::lock_guard<std::mutex> g(g_comms.m);
        g_comms.drop();
        return FPL_OK;
    }
    const int rc0 = check_merge_args(ctxs, n);
    if (rc0 != FPL_OK) return rc0;
    if (n == 1 && !rccl_forced()) return FPL_OK; /* (one context: the merge needs no communicator) */
    std::lock_guard<std::mutex> g(g_comms.m);
    if (g_comms.matches(ctxs, n)) return FPL_OK;
    std::string err;
    if (!g_rccl.load(err)) return FPL_ERR_STATE; /* (fpl_allreduce_counters will say why) */
    g_comms.drop();
    std::vector<int> devs((size_t)n);
    for (int i = 0; i < n; i++) devs[(size_t)i] = ctxs[i]->device;
    std::vector<ncclComm_t> comms((size_t)n, nullptr);
    if (g_rccl.CommInitAll(comms.data(), n, devs.data()) != ncclSuccess) return FPL_ERR_HIP;
    g_comms.devs = devs;
    g_comms.comms = comms;
    return FPL_OK;
}

int fpl_allreduce_counters(fpl_ctx** ctxs, int32_t n) {
    const int rc0 = check_merge_args(ctxs, n);
    if (rc0 != FPL_OK) return rc0;
    fpl_ctx* ctx = ctxs[0]; /* (FPL_HIP reports through this one) */
    u32 C = 0;
    for (int i = 0; i < n; i++) {
        if (ctxs[i]->submitted != ctxs[i]->waited) return FPL_ERR_STATE;
        C = std::max(C, ctxs[i]->C);
    }
    for (int i = 0; i < n; i++) {
        const int r = fpl_reserve_cycles(ctxs[i], C);
        if (r != FPL_OK) return r;
        FPL_HIP(hipSetDevice(ctxs[i]->device));
        FPL_HIP(hipDeviceSynchronize());
    }
    /* one context: nothing to merge.  FPL_RCCL_FORCE=1 (a test hook) runs the collective all the same -- a one-rank communicator,
       the in-place sum on the context's stream -- so that the loader, the communicator set-up and the call are exercised on a
       box with a single GPU; the buffer must come out unchanged. */
    if (n == 1 && !rccl_forced()) return FPL_OK;
    /* (the loader, the communicator cache and the library's path are all behind g_comms.m: a host may merge while a thread of
       its own is still inside fpl_comm_init) */
    std::lock_guard<std::mutex> keep(g_comms.m);
    if (!g_rccl.load(ctx->err)) return FPL_ERR_STATE;
#define FPL_NCCL(call)                                                                                   \
    do {                                                                                                 \
        const ncclResult_t r__ = (call);                                                                 \
        if (r__ != ncclSuccess) {                                                                        \
            ctx->err = std::string(#call) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r__) : "rccl error"); \
            rc = FPL_ERR_HIP;                                                                            \
        }                                                                                                \
    } while (0)
    int rc = FPL_OK;
    /* the communicators fpl_comm_init made for exactly these devices, else a set of this call's own */
    const bool kept = g_comms.matches(ctxs, n);
    std::vector<ncclComm_t> own;
    if (!kept) {
        own.assign((size_t)n, nullptr);
        std::vector<int> devs((size_t)n);
        for (int i = 0; i < n; i++) devs[(size_t)i] = ctxs[i]->device;
        FPL_NCCL(g_rccl.CommInitAll(own.data(), n, devs.data()));
        if (rc != FPL_OK) return rc;
    }
    const std::vector<ncclComm_t>& comms = kept ? g_comms.comms : own;
    const size_t len = FPL_COUNTERS_LEN(C, ctx->n_adapters);
    FPL_NCCL(g_rccl.GroupStart());
    for (int i = 0; i < n && rc == FPL_OK; i++) {
        if (hipSetDevice(ctxs[i]->device) != hipSuccess) {
            ctx->err = "hipSetDevice failed inside the all-reduce group";
            rc = FPL_ERR_HIP;
            break;
        }
        FPL_NCCL(g_rccl.AllReduce(ctxs[i]->d_counters.ptr, ctxs[i]->d_counters.ptr, len, ncclInt64, ncclSum, comms[(size_t)i], ctxs[i]->s_aux));
    }
    FPL_NCCL(g_rccl.GroupEnd());
    for (int i = 0; i < n; i++) {
        if (hipSetDevice(ctxs[i]->device) != hipSuccess || hipStreamSynchronize(ctxs[i]->s_aux) != hipSuccess) {
            if (rc == FPL_OK) ctx->err = "synchronizing the all-reduce failed";
            rc = FPL_ERR_HIP;
        }
    }
    for (ncclComm_t c : own)
        if (c) FPL_NCCL(g_rccl.CommDestroy(c));
#undef FPL_NCCL
    return rc;
}

const char* fpl_rccl_library(void) {
    /* a copy taken under the lock (the loader may be running on another thread); it stays valid until the next call on this thread */
    static thread_local std::string copy;
    std::lock_guard<std::mutex> g(g_comms.m);
    copy = g_rccl.path;
    return copy.c_str();
}

int fpl_assume_inputs_ready(fpl_ctx* ctx, int yes) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->inputs_ready = yes != 0;
    return FPL_OK;
}

int fpl_get_batch_forms(const fpl_ctx* ctx, uint64_t out[6]) {
    if (!ctx || !out) return FPL_ERR_ARG;
    for (int i = 0; i < 6; i++) out[i] = ctx->forms[i];
    return FPL_OK;
}

int fpl_get_gzip_batches(const fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    *out = ctx->gz_batches;
    return FPL_OK;
}

int fpl_reset_counters(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    for (int i = 0; i < 6; i++) ctx->forms[i] = 0;
    ctx->gz_batches = 0;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    FPL_HIP(hipMemset(ctx->d_counters.ptr, 0, fpl_counters_len(ctx) * sizeof(long long)));
    return FPL_OK;
}

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
        int r = fpl_reserve_cycles(ctx, want > 0x7FFFFFFFull ? max_read_len : (u32)want);
        if (r != FPL_OK) return r;
    }
    /* which statistics pass the batch takes: asked ONCE -- the side stream's slabs, the launch sequence and the form counters all
       follow this one answer (a drift between separate askings would size the slabs for one form and launch the other) */
    const bool sorted_form = n_reads && stats_takes_sorted(n_reads, n_bytes, max_read_len, ctx->n_cu, ctx->tune, ctx->hcfg.defer != 0);
    if (n_reads) {
        int r = ensure_workspace(ctx, n_reads);
        if (r != FPL_OK) return r;
        r = ensure_scratch(ctx, n_reads, n_bytes, max_read_len);
        if (r != FPL_OK) return r;
        r = ensure_extra_scratch(ctx, n_reads, max_read_len, sorted_form);
        if (r != FPL_OK) return r;
        r = ensure_sort_ws(ctx, n_reads, n_bytes);
        if (r != FPL_OK) return r;
        r = ensure_break_mask(ctx, n_reads, n_bytes);
        if (r != FPL_OK) return r;
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
    if (ctx->trim_ahead && ctx->overlap) a.ev_stats_done = (void*)ctx->ev_stats_done[par];
    if (ahead) {
        a.trim_stream = ctx->s_trim;
        a.ev_trim_done = (void*)ctx->ev_trim_done;
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
        a.ev_fork = (void*)ctx->ev_fork;
        a.ev_join = (void*)ctx->ev_join;
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
    if (ctx->hcfg.defer) {
        ctx->err = "fpl_emit_batch_device: with break_enabled / mask_enabled the output reads are the fragment list's (fpl_get_fragments)";
        return FPL_ERR_STATE;
    }
    hipStream_t stream = (hipStream_t)stream_v;
    FPL_HIP(hipSetDevice(ctx->device));
    if (!n_reads) {
        FPL_HIP(hipMemsetAsync(d_info, 0, sizeof(fpl_emit_info), stream));
        if (d_off_out) FPL_HIP(hipMemsetAsync(d_off_out, 0, sizeof(uint64_t), stream));
        return FPL_OK;
    }
    const u32 nblk = cdiv(n_reads, (u32)EM_LAYOUT_READS);
    /* (the fill runs only when the output reads fit the caller's capacity, and a read gives two at the most) */
    const size_t n_from = (size_t)std::min<uint64_t>(2ull * n_reads, out_cap_reads);
    const int r = ensure_emit(ctx, nblk, n_from ? n_from : 1);
    if (r != FPL_OK) return r;
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

static int ensure_host_streams(fpl_ctx* ctx) {
    if (ctx->stream) return FPL_OK;
    FPL_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    FPL_HIP(hipStreamCreateWithFlags(&ctx->s_h2d, hipStreamNonBlocking));
    FPL_HIP(hipStreamCreateWithFlags(&ctx->s_d2h, hipStreamNonBlocking));
    FPL_HIP(hipStreamCreateWithFlags(&ctx->s_parse, hipStreamNonBlocking));
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

/* ---- FASTQ text in (ABI v7): csrc/text_parse.h ---- */
static int ensure_text_slot(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint64_t n_bytes) {
    fpl_ctx::Slot::Text& t = sl.text;
    int r = ensure_slot(ctx, sl, (u32)(n_bytes / 64 + 16), n_bytes / 2 + 64, false);
    if (r != FPL_OK) return r;
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

/* ---- gzip members of a text batch (ABI v9) and of a BAM batch (ABI v10): csrc/gz_emit.h ---- */
/* behind the per-read kernels of the batch, on their stream: where every record's output and every deflate block starts */
static int gz_layout(fpl_ctx* ctx, fpl_ctx::Slot& sl, u32 n) {
    fpl_ctx::Slot::Gzip& g = sl.gzip;
    const bool bam = bam_records(sl.kind);
    if (!g.d_hdr.ptr) {
        FPL_HIP(g.d_hdr.alloc(1));
        FPL_HIP(g.h_hdr.alloc(1));
    }
    const uint64_t blk_want = (bam ? gz_bam_blocks_bound(sl.bam.bases, n) : gz_blocks_bound(sl.text.bytes, n)) + 1;
    if (blk_want > 0xFFFFFFF0ull) return FPL_ERR_ARG;
    FPL_HIP(g.d_rec_off.grow((size_t)n + 1, 4096 / sizeof(u64)));
    if (!g.d_blk_start.holds(blk_want)) {
        const size_t cap = grown(blk_want, 64, 0xFFFFFFF0u); /* (the kernels take it as 32 bits) */
        FPL_HIP(regrow(g.d_blk_start.want(cap), g.d_blk_off.want(cap), g.d_blk_size.want(cap), g.d_blk_crc.want(cap)));
    }
    const u32 blk_cap = (u32)g.d_blk_start.cap;
    hipStream_t st = ctx->stream;
    if (bam)
        hipLaunchKernelGGL(k_gz_layout_bam, dim3(1), dim3(1024), 0, st, (const u8*)sl.bam.d_bam.ptr, (const uint64_t*)sl.bam.d_rec.ptr,
                           (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, g.d_rec_off.ptr, g.d_blk_start.ptr, blk_cap - 1, g.d_hdr.ptr);
    else
        hipLaunchKernelGGL(k_gz_layout, dim3(1), dim3(1024), 0, st, (const u8*)sl.text.d_text.ptr, (const u32*)sl.text.d_line.ptr,
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
    if (h.status) {
        ctx->err = "gzip layout: more deflate blocks than the bound allows";
        return FPL_ERR_STATE;
    }
    if (h.total == 0) return FPL_OK;
    const u32 n = sl.n_reads;
    const uint64_t out_want = GZ_MEMBER_EXTRA + h.total + (uint64_t)GZ_SLACK * h.n_blocks;
    FPL_HIP(g.d_comp.grow(h.total + 16, 4096));
    FPL_HIP(g.d_tmp.grow(out_want + 16, 4096));
    FPL_HIP(g.d_out.grow(out_want + 16, 4096));
    hipStream_t st = ctx->stream;
    if (bam_records(sl.kind))
        hipLaunchKernelGGL(k_gz_compose_bam, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.bam.d_bam.ptr,
                           (const uint64_t*)sl.bam.d_rec.ptr, (const u8*)sl.d_seq.ptr, (const u8*)sl.d_qual.ptr, (const uint64_t*)sl.d_off.ptr,
                           (const fpl_read_result*)sl.d_results.ptr, n, (const u64*)g.d_rec_off.ptr, g.d_comp.ptr, (u64)h.total);
    else
        hipLaunchKernelGGL(k_gz_compose, dim3(8 * ctx->n_cu), dim3(256), 0, st, (const u8*)sl.text.d_text.ptr, (const u32*)sl.text.d_line.ptr,
                           (const u32*)sl.text.d_nl.ptr, (const fpl_read_result*)sl.d_results.ptr, n, (const u64*)g.d_rec_off.ptr,
                           g.d_comp.ptr, (u64)h.total);
    const u32 grid = std::max<u32>(1u, std::min<u32>(h.n_blocks, 8u * ctx->n_cu));
    hipLaunchKernelGGL(k_gz_block, dim3(grid), dim3(GZ_THREADS), 0, st, (const u8*)g.d_comp.ptr, (const u64*)g.d_blk_start.ptr,
                       (const GzHeader*)g.d_hdr.ptr, g.d_tmp.ptr, g.d_blk_size.ptr, g.d_blk_crc.ptr);
    hipLaunchKernelGGL(k_gz_finish, dim3(1), dim3(1024), 0, st, (const u32*)g.d_blk_size.ptr, (const u32*)g.d_blk_crc.ptr,
                       (u64*)g.d_blk_off.ptr, g.d_hdr.ptr, g.d_out.ptr, (u64)out_want);
    hipLaunchKernelGGL(k_gz_compact, dim3(grid), dim3(GZ_THREADS), 0, st, (const u8*)g.d_tmp.ptr, (const u64*)g.d_blk_start.ptr,
                       (const u32*)g.d_blk_size.ptr, (const u64*)g.d_blk_off.ptr, (const GzHeader*)g.d_hdr.ptr, g.d_out.ptr, (u64)out_want);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipMemcpyAsync(g.h_hdr.ptr, g.d_hdr.ptr, sizeof(GzHeader), hipMemcpyDeviceToHost, st));
    FPL_HIP(hipEventRecord(g.ev, st));
    FPL_HIP(g.h_out.grow(out_want, 4096)); /* (beside the kernels) */
    FPL_HIP(hipEventSynchronize(g.ev));
    const GzHeader h2 = *g.h_hdr.ptr;
    if (h2.status || h2.gz_len == 0 || h2.gz_len > out_want) {
        ctx->err = "gzip member: the kernels report a size outside the bound";
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
    if (sl.gz) return gz_layout(ctx, sl, n); /* (on the compute stream) */
    return FPL_OK;
}
/* after an enqueue error: "nothing is in flight" is what the caller reads into it, and it recycles the host arrays at once.  Copies
   or kernels that did get enqueued before the failing call may still read them (and the slot): wait them out first. */
static void drain(fpl_ctx* ctx) {
    for (hipStream_t st : {ctx->s_h2d, ctx->s_parse, ctx->stream, ctx->s_d2h})
        if (st) (void)hipStreamSynchronize(st);
}
/* the offsets of read i rise and it is no longer than 2^31 - 1; max_len follows the longest read */
static inline bool read_len_ok(const uint64_t* off, u32 i, u32& max_len) {
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x7FFFFFFFull) return false;
    max_len = std::max(max_len, (u32)(off[i + 1] - off[i]));
    return true;
}

/* stage 2 of a text batch: the header is in -- enqueue the per-read kernels and the way back of the records and line starts */
/* (called by fpl_wait_text only: a submission never waits for a parse, so the next chunk's copy goes out behind this one's at
   once -- no round trip to the host between two chunks on the link -- and a batch that has only been peeked at is in no counter) */
static int text_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl) {
    if (sl.kind != BatchKind::Text || sl.text.stage != 1) return FPL_OK;
    sl.text.stage = 2;
    FPL_HIP(hipEventSynchronize(sl.ev_parsed));
    const TextHeader h = *sl.text.h_hdr.ptr;
    sl.n_reads = 0;
    if (h.status != 0 || h.n_records == 0) return FPL_OK; /* nothing to run: fpl_wait_text reports */
    const u32 n = h.n_records;
    if (!sl.text.h_line.holds(4 * (size_t)n)) FPL_HIP(regrow(sl.text.h_line.want(4 * grown(n, 16))));
    FPL_HIP(sl.h_results.grow(n, 1024));
    const int r = submit_tail(ctx, sl, sl.ev_parsed, n, h.n_bases, h.max_len);
    if (r == FPL_OK) sl.n_reads = n;
    return r;
}
int fpl_process_text_async(fpl_ctx* ctx, const uint8_t* text, uint64_t n_bytes) {
    if (!ctx || (n_bytes && !text)) return FPL_ERR_ARG;
    if (n_bytes > 0xFFFFFFF0ull) return FPL_ERR_ARG; /* (line positions are 32 bits wide: cut the file in smaller chunks) */
    if (ctx->submitted - ctx->waited >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    if (ctx->hcfg.defer) return FPL_ERR_STATE; /* (--break / --mask read their fragment lists batch by batch: the CSR entry points) */
    int r = FPL_OK;
    fpl_ctx::Slot& sl = ctx->slot[ctx->submitted % FPL_MAX_IN_FLIGHT];
    fpl_ctx::Slot::Text& t = sl.text;
    sl.kind = BatchKind::Text;
    sl.gz = ctx->text_gzip;
    t.stage = 2;
    t.cancelled = false;
    sl.n_reads = 0;
    sl.rc = FPL_OK;
    t.bytes = n_bytes;
    r = ensure_host_streams(ctx);
    if (r != FPL_OK) return r;
    r = ensure_text_slot(ctx, sl, n_bytes);
    if (r != FPL_OK) return r;
    if (n_bytes == 0) {
        memset(t.h_hdr.ptr, 0, sizeof(TextHeader));
        t.h_hdr.ptr->bad_record = ~0ull;
        ctx->submitted++;
        return FPL_OK;
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
    r = enqueue();
    if (r != FPL_OK) {
        drain(ctx);
        return r;
    }
    t.stage = 1;
    ctx->submitted++;
    return FPL_OK;
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

/* the oldest text batch in flight that is neither started nor cancelled: what fpl_peek_text / fpl_start_text / fpl_cancel_text act on */
static fpl_ctx::Slot* text_pending(fpl_ctx* ctx) {
    for (u32 k = ctx->waited; k != ctx->submitted; k++) {
        fpl_ctx::Slot& sl = ctx->slot[k % FPL_MAX_IN_FLIGHT];
        if (sl.kind == BatchKind::Text && sl.text.stage == 1 && !sl.text.cancelled) return &sl;
    }
    return nullptr;
}

int fpl_peek_text(fpl_ctx* ctx, fpl_text_result* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl = text_pending(ctx);
    if (!sl) return FPL_ERR_STATE;
    memset(out, 0, sizeof(*out));
    if (sl->rc != FPL_OK) return sl->rc;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipEventSynchronize(sl->ev_parsed));
    text_info(*sl, out);
    return FPL_OK;
}

int fpl_start_text(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl = text_pending(ctx);
    if (!sl) return FPL_ERR_STATE;
    if (sl->rc != FPL_OK) return sl->rc;
    FPL_HIP(hipSetDevice(ctx->device));
    const int r = text_continue(ctx, *sl);
    if (r != FPL_OK) sl->rc = r;
    return r;
}

int fpl_cancel_text(fpl_ctx* ctx) {
    if (!ctx) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl = text_pending(ctx);
    if (!sl) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    if (sl->rc == FPL_OK) FPL_HIP(hipEventSynchronize(sl->ev_parsed)); /* (its copy and parse read the caller's text) */
    sl->text.cancelled = true;
    sl->n_reads = 0;
    return FPL_OK;
}

int fpl_set_text_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    ctx->text_gzip = on != 0;
    return FPL_OK;
}

static int wait_text(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                     const uint8_t** gz, uint64_t* gz_len);
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
static int wait_text(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                     const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out) return FPL_ERR_ARG;
    if (ctx->submitted == ctx->waited) return FPL_ERR_STATE;
    fpl_ctx::Slot& sl = ctx->slot[ctx->waited % FPL_MAX_IN_FLIGHT];
    if (sl.kind != BatchKind::Text) return FPL_ERR_STATE; /* (a CSR or BAM batch: fpl_wait) */
    memset(out, 0, sizeof(*out));
    if (results) *results = nullptr;
    if (line_starts) *line_starts = nullptr;
    FPL_HIP(hipSetDevice(ctx->device));
    if (sl.text.cancelled) {
        ctx->waited++;
        out->status = FPL_TEXT_CANCELLED;
        out->bad_record = ~0ull;
        return FPL_OK;
    }
    if (sl.rc == FPL_OK) {
        const int r = text_continue(ctx, sl); /* (no-op when fpl_start_text did it) */
        if (r != FPL_OK) sl.rc = r;
    }
    ctx->waited++;
    if (sl.rc != FPL_OK) return sl.rc;
    text_info(sl, out);
    if (out->status != FPL_TEXT_OK || sl.n_reads == 0) return FPL_OK;
    if (gz && sl.gz) {
        const int r = gz_emit(ctx, sl, gz, gz_len);
        if (r != FPL_OK) return r;
    }
    FPL_HIP(hipEventSynchronize(sl.ev_done));
    if (results) *results = sl.h_results.ptr;
    if (line_starts) *line_starts = sl.text.h_line.ptr;
    return FPL_OK;
}

int fpl_in_flight(const fpl_ctx* ctx) { return ctx ? (int)(ctx->submitted - ctx->waited) : 0; }

/* gz != nullptr: fpl_wait_bam_gz -- the member of a gzip BAM batch is made before the records are handed over */
static int wait_batch(fpl_ctx* ctx, const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx) return FPL_ERR_ARG;
    if (ctx->submitted == ctx->waited) return FPL_ERR_STATE;
    fpl_ctx::Slot& sl = ctx->slot[ctx->waited % FPL_MAX_IN_FLIGHT];
    if (sl.kind == BatchKind::Text || sl.kind == BatchKind::BGZF) return FPL_ERR_STATE; /* (fpl_wait_text, fpl_wait_bgzf_bam) */
    ctx->waited++;
    if (sl.rc != FPL_OK) return sl.rc; /* nothing was enqueued behind the failure */
    if (sl.n_reads == 0) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    if (gz && sl.gz) {
        const int r = gz_emit(ctx, sl, gz, gz_len);
        if (r != FPL_OK) return r;
    }
    FPL_HIP(hipEventSynchronize(sl.ev_done));
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
int fpl_set_bam_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    if (on && ctx->hcfg.defer) return FPL_ERR_STATE; /* (--break / --mask write from fragment lists) */
    ctx->bam_gzip = on != 0;
    return FPL_OK;
}

int fpl_process_batch_async(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off,
                            uint32_t n_reads, fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    if (n_reads && (!seq || !qual || !off || !results)) return FPL_ERR_ARG;
    if (ctx->submitted - ctx->waited >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    /* --break / --mask: the fragment lists of the batch in flight live in buffers this batch's kernels reuse */
    if (ctx->hcfg.defer && ctx->submitted != ctx->waited) return FPL_ERR_STATE;
    /* (a text batch in flight keeps waiting for ITS wait: the kernels of this batch go first -- the order of the kernels is free,
       the slots are collected in the order of submission) */
    fpl_ctx::Slot& sl = ctx->slot[ctx->submitted % FPL_MAX_IN_FLIGHT];
    sl.kind = BatchKind::CSR;
    sl.gz = false;
    sl.n_reads = n_reads;
    sl.user_results = results;
    sl.rc = FPL_OK;
    if (n_reads == 0) {
        ctx->submitted++;
        return FPL_OK;
    }
    const uint64_t n_bytes = off[n_reads];
    u32 max_len = 0;
    for (u32 i = 0; i < n_reads; i++)
        if (!read_len_ok(off, i, max_len)) return FPL_ERR_ARG;
    int r = ensure_host_streams(ctx);
    if (r != FPL_OK) return r;
    r = ensure_slot(ctx, sl, n_reads, n_bytes);
    if (r != FPL_OK) return r;
    /* (the slot's previous batch has been waited for -- FPL_MAX_IN_FLIGHT slots, FIFO -- so its buffers are free) */
    auto enqueue = [&]() -> int {
        if (n_bytes) {
            FPL_HIP(hipMemcpyAsync(sl.d_seq.ptr, seq, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
            FPL_HIP(hipMemcpyAsync(sl.d_qual.ptr, qual, n_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        }
        FPL_HIP(hipMemcpyAsync(sl.d_off.ptr, off, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, ctx->s_h2d));
        FPL_HIP(hipEventRecord(sl.ev_h2d, ctx->s_h2d));
        return submit_tail(ctx, sl, sl.ev_h2d, n_reads, n_bytes, max_len);
    };
    r = enqueue();
    if (r != FPL_OK) {
        drain(ctx);
        return r;
    }
    ctx->submitted++;
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
    if (ctx->submitted - ctx->waited >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    if (ctx->hcfg.defer && ctx->submitted != ctx->waited) return FPL_ERR_STATE; /* (--break / --mask: as fpl_process_batch_async) */
    u32 max_len = 0;
    if (n_reads && bam_check(bam, n_bytes, rec_start, off, n_reads, &max_len) != FPL_OK) {
        ctx->err = "fpl_process_bam_async: a record does not lie inside the bytes given, or its l_seq disagrees with the offsets";
        return FPL_ERR_ARG;
    }
    fpl_ctx::Slot& sl = ctx->slot[ctx->submitted % FPL_MAX_IN_FLIGHT];
    sl.kind = BatchKind::BAM;
    sl.gz = ctx->bam_gzip;
    sl.n_reads = n_reads;
    sl.user_results = results;
    sl.rc = FPL_OK;
    if (n_reads == 0) {
        ctx->submitted++;
        return FPL_OK;
    }
    fpl_ctx::Slot::Bam& b = sl.bam;
    const uint64_t o_begin = off[0], o_end = off[n_reads];
    b.o_begin = o_begin;
    b.bases = o_end - o_begin;
    b.seq_out = seq_out;
    b.qual_out = qual_out;
    int r = ensure_host_streams(ctx);
    if (r != FPL_OK) return r;
    r = ensure_slot(ctx, sl, n_reads, o_end + 16); /* (the decode writes whole 16-byte words) */
    if (r != FPL_OK) return r;
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
    r = enqueue();
    if (r != FPL_OK) {
        drain(ctx);
        return r;
    }
    ctx->submitted++;
    return FPL_OK;
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
static bool bgzf_in_flight(const fpl_ctx* ctx) {
    for (u32 k = ctx->waited; k != ctx->submitted; k++)
        if (ctx->slot[k % FPL_MAX_IN_FLIGHT].kind == BatchKind::BGZF) return true;
    return false;
}
/* the walk's state and the tail buffer, made on first use (all zero: no tail, nothing refused) */
/* k_bgzf_inflate's grid: a wave per block; as many workgroups as the device keeps resident (the tables' LDS bounds them), the rest
   off the counter */
static inline u32 bgzf_grid(u32 n_blocks, u32 n_cu) {
    const u32 per_cu = std::max<u32>(1, std::min<u32>(8, (u32)(160u * 1024 / (sizeof(BgzfWaveLds) * (BGZF_THREADS / WAVE) + 1024))));
    return std::min<u32>((n_blocks + BGZF_THREADS / WAVE - 1) / (BGZF_THREADS / WAVE), n_cu * per_cu);
}
/* room for a submission's names: a quarter of [tail room | inflated bytes] and 1 MiB, never more than all of it (a name is part of
   its record).  Records whose names take more than that are FPL_BAMW_TOO_MANY, as more than a record per 64 bytes is. */
static inline uint64_t bam_names_cap(uint64_t hi) { return std::min<uint64_t>(hi, hi / 4 + (1u << 20)); }
static int ensure_bam_tail(fpl_ctx* ctx) {
    if (!ctx->d_bamw_state.ptr) {
        FPL_HIP(ctx->d_bamw_state.alloc(1));
        FPL_HIP(hipMemset(ctx->d_bamw_state.ptr, 0, sizeof(BamWalkState)));
    }
    if (!ctx->d_bam_tail.ptr) FPL_HIP(ctx->d_bam_tail.alloc((size_t)std::max<uint64_t>(ctx->bam_tail_cap, 1)));
    return FPL_OK;
}

int fpl_process_bgzf_bam_async(fpl_ctx* ctx, const uint8_t* comp, uint64_t comp_bytes, const fpl_bgzf_block* blocks, uint32_t n_blocks,
                               uint64_t skip) {
    if (!ctx || (n_blocks && !blocks) || (comp_bytes && !comp)) return FPL_ERR_ARG;
    if (ctx->submitted - ctx->waited >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    if (ctx->hcfg.defer) return FPL_ERR_STATE; /* (--break / --mask read their fragment lists batch by batch: the CSR entry points) */
    if (skip && !ctx->bam_fresh) {
        ctx->err = "fpl_process_bgzf_bam_async: skip is valid only while the context holds no tail";
        return FPL_ERR_ARG;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_blocks; i++) { /* every range, before anything is enqueued; in order and without gaps */
        const fpl_bgzf_block& d = blocks[i];
        if (d.comp_len > BGZF_MAX_COMP || d.isize > BGZF_MAX_ISIZE || d.comp_off > comp_bytes || comp_bytes - d.comp_off < d.comp_len ||
            d.out_off != total)
            return FPL_ERR_ARG;
        total += d.isize;
        if (total > 0xFFFFFFF0ull) return FPL_ERR_ARG;
    }
    BamWalkJob j;
    if (!bam_walk_plan(j, ctx->bam_tail_cap, total, skip, ctx->bam_seg_bytes)) return FPL_ERR_ARG;
    fpl_ctx::Slot& sl = ctx->slot[ctx->submitted % FPL_MAX_IN_FLIGHT];
    fpl_ctx::Slot::Bam& b = sl.bam;
    sl.kind = BatchKind::BGZF;
    sl.gz = ctx->bam_gzip;
    sl.n_reads = 0;
    sl.user_results = nullptr;
    sl.rc = FPL_OK;
    b.stage = 0;
    b.o_begin = b.bases = 0;
    b.seq_out = b.qual_out = nullptr;
    int r = ensure_host_streams(ctx);
    if (r != FPL_OK) return r;
    r = ensure_bam_tail(ctx);
    if (r != FPL_OK) return r;
    const u32 rec_cap = bam_walk_rec_cap(total);
    const uint64_t hi = j.tail_cap + total;
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
        if (n_blocks) {
            FPL_HIP(hipMemsetAsync(b.d_next.ptr, 0, sizeof(u32), st));
            const u32 grid = bgzf_grid(n_blocks, ctx->n_cu);
            hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZF_THREADS), 0, st, (const u8*)b.d_comp.ptr, b.d_blocks.ptr, n_blocks,
                               b.d_bam.ptr + j.tail_cap, b.d_next.ptr);
        }
        bam_walk_enqueue(j, st);
        FPL_HIP(hipGetLastError());
        FPL_HIP(hipMemcpyAsync(b.h_whdr.ptr, b.d_whdr.ptr, sizeof(fpl_bam_window), hipMemcpyDeviceToHost, st));
        FPL_HIP(hipEventRecord(sl.ev_parsed, st));
        return FPL_OK;
    };
    r = enqueue();
    if (r != FPL_OK) {
        drain(ctx);
        return r;
    }
    b.stage = 1;
    ctx->bam_fresh = false;
    ctx->submitted++;
    return FPL_OK;
}

/* stage 2 of a BGZF batch: the header is in -- the decode, the per-read kernels, the way back of the records and the names */
static int bgzf_continue(fpl_ctx* ctx, fpl_ctx::Slot& sl, uint8_t* seq_out, uint8_t* qual_out) {
    fpl_ctx::Slot::Bam& b = sl.bam;
    if (sl.kind != BatchKind::BGZF || b.stage != 1) return FPL_OK;
    b.stage = 2;
    FPL_HIP(hipEventSynchronize(sl.ev_parsed));
    const fpl_bam_window h = *b.h_whdr.ptr;
    sl.n_reads = 0;
    if (h.status != FPL_BAMW_OK || h.n_reads == 0) return FPL_OK; /* nothing to run: the wait reports */
    const u32 n = h.n_reads;
    b.o_begin = 0;
    b.bases = h.n_bases;
    b.seq_out = seq_out;
    b.qual_out = qual_out;
    int r = ensure_slot(ctx, sl, n, h.n_bases + 16); /* (the decode writes whole 16-byte words; d_off / d_results hold rec_cap already) */
    if (r != FPL_OK) return r;
    FPL_HIP(b.h_names.grow((size_t)h.name_bytes + 1, 4096));
    FPL_HIP(b.h_name_off.grow((size_t)n + 1, 1024));
    FPL_HIP(hipStreamWaitEvent(ctx->stream, sl.ev_parsed, 0));
    bam_launch(b.d_bam.ptr, b.d_rec.ptr, sl.d_off.ptr, n, 0, h.n_bases, sl.d_seq.ptr, sl.d_qual.ptr, ctx->stream);
    FPL_HIP(hipGetLastError());
    FPL_HIP(hipEventRecord(sl.ev_parsed, ctx->stream)); /* (from here on: the bases are decoded, as for a BAM batch) */
    FPL_HIP(hipMemcpyAsync(b.h_names.ptr, b.d_names.ptr, (size_t)h.name_bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
    FPL_HIP(hipMemcpyAsync(b.h_name_off.ptr, b.d_name_off.ptr, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->s_d2h));
    r = submit_tail(ctx, sl, sl.ev_parsed, n, h.n_bases, h.max_read_len);
    if (r == FPL_OK) sl.n_reads = n;
    return r;
}

/* the oldest BGZF batch in flight that is not started: what fpl_peek_bgzf_bam / fpl_start_bgzf_bam act on */
static fpl_ctx::Slot* bgzf_pending(fpl_ctx* ctx) {
    for (u32 k = ctx->waited; k != ctx->submitted; k++) {
        fpl_ctx::Slot& sl = ctx->slot[k % FPL_MAX_IN_FLIGHT];
        if (sl.kind == BatchKind::BGZF && sl.bam.stage == 1) return &sl;
    }
    return nullptr;
}

int fpl_peek_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl = bgzf_pending(ctx);
    if (!sl) return FPL_ERR_STATE;
    memset(out, 0, sizeof(*out));
    if (sl->rc != FPL_OK) return sl->rc;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipEventSynchronize(sl->ev_parsed));
    *out = *sl->bam.h_whdr.ptr;
    return FPL_OK;
}

int fpl_start_bgzf_bam(fpl_ctx* ctx, uint8_t* seq_out, uint8_t* qual_out) {
    if (!ctx || (!seq_out) != (!qual_out)) return FPL_ERR_ARG;
    fpl_ctx::Slot* sl = bgzf_pending(ctx);
    if (!sl) return FPL_ERR_STATE;
    if (sl->rc != FPL_OK) return sl->rc;
    FPL_HIP(hipSetDevice(ctx->device));
    const int r = bgzf_continue(ctx, *sl, seq_out, qual_out);
    if (r != FPL_OK) sl->rc = r;
    return r;
}

int fpl_wait_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out, const fpl_read_result** results, const uint8_t** names, const uint64_t** name_off,
                      const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out || (!gz) != (!gz_len)) return FPL_ERR_ARG;
    if (ctx->submitted == ctx->waited) return FPL_ERR_STATE;
    fpl_ctx::Slot& sl = ctx->slot[ctx->waited % FPL_MAX_IN_FLIGHT];
    if (sl.kind != BatchKind::BGZF) return FPL_ERR_STATE; /* (fpl_wait, fpl_wait_text) */
    memset(out, 0, sizeof(*out));
    if (results) *results = nullptr;
    if (names) *names = nullptr;
    if (name_off) *name_off = nullptr;
    if (gz) {
        *gz = nullptr;
        *gz_len = 0;
    }
    FPL_HIP(hipSetDevice(ctx->device));
    if (sl.rc == FPL_OK) {
        const int r = bgzf_continue(ctx, sl, nullptr, nullptr); /* (no-op when fpl_start_bgzf_bam did it) */
        if (r != FPL_OK) sl.rc = r;
    }
    ctx->waited++;
    if (sl.rc != FPL_OK) return sl.rc;
    *out = *sl.bam.h_whdr.ptr;
    if (out->status != FPL_BAMW_OK || sl.n_reads == 0) return FPL_OK;
    if (gz && sl.gz) {
        const int r = gz_emit(ctx, sl, gz, gz_len);
        if (r != FPL_OK) return r;
    }
    FPL_HIP(hipEventSynchronize(sl.ev_done));
    if (results) *results = sl.h_results.ptr;
    if (names) *names = sl.bam.h_names.ptr;
    if (name_off) *name_off = sl.bam.h_name_off.ptr;
    return FPL_OK;
}

/* (the recovery calls run with no BGZF batch in flight: every walk is done -- its header was waited for -- and the state is at rest) */
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
    const int r = ensure_bam_tail(ctx);
    if (r != FPL_OK) return r;
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
    const int r = bam_state_update(ctx, true, len);
    if (r != FPL_OK) return r;
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

/* ---- BGZF inflate (bgzf_inflate.h): a handle of its own, no context ---- */
struct fpl_inflater {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf<u8> d_comp, d_out;
    DevBuf<fpl_bgzf_block> d_blocks;
    DevBuf<u32> d_next; /* the kernel's work counter */
    int n_cu = 0;
    std::vector<std::pair<uint64_t, uint64_t>> runs; /* output ranges to bring back, merged */
    /* fpl_inflate_gzip (gzip_inflate.h): the chunks' records, their rooms of 16-bit elements, the 32 KiB windows, the result */
    DevBuf<GzipChunk> d_chunks;
    DevBuf<unsigned short> d_room;
    DevBuf<u8> d_wins;
    DevBuf<fpl_gzip_window> d_res;
};

fpl_inflater* fpl_inflater_create(int32_t device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    fpl_inflater* inf = new (std::nothrow) fpl_inflater();
    if (!inf) return nullptr;
    inf->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || hipStreamCreateWithFlags(&inf->stream, hipStreamNonBlocking) != hipSuccess ||
        inf->d_next.alloc(1) != hipSuccess) {
        fpl_inflater_destroy(inf);
        return nullptr;
    }
    inf->n_cu = prop.multiProcessorCount;
    return inf;
}

void fpl_inflater_destroy(fpl_inflater* inf) {
    if (!inf) return;
    if (inf->device >= 0) (void)hipSetDevice(inf->device);
    if (inf->stream) {
        (void)hipStreamSynchronize(inf->stream);
        (void)hipStreamDestroy(inf->stream);
    }
    delete inf;
}

int fpl_inflate_bgzf(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                     uint64_t out_bytes) {
    if (!inf) return FPL_ERR_ARG;
    if (n_blocks == 0) return FPL_OK;
    if (!blocks || (comp_bytes && !comp) || (out_bytes && !out)) return FPL_ERR_ARG;
    inf->runs.clear();
    for (uint32_t i = 0; i < n_blocks; i++) { /* every range, before anything is enqueued */
        const fpl_bgzf_block& d = blocks[i];
        if (d.comp_len > BGZF_MAX_COMP || d.isize > BGZF_MAX_ISIZE || d.comp_off > comp_bytes || comp_bytes - d.comp_off < d.comp_len ||
            d.out_off > out_bytes || out_bytes - d.out_off < d.isize)
            return FPL_ERR_ARG;
        if (d.isize) inf->runs.emplace_back(d.out_off, d.out_off + d.isize);
    }
    std::sort(inf->runs.begin(), inf->runs.end());
    size_t n_runs = 0;
    for (const auto& r : inf->runs) { /* ranges that touch are one copy: a reader's window comes back in one */
        if (n_runs && r.first <= inf->runs[n_runs - 1].second)
            inf->runs[n_runs - 1].second = std::max(inf->runs[n_runs - 1].second, r.second);
        else
            inf->runs[n_runs++] = r;
    }
    FPL_HIP_RC(hipSetDevice(inf->device));
    FPL_HIP_RC(inf->d_comp.grow((size_t)comp_bytes + 1, 4096));
    FPL_HIP_RC(inf->d_out.grow((size_t)out_bytes + 1, 4096));
    FPL_HIP_RC(inf->d_blocks.grow(n_blocks, 64));
    hipStream_t s = inf->stream;
    if (comp_bytes) FPL_HIP_RC(hipMemcpyAsync(inf->d_comp.ptr, comp, comp_bytes, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(hipMemcpyAsync(inf->d_blocks.ptr, blocks, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(hipMemsetAsync(inf->d_next.ptr, 0, sizeof(u32), s));
    const u32 grid = bgzf_grid(n_blocks, (u32)inf->n_cu);
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(BGZF_THREADS), 0, s, (const u8*)inf->d_comp.ptr, inf->d_blocks.ptr, n_blocks, inf->d_out.ptr,
                       inf->d_next.ptr);
    FPL_HIP_RC(hipGetLastError());
    for (size_t k = 0; k < n_runs; k++)
        FPL_HIP_RC(hipMemcpyAsync(out + inf->runs[k].first, inf->d_out.ptr + inf->runs[k].first, inf->runs[k].second - inf->runs[k].first,
                                  hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipMemcpyAsync(blocks, inf->d_blocks.ptr, sizeof(fpl_bgzf_block) * (size_t)n_blocks, hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipStreamSynchronize(s));
    return FPL_OK;
}

int fpl_inflate_gzip(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, uint64_t start_bit, const uint8_t* dict, uint32_t dict_len,
                     uint8_t* out, uint64_t out_cap, uint32_t chunk_bytes, fpl_gzip_window* res) {
    GzipJob job;
    if (!inf || !res || !comp || (dict_len && !dict) || (out_cap && !out) ||
        !gzip_plan(job, comp_bytes, start_bit, dict_len, out_cap, chunk_bytes)) /* every argument, before anything is enqueued */
        return FPL_ERR_ARG;
    const uint64_t skip = start_bit >> 3;
    const size_t room = (size_t)job.n_chunks * job.room_per_chunk + job.room0_extra;
    const size_t out_room = (size_t)std::min<uint64_t>(out_cap, room); /* (a byte per element at most) */
    FPL_HIP_RC(hipSetDevice(inf->device));
    FPL_HIP_RC(inf->d_comp.grow((size_t)job.comp_len + 1, 4096));
    FPL_HIP_RC(inf->d_out.grow(out_room + 1, 4096));
    FPL_HIP_RC(inf->d_chunks.grow(job.n_chunks, 64));
    FPL_HIP_RC(inf->d_room.grow(room, 4096));
    FPL_HIP_RC(inf->d_wins.grow(((size_t)job.n_chunks + 1) * GZIP_WINDOW, 4096));
    if (!inf->d_res.ptr) FPL_HIP_RC(inf->d_res.alloc(1));
    job.comp = inf->d_comp.ptr;
    job.chunks = inf->d_chunks.ptr;
    job.room = inf->d_room.ptr;
    job.wins = inf->d_wins.ptr;
    job.out = inf->d_out.ptr;
    job.res = inf->d_res.ptr;
    job.out_cap = out_room;
    hipStream_t s = inf->stream;
    FPL_HIP_RC(hipMemcpyAsync(inf->d_comp.ptr, comp + skip, job.comp_len, hipMemcpyHostToDevice, s));
    FPL_HIP_RC(hipMemsetAsync(inf->d_wins.ptr, 0, GZIP_WINDOW, s));
    if (dict_len) FPL_HIP_RC(hipMemcpyAsync(inf->d_wins.ptr + (GZIP_WINDOW - dict_len), dict, dict_len, hipMemcpyHostToDevice, s));
    gzip_enqueue(job, (u32)inf->n_cu, s);
    FPL_HIP_RC(hipGetLastError());
    /* the result first: it says how many bytes to bring back */
    FPL_HIP_RC(hipMemcpyAsync(res, inf->d_res.ptr, sizeof(fpl_gzip_window), hipMemcpyDeviceToHost, s));
    FPL_HIP_RC(hipStreamSynchronize(s));
    if (res->status == FPL_GZIP_OK && res->out_bytes) {
        if (res->out_bytes > out_room) return FPL_ERR_HIP; /* (cannot be: k_gzip_windows checks every chunk against out_cap) */
        FPL_HIP_RC(hipMemcpyAsync(out, inf->d_out.ptr, res->out_bytes, hipMemcpyDeviceToHost, s));
        FPL_HIP_RC(hipStreamSynchronize(s));
    }
    res->end_bit += 8 * skip;
    return FPL_OK;
}

int fpl_process_batch(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint32_t n_reads,
                      fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    if (ctx->submitted != ctx->waited) return FPL_ERR_STATE; /* (collect the asynchronous batches first) */
    if (n_reads == 0) return FPL_OK;
    const int r = fpl_process_batch_async(ctx, seq, qual, off, n_reads, results);
    if (r != FPL_OK) return r;
    return fpl_wait(ctx);
}

/* Large blocks (a host's batch arenas: hundreds of megabytes) are anonymous memory on transparent huge pages, touched once from a few
   threads and then registered with the runtime: page-locking goes page by page, and hipHostMalloc locks 4 KB pages at 4 GB/s -- 0.18 s
   for the CLI's 740 MB arena, every run, before the first byte is read; 370 huge pages are touched in 11 ms and registered in 1.5 ms,
   and the DMA engines read them at the same 56 GB/s (tools/pin_probe.cpp).  Without huge pages (THP off) the same path costs what
   hipHostMalloc costs.  Small blocks, and any failure on the way, take hipHostMalloc.  FPL_NO_HUGE_PIN: measurement hook. */
namespace {
struct HugeBlocks {
    std::mutex mu;
    std::map<void*, std::pair<void*, size_t>> m; /* registered address -> (mapping, its length) */
};
HugeBlocks* huge_blocks() {
    static HugeBlocks* h = new HugeBlocks; /* (never destroyed: a buffer may be freed from a static's destructor) */
    return h;
}
constexpr size_t HUGE_PAGE = 2u << 20;
constexpr size_t HUGE_MIN = 8u << 20;
}  // namespace
void* fpl_host_alloc(size_t bytes) {
    if (bytes >= HUGE_MIN && !getenv("FPL_NO_HUGE_PIN")) {
        const size_t len = (bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1);
        void* const m = mmap(nullptr, len + HUGE_PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m != MAP_FAILED) {
            char* const a = (char*)(((size_t)m + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1));
            (void)madvise(a, len, MADV_HUGEPAGE);
            /* first touch (the kernel clears a huge page per fault): a few threads side by side, one byte per small page */
            const int nt = (int)std::min<size_t>(4, len / (64u << 20) + 1);
            auto touch = [a, len, nt](int t) {
                const size_t lo = len / HUGE_PAGE * (size_t)t / (size_t)nt * HUGE_PAGE, hi = len / HUGE_PAGE * (size_t)(t + 1) / (size_t)nt * HUGE_PAGE;
                for (size_t o = lo; o < hi; o += 4096) ((volatile char*)a)[o] = 0;
            };
            std::vector<std::thread> th;
            for (int t = 1; t < nt; t++) th.emplace_back(touch, t);
            touch(0);
            for (auto& x : th) x.join();
            if (hipHostRegister(a, len, hipHostRegisterPortable) == hipSuccess) {
                HugeBlocks& h = *huge_blocks();
                std::lock_guard<std::mutex> g(h.mu);
                h.m[a] = std::make_pair(m, len + HUGE_PAGE);
                return a;
            }
            (void)hipGetLastError();
            munmap(m, len + HUGE_PAGE);
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void fpl_host_free(void* p) {
    if (!p) return;
    {
        HugeBlocks& h = *huge_blocks();
        std::unique_lock<std::mutex> g(h.mu);
        auto it = h.m.find(p);
        if (it != h.m.end()) {
            const std::pair<void*, size_t> mp = it->second;
            h.m.erase(it);
            g.unlock();
            (void)hipHostUnregister(p);
            munmap(mp.first, mp.second);
            return;
        }
    }
    (void)hipHostFree(p);
}

int fpl_enable_timing(fpl_ctx* ctx, int enable) {
    if (!ctx) return FPL_ERR_ARG;
    if (enable && !ctx->ev_ready) { /* all or nothing: a ring with holes would hand null events to hipEventRecord later */
        FPL_HIP(hipSetDevice(ctx->device));
        hipError_t bad = hipSuccess;
        for (int r = 0; r < fpl_ctx::EV_RING && bad == hipSuccess; r++)
            for (int i = 0; i <= N_STAGES && bad == hipSuccess; i++) bad = hipEventCreate(&ctx->ev[r][i]);
        if (bad != hipSuccess) {
            for (int r = 0; r < fpl_ctx::EV_RING; r++)
                for (int i = 0; i <= N_STAGES; i++) {
                    if (ctx->ev[r][i]) (void)hipEventDestroy(ctx->ev[r][i]);
                    ctx->ev[r][i] = nullptr;
                }
            ctx->timing = 0;
            FPL_HIP(bad);
        }
        ctx->ev_ready = true;
    }
    ctx->timing = enable ? 1 : 0;
    ctx->ev_calls = 0;
    return FPL_OK;
}

int fpl_get_kernel_times(fpl_ctx* ctx, float* ms, const char** names, int* n, int* n_batches) {
    if (!ctx || !ms || !n) return FPL_ERR_ARG;
    if (ctx->ev_calls <= 0) return FPL_ERR_STATE;
    FPL_HIP(hipSetDevice(ctx->device));
    const int calls = ctx->ev_calls < fpl_ctx::EV_RING ? ctx->ev_calls : fpl_ctx::EV_RING;
    for (int i = 0; i < N_STAGES; i++) ms[i] = 0.f;
    for (int c = 0; c < calls; c++) {
        const int slot = (ctx->ev_calls - 1 - c) % fpl_ctx::EV_RING;
        FPL_HIP(hipEventSynchronize(ctx->ev[slot][N_STAGES]));
        for (int i = 0; i < N_STAGES; i++) {
            float t = 0.f;
            FPL_HIP(hipEventElapsedTime(&t, ctx->ev[slot][i], ctx->ev[slot][i + 1]));
            ms[i] += t;
        }
    }
    for (int i = 0; i < N_STAGES; i++)
        if (names) names[i] = STAGE_NAMES[i];
    *n = N_STAGES;
    if (n_batches) *n_batches = calls;
    return FPL_OK;
}

} /* extern "C" */

extern "C" int fpl_fragment_counts(fpl_ctx* ctx, uint32_t* n_fragments, uint32_t* n_regions) {
    if (!ctx || !n_fragments || !n_regions) return FPL_ERR_ARG;
    *n_fragments = *n_regions = 0;
    if (!ctx->hcfg.defer || !ctx->d_bm_counts.ptr) return FPL_OK;
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipDeviceSynchronize());
    u32 c[4] = {0, 0, 0, 0};
    FPL_HIP(hipMemcpy(c, ctx->d_bm_counts.ptr, sizeof(c), hipMemcpyDeviceToHost));
    if (c[2]) {
        ctx->err = "break/mask lists overflowed their capacity";
        return FPL_ERR_CAPACITY;
    }
    *n_fragments = c[0];
    *n_regions = c[1];
    return FPL_OK;
}

extern "C" int fpl_get_fragments(fpl_ctx* ctx, fpl_fragment* fragments, uint32_t n_fragments, fpl_region* regions,
                                 uint32_t n_regions) {
    if (!ctx || (n_fragments && !fragments) || (n_regions && !regions)) return FPL_ERR_ARG;
    uint32_t nf = 0, nr = 0;
    int r = fpl_fragment_counts(ctx, &nf, &nr);
    if (r != FPL_OK) return r;
    if (n_fragments < nf || n_regions < nr) return FPL_ERR_ARG;
    if (nf) FPL_HIP(hipMemcpy(fragments, ctx->d_bm_frags.ptr, sizeof(fpl_fragment) * (size_t)nf, hipMemcpyDeviceToHost));
    if (nr) FPL_HIP(hipMemcpy(regions, ctx->d_bm_regs.ptr, sizeof(fpl_region) * (size_t)nr, hipMemcpyDeviceToHost));
    std::sort(fragments, fragments + nf, [](const fpl_fragment& a, const fpl_fragment& b) {
        return a.read != b.read ? a.read < b.read : a.seq_no < b.seq_no;
    });
    return FPL_OK;
}

#ifdef FPL_PROF
/* profiling builds only: read (and clear) the section timers the kernels accumulate */
extern "C" int fpl_debug_prof(unsigned long long* out, int n) {
    unsigned long long tmp[64];
    if (hipMemcpyFromSymbol(tmp, HIP_SYMBOL(fpl::g_fpl_prof), sizeof(tmp)) != hipSuccess) return -1;
    for (int i = 0; i < n && i < 64; i++) out[i] = tmp[i];
    memset(tmp, 0, sizeof(tmp));
    if (hipMemcpyToSymbol(HIP_SYMBOL(fpl::g_fpl_prof), tmp, sizeof(tmp)) != hipSuccess) return -1;
    return 0;
}
#endif

/* the counting of the detection: tables in device memory, freed with the caller's KmerTables */
struct KmerTables {
    DevBuf<u8> d_seq;
    DevBuf<uint64_t> d_off;
    DevBuf<u32> d_counts;
    DevBuf<unsigned long long> d_pos, d_total;
};
static int count_end_kmers_device(int32_t device, const uint8_t* seq, const uint64_t* off, uint32_t n_reads, int32_t side,
                                  int32_t shift_tail, KmerTables& t) {
    if (!off || (n_reads && !seq) || side < 0 || side > 1 || shift_tail < 0) return FPL_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) return FPL_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FPL_ERR_NO_DEVICE;
    const size_t n_keys = (size_t)pick::NKEYS;
    const uint64_t n_bytes = n_reads ? off[n_reads] : 0;
    int rc = FPL_OK;
    auto ok = [&](hipError_t e) {
        if (e != hipSuccess && rc == FPL_OK) rc = FPL_ERR_HIP;
        return e == hipSuccess;
    };
    if (ok(t.d_seq.alloc(n_bytes ? n_bytes : 1)) && ok(t.d_off.alloc((size_t)n_reads + 1)) && ok(t.d_counts.alloc(n_keys)) &&
        ok(t.d_pos.alloc(n_keys)) && ok(t.d_total.alloc(1))) {
        ok(hipMemcpy(t.d_seq.ptr, seq, n_bytes, hipMemcpyHostToDevice));
        ok(hipMemcpy(t.d_off.ptr, off, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice));
        ok(hipMemset(t.d_counts.ptr, 0, sizeof(u32) * n_keys));
        ok(hipMemset(t.d_pos.ptr, 0, sizeof(unsigned long long) * n_keys));
        ok(hipMemset(t.d_total.ptr, 0, sizeof(unsigned long long)));
        if (rc == FPL_OK && n_reads) {
            u32 blocks = (n_reads + 3) / 4;
            if (blocks > 8192) blocks = 8192;
            hipLaunchKernelGGL(k_count_end_kmers, dim3(blocks), dim3(256), 0, 0, (const u8*)t.d_seq.ptr, (const uint64_t*)t.d_off.ptr, n_reads,
                               (int)side, (int)shift_tail, t.d_counts.ptr, t.d_pos.ptr, t.d_total.ptr);
            ok(hipGetLastError());
        }
    }
    return rc;
}

int fpl_count_end_kmers(int32_t device, const uint8_t* seq, const uint64_t* off, uint32_t n_reads, int32_t side, int32_t shift_tail,
                        uint32_t* counts, uint64_t* position_acc, uint64_t* total) {
    if (!counts || !position_acc || !total) return FPL_ERR_ARG;
    KmerTables t;
    int rc = count_end_kmers_device(device, seq, off, n_reads, side, shift_tail, t);
    if (rc == FPL_OK) {
        const size_t n_keys = (size_t)pick::NKEYS;
        if (hipMemcpy(counts, t.d_counts.ptr, sizeof(u32) * n_keys, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(position_acc, t.d_pos.ptr, sizeof(unsigned long long) * n_keys, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(total, t.d_total.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
            rc = FPL_ERR_HIP;
    }
    return rc;
}

static_assert(sizeof(fpl_adapter_pick) >= sizeof(pick::Pick) && sizeof(((fpl_adapter_pick*)0)->seq) >= sizeof(((pick::Pick*)0)->seq),
              "the ABI record holds what the kernel writes");
int fpl_pick_adapter(int32_t device, const uint8_t* seq, const uint64_t* off, uint32_t n_reads, int32_t side, int32_t shift_tail,
                     int32_t is_rna, fpl_adapter_pick* out) {
    if (!out) return FPL_ERR_ARG;
    KmerTables t;
    DevBuf<pick::Pick> d_pick;
    int rc = count_end_kmers_device(device, seq, off, n_reads, side, shift_tail, t);
    if (rc == FPL_OK && d_pick.alloc(1) != hipSuccess) rc = FPL_ERR_HIP;
    if (rc == FPL_OK) {
        hipLaunchKernelGGL(k_pick_adapter, dim3(1), dim3(1024), 0, 0, (const u32*)t.d_counts.ptr,
                           (const unsigned long long*)t.d_pos.ptr, (int)(is_rna != 0), d_pick.ptr);
        pick::Pick p;
        unsigned long long total = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpy(&p, d_pick.ptr, sizeof(p), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(&total, t.d_total.ptr, sizeof(total), hipMemcpyDeviceToHost) != hipSuccess)
            rc = FPL_ERR_HIP;
        else {
            memset(out, 0, sizeof(*out));
            out->key = p.key;
            out->count = p.count;
            out->total_key = p.total_key;
            out->len = p.len;
            out->total = total;
            memcpy(out->seq, p.seq, sizeof(p.seq));
        }
    }
    return rc;
}

#ifdef FPL_PROF_BLOCKS
extern "C" int fpl_debug_read_blockprof(void* dst, size_t bytes) {
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(fpl::g_blockprof), bytes) == hipSuccess ? 0 : -1;
}
#endif
