/*
 * fpl_hip.hip -- the C-ABI of include/fastplong_amd.h on top of the gfx950 kernels: THE translation unit of the library.
 * Built by hipcc only (--offload-arch=gfx950); there is no CPU path in this library.
 *
 * The host code lives in the rt_*.h units included below, once each and in this order (a unit uses what the ones above it
 * define; all but the context's definition stand inside this file's extern "C" block, as its own code does); this file keeps
 * what makes and ends a context, and the calls around its counters.
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
#include "bam_emit.h"
#include "bam_tags.h"
#include "bam_mods.h"
#include "bam_moves.h"
#include "bam_comments.h"
#include "bam_decode.h"
#include "bgzf_inflate.h"
#include "bam_walk.h"
#include "text_walk.h"
#include "gzip_inflate.h"
#include "emit.h"

using namespace fpl;

#include "rt_ctx.h"

extern "C" {

#include "rt_batch.h"
#include "rt_slots.h"
#include "rt_text.h"
#include "rt_bam.h"
#include "rt_bgzf_text.h"
#include "rt_inflater.h"
#include "rt_merge.h"
#include "rt_misc.h"

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
        FPL_HIP(ctx->s_aux.create());
        FPL_HIP(ctx->s_trim.create());
        for (Event* e : {&ctx->ev_trim_done, &ctx->ev_batch_done[0], &ctx->ev_batch_done[1], &ctx->ev_stats_done[0], &ctx->ev_stats_done[1],
                         &ctx->ev_fork, &ctx->ev_join})
            FPL_HIP(e->create());
        if (const char* e = getenv("FPL_TRIM_AHEAD_GATE")) ctx->ahead_gate = atoi(e);
        if (const char* e = getenv("FPL_NO_TRIM_AHEAD")) ctx->trim_ahead = atoi(e) == 0;
        if (const char* e = getenv("FPL_NO_OVERLAP")) ctx->overlap = atoi(e) == 0;
        if (const char* e = getenv("FPL_BAM_SEG_BYTES")) { /* (a test hook: small segments; a value the walk cannot use is ignored) */
            const long v = atol(e);
            ctx->bam_seg_bytes = v >= (long)BAMW_MIN_SEG && v <= (1l << 30) ? (u32)v : 0;
        }
        for (auto& sl : ctx->slot)
            for (Event* e : {&sl.ev_h2d, &sl.ev_kern, &sl.ev_done, &sl.ev_parsed, &sl.gzip.ev}) FPL_HIP(e->create());
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
        FPL_TRY(alloc_counters(ctx, ctx->C, ctx->d_counters));
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
    /* (the buffers, events and streams of the context and of its slots go with the `delete` below) */
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
    FPL_TRY(alloc_counters(ctx, Cn, nw));
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

int fpl_get_bam_tag_stats(fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    for (int k = 0; k < 4; k++) out[k] = 0;
    if (!ctx->d_tag_counters.ptr) return FPL_OK; /* (no batch has carried tags yet) */
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipStreamSynchronize(ctx->stream)); /* (k_bam_tags of every batch submitted so far has added its share) */
    unsigned long long c[4];
    FPL_HIP(hipMemcpy(c, ctx->d_tag_counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = c[k];
    return FPL_OK;
}

int fpl_get_bam_mod_stats(fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    for (int k = 0; k < 4; k++) out[k] = 0;
    if (!ctx->d_mod_counters.ptr) return FPL_OK; /* (no batch has re-indexed anything yet) */
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipStreamSynchronize(ctx->stream)); /* (k_bam_mods_plan of every batch submitted so far has added its share) */
    unsigned long long c[4];
    FPL_HIP(hipMemcpy(c, ctx->d_mod_counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = c[k];
    return FPL_OK;
}

int fpl_get_bam_comment_stats(fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    for (int k = 0; k < 4; k++) out[k] = 0;
    if (!ctx->d_note_counters.ptr) return FPL_OK; /* (no batch has carried comments yet) */
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipStreamSynchronize(ctx->stream)); /* (k_bam_comment_len of every batch submitted so far has added its share) */
    unsigned long long c[4];
    FPL_HIP(hipMemcpy(c, ctx->d_note_counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = c[k];
    return FPL_OK;
}

int fpl_get_bam_move_stats(fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    for (int k = 0; k < 4; k++) out[k] = 0;
    if (!ctx->d_move_counters.ptr) return FPL_OK; /* (no batch has re-indexed anything yet) */
    FPL_HIP(hipSetDevice(ctx->device));
    FPL_HIP(hipStreamSynchronize(ctx->stream)); /* (k_bam_moves_plan of every batch submitted so far has added its share) */
    unsigned long long c[4];
    FPL_HIP(hipMemcpy(c, ctx->d_move_counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out[k] = c[k];
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

} /* extern "C" */
