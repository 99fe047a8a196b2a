/* rt_misc.h -- what stands beside the batch paths: page-locked host memory, kernel timing, the fragment lists of --break / --mask,
   the k-mer counting and adapter pick of the detection, and the debug reads of profiling builds. */
#pragma once

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
            for (int i = 0; i <= N_STAGES && bad == hipSuccess; i++) bad = ctx->ev[r][i].create(hipEventDefault);
        if (bad != hipSuccess) {
            for (int r = 0; r < fpl_ctx::EV_RING; r++)
                for (int i = 0; i <= N_STAGES; i++) ctx->ev[r][i].reset();
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

int fpl_fragment_counts(fpl_ctx* ctx, uint32_t* n_fragments, uint32_t* n_regions) {
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

int fpl_get_fragments(fpl_ctx* ctx, fpl_fragment* fragments, uint32_t n_fragments, fpl_region* regions,
                                 uint32_t n_regions) {
    if (!ctx || (n_fragments && !fragments) || (n_regions && !regions)) return FPL_ERR_ARG;
    uint32_t nf = 0, nr = 0;
    FPL_TRY(fpl_fragment_counts(ctx, &nf, &nr));
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
