/* rt_merge.h -- the counters of several contexts summed across their devices: RCCL loaded on first use, the communicators kept
   between merges, the all-reduce. */
#pragma once

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
    FPL_TRY(check_merge_args(ctxs, n));
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
    FPL_TRY(check_merge_args(ctxs, n));
    fpl_ctx* ctx = ctxs[0]; /* (FPL_HIP reports through this one) */
    u32 C = 0;
    for (int i = 0; i < n; i++) {
        if (ctxs[i]->submitted != ctxs[i]->waited) return FPL_ERR_STATE;
        C = std::max(C, ctxs[i]->C);
    }
    for (int i = 0; i < n; i++) {
        FPL_TRY(fpl_reserve_cycles(ctxs[i], C));
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
