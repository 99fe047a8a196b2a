/*
 * bgzf_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_bgzf/libfastplong_amd.so, built by tests/stub_bgzf/build.py).
 *
 * The stand-in library of tests/stub_bamgz (bamgz_stand_in.cpp, unchanged: compiled into this translation unit) plus the three
 * inflater calls, backed by the product's k_bgzf_inflate on the emulator (tests/emu_bgzf/driver.cpp, linked beside this file,
 * without sanitizers) -- so bin/fastplong_amd's --device_inflate path runs on a box without GPUs.
 * FPL_STUB_BGZF_LOG=<file>: "<device> inflate <blocks> <refused>" per call.
 */
#include "../stub_bamgz/bamgz_stand_in.cpp"

extern "C" int emu_bgzf_inflate(const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                                uint64_t out_bytes, uint32_t grid);

struct fpl_inflater {
    int device;
};

extern "C" fpl_inflater* fpl_inflater_create(int32_t device) {
    if (device < 0) return nullptr;
    return new fpl_inflater{device};
}

extern "C" void fpl_inflater_destroy(fpl_inflater* inf) { delete inf; }

extern "C" int fpl_inflate_bgzf(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks,
                                uint8_t* out, uint64_t out_bytes) {
    if (!inf) return FPL_ERR_ARG;
    if (n_blocks == 0) return FPL_OK;
    if (!blocks) return FPL_ERR_ARG;
    int rc;
    {
        std::lock_guard<std::mutex> g(g_emu_m); /* (the emulator's __shared__ is static storage) */
        rc = emu_bgzf_inflate(comp, comp_bytes, blocks, n_blocks, out, out_bytes, 0);
    }
    if (rc != 0) return FPL_ERR_ARG;
    if (const char* lf = getenv("FPL_STUB_BGZF_LOG")) {
        uint32_t refused = 0;
        for (uint32_t i = 0; i < n_blocks; i++) refused += blocks[i].status != 0;
        std::lock_guard<std::mutex> g(g_log_m);
        if (FILE* f = fopen(lf, "a")) {
            fprintf(f, "%d inflate %u %u\n", inf->device, n_blocks, refused);
            fclose(f);
        }
    }
    return FPL_OK;
}
