/*
 * driver.cpp -- TEST INFRASTRUCTURE ONLY (tests/emu_gzip/emu_gzip_run; tests/emu_gzip/build.py).
 *
 * The kernels of fastplong_amd/csrc/gzip_inflate.h compiled for the host on the lock-step emulator of tests/emu/hip_emu.h.
 * emu_gzip_inflate is fpl_inflate_gzip without the device: the same argument checks (gzip_plan), the same launches
 * (gzip_enqueue).  Every buffer is a heap block of exactly the size the kernels are promised, so under AddressSanitizer a read
 * outside the payload or a store outside a chunk's room, a window or out ends the program with a report.
 * With EMU_GZIP_MAIN the file is that program: jobs in, results out (build.py says how).
 */
#define FPL_EMU 1
#include "../../fastplong_amd/csrc/gzip_inflate.h"

#include <vector>

using namespace fpl;

extern "C" int emu_gzip_inflate(const uint8_t* comp, uint64_t comp_bytes, uint64_t start_bit, const uint8_t* dict, uint32_t dict_len,
                                uint8_t* out, uint64_t out_cap, uint32_t chunk_bytes, fpl_gzip_window* res) {
    GzipJob job;
    if (!res || !comp || (dict_len && !dict) || (out_cap && !out) || !gzip_plan(job, comp_bytes, start_bit, dict_len, out_cap, chunk_bytes))
        return -1;
    const size_t room = (size_t)job.n_chunks * job.room_per_chunk + job.room0_extra;
    const size_t out_room = (size_t)std::min<uint64_t>(out_cap, room);
    u8* d_comp = (u8*)malloc(job.comp_len);
    memcpy(d_comp, comp + (start_bit >> 3), job.comp_len);
    GzipChunk* chunks = (GzipChunk*)malloc(sizeof(GzipChunk) * job.n_chunks);
    memset(chunks, 0xA5, sizeof(GzipChunk) * job.n_chunks); /* (nothing may rely on an initial value) */
    unsigned short* d_room = (unsigned short*)malloc(2 * room);
    memset(d_room, 0xA5, 2 * room);
    u8* wins = (u8*)malloc(((size_t)job.n_chunks + 1) * GZIP_WINDOW);
    memset(wins, 0, GZIP_WINDOW);
    if (dict_len) memcpy(wins + (GZIP_WINDOW - dict_len), dict, dict_len);
    u8* d_out = (u8*)malloc(out_room ? out_room : 1);
    fpl_gzip_window r;
    memset(&r, 0xA5, sizeof(r));
    job.comp = d_comp, job.chunks = chunks, job.room = d_room, job.wins = wins, job.out = d_out, job.res = &r, job.out_cap = out_room;
    gzip_enqueue(job, 2, nullptr);
    int rc = 0;
    if (r.status == FPL_GZIP_OK) {
        if (r.out_bytes > out_room)
            rc = -2;
        else if (r.out_bytes)
            memcpy(out, d_out, r.out_bytes);
    }
    r.end_bit += 8 * (start_bit >> 3);
    *res = r;
    free(d_comp), free(chunks), free(d_room), free(wins), free(d_out);
    return rc;
}

#ifdef EMU_GZIP_MAIN
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    FILE* g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    uint64_t n_jobs;
    if (fread(&n_jobs, 8, 1, f) != 1) return 2;
    for (uint64_t j = 0; j < n_jobs; j++) {
        uint64_t h[5]; /* comp_bytes, start_bit, dict_len, out_cap, chunk_bytes */
        if (fread(h, 8, 5, f) != 5) return 2;
        uint8_t* comp = (uint8_t*)malloc(h[0] ? h[0] : 1);
        uint8_t* dict = (uint8_t*)malloc(h[2] ? h[2] : 1);
        uint8_t* out = (uint8_t*)malloc(h[3] ? h[3] : 1);
        if (h[0] && fread(comp, 1, h[0], f) != h[0]) return 2;
        if (h[2] && fread(dict, 1, h[2], f) != h[2]) return 2;
        fpl_gzip_window r;
        memset(&r, 0, sizeof(r));
        const int64_t rc = emu_gzip_inflate(h[0] ? comp : nullptr, h[0], h[1], h[2] ? dict : nullptr, (uint32_t)h[2], h[3] ? out : nullptr, h[3],
                                            (uint32_t)h[4], &r);
        if (rc == -2) return 3; /* more bytes than out_cap: must not happen */
        fwrite(&rc, 8, 1, g);
        fwrite(&r, sizeof(r), 1, g);
        if (rc == 0 && r.status == FPL_GZIP_OK && r.out_bytes) fwrite(out, 1, r.out_bytes, g);
        free(comp), free(dict), free(out);
    }
    fclose(f);
    fclose(g);
    return 0;
}
#endif
