/*
 * gz_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_gz/libfastplong_amd.so, built by tests/stub_gz/build.py).
 *
 * The CPU stand-in of tests/stub (fpl_stub.cpp, unchanged: compiled into this translation unit so that its queue can be seen)
 * plus the three gzip entry points of ABI v9.  The stand-in is independent of the device coder: it composes the batch's output
 * with the host's formatter (fplh::format_batch over the text and the records) and deflates it with zlib into one gzip member,
 * so bin/fastplong_amd's device-gzip path -- the choice of form, members in order, host members between them -- runs on a box
 * without GPUs.  FPL_STUB_GZ_LOG=<file>: one line per member made ("<device> gz <text bytes out> <member bytes>").
 */
#include "../stub/fpl_stub.cpp"

#include <zlib.h>

#include <map>

#include "../../fastplong_amd/host/fastq.h"

namespace {
std::mutex g_gz_m;
std::map<fpl_ctx*, bool> g_on;                                   /* fpl_set_text_gzip */
std::map<fpl_ctx*, std::string> g_member[FPL_MAX_IN_FLIGHT + 1]; /* what fpl_wait_text_gz hands out stays valid as long as the records */
std::map<fpl_ctx*, unsigned> g_no;
std::map<fpl_ctx*, uint64_t> g_made;
}  // namespace

extern "C" int fpl_set_text_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_gz_m);
    g_on[ctx] = on != 0;
    return FPL_OK;
}

extern "C" int fpl_get_gzip_batches(const fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_gz_m);
    *out = g_made[(fpl_ctx*)ctx];
    return FPL_OK;
}

extern "C" int fpl_wait_text_gz(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                                const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !out || !gz || !gz_len) return FPL_ERR_ARG;
    *gz = nullptr;
    *gz_len = 0;
    if (ctx->q.empty() || !ctx->q.front().is_text) return FPL_ERR_STATE;
    const uint8_t* text = ctx->q.front().text;
    const uint64_t n_bytes = ctx->q.front().text_bytes;
    const fpl_read_result* rr = nullptr;
    const uint32_t* ls = nullptr;
    const int rc = fpl_wait_text(ctx, out, &rr, &ls);
    if (results) *results = rr;
    if (line_starts) *line_starts = ls;
    bool on;
    {
        std::lock_guard<std::mutex> g(g_gz_m);
        on = g_on[ctx];
    }
    if (rc != FPL_OK || !on || out->status != FPL_TEXT_OK || out->n_reads == 0) return rc;
    fplh::Batch b;
    b.text_backed = true;
    b.raw.resize_uninit(n_bytes);
    memcpy(b.raw.data(), text, n_bytes);
    b.raw_begin = 0;
    b.raw_len = n_bytes;
    b.adopt_lines(ls, out->n_reads);
    std::string o;
    fplh::format_batch(b, rr, o, nullptr);
    if (o.empty()) return FPL_OK;
    std::string member(compressBound(o.size()) + 64, '\0');
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return FPL_ERR_STATE;
    z.next_in = (Bytef*)o.data();
    z.avail_in = (uInt)o.size();
    z.next_out = (Bytef*)&member[0];
    z.avail_out = (uInt)member.size();
    const int zr = deflate(&z, Z_FINISH);
    member.resize(z.total_out);
    deflateEnd(&z);
    if (zr != Z_STREAM_END) return FPL_ERR_STATE;
    std::lock_guard<std::mutex> g(g_gz_m);
    std::string& keep = g_member[g_no[ctx]++ % (FPL_MAX_IN_FLIGHT + 1)][ctx];
    keep.swap(member);
    *gz = (const uint8_t*)keep.data();
    *gz_len = keep.size();
    g_made[ctx]++;
    if (const char* lf = getenv("FPL_STUB_GZ_LOG"))
        if (FILE* f = fopen(lf, "a")) {
            fprintf(f, "%d gz %llu %llu\n", ctx->device, (unsigned long long)o.size(), (unsigned long long)keep.size());
            fclose(f);
        }
    return FPL_OK;
}
