/*
 * bamgz_stand_in.cpp -- TEST INFRASTRUCTURE ONLY (tests/stub_bamgz/libfastplong_amd.so, built by tests/stub_bamgz/build.py).
 *
 * The CPU stand-in of tests/stub (fpl_stub.cpp, unchanged: compiled into this translation unit so that its queue can be seen) plus
 * the BAM entry points of ABI v8 and the gzip-BAM entry points of ABI v10.  The decoded bases and the member come from the
 * product's own kernels on the emulator (tests/emu_bamgz/driver.cpp, linked beside this file): k_bam_decode, the BAM forms of
 * k_gz_layout / k_gz_compose and the block kernels, over the per-read records the stand-in's oracle made -- so bin/fastplong_amd's
 * BAM-to-.gz path (the choice of form, NULL arrays, members in order) runs on a box without GPUs.
 * FPL_STUB_BAMGZ_LOG=<file>: "<device> bam <n_reads> seq_out=<0|1> gz=<0|1>" per submission and
 * "<device> gz <text bytes out> <member bytes>" per member made.
 */
#include "../stub/fpl_stub.cpp"

#include <map>
#include <memory>

extern "C" int emu_bamgz_decode(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, uint32_t n_rec, uint8_t* seq, uint8_t* qual);
extern "C" int emu_bamgz_emit(const uint8_t* bam, const uint64_t* rec_start, const uint64_t* off, const fpl_read_result* res, uint32_t n_rec,
                              uint8_t* out, uint64_t out_cap, uint64_t* info, uint8_t* comp_out, uint64_t* blk_out, uint64_t blk_out_cap);
extern "C" uint32_t emu_bamgz_pad(void);

namespace {
struct BamBatch { /* what a gzip batch needs until its wait */
    std::vector<uint8_t> bam, seq, qual; /* the records with the pad behind them; the decoded arrays when the caller gave none */
    const uint64_t *rec_start, *off;
    uint32_t n;
};
std::mutex g_bg_m;
std::mutex g_emu_m; /* the emulator's __shared__ is static storage: one launch at a time, whichever "device" asks */
std::map<fpl_ctx*, bool> g_bam_on;                                      /* fpl_set_bam_gzip */
std::map<const fpl_read_result*, std::unique_ptr<BamBatch>> g_batch;    /* by the batch's record array */
std::map<fpl_ctx*, std::string> g_bam_member[FPL_MAX_IN_FLIGHT + 1];    /* what fpl_wait_bam_gz hands out stays valid as long as the records */
std::map<fpl_ctx*, unsigned> g_bam_no;
std::map<fpl_ctx*, uint64_t> g_bam_made;

void bg_log(const std::string& line) {
    const char* lf = getenv("FPL_STUB_BAMGZ_LOG");
    if (!lf) return;
    std::lock_guard<std::mutex> g(g_log_m);
    if (FILE* f = fopen(lf, "a")) {
        fprintf(f, "%s\n", line.c_str());
        fclose(f);
    }
}
std::vector<uint8_t> padded(const uint8_t* bam, uint64_t n_bytes) {
    std::vector<uint8_t> v((size_t)n_bytes + emu_bamgz_pad(), 0);
    if (n_bytes) memcpy(v.data(), bam, (size_t)n_bytes);
    return v;
}
void decode(const uint8_t* bam_padded, const uint64_t* rec_start, const uint64_t* off, uint32_t n, uint8_t* seq, uint8_t* qual) {
    const uint64_t total = off[n];
    std::vector<uint8_t> s((size_t)((total + 15) / 16 * 16 + 32)), q(s.size()); /* (the kernel writes whole 16-byte words) */
    {
        std::lock_guard<std::mutex> g(g_emu_m);
        emu_bamgz_decode(bam_padded, rec_start, off, n, s.data(), q.data());
    }
    if (total > off[0]) {
        memcpy(seq + off[0], s.data() + off[0], (size_t)(total - off[0]));
        memcpy(qual + off[0], q.data() + off[0], (size_t)(total - off[0]));
    }
}
}  // namespace

extern "C" int fpl_set_bam_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    if (on && (ctx->opt.break_enabled || ctx->opt.mask_enabled)) return FPL_ERR_STATE;
    std::lock_guard<std::mutex> g(g_bg_m);
    g_bam_on[ctx] = on != 0;
    return FPL_OK;
}

extern "C" int fpl_get_gzip_batches(const fpl_ctx* ctx, uint64_t* out) {
    if (!ctx || !out) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_bg_m);
    *out = g_bam_made[(fpl_ctx*)ctx];
    return FPL_OK;
}

extern "C" int fpl_process_bam_async(fpl_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                                     uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out, fpl_read_result* results) {
    if (!ctx) return FPL_ERR_ARG;
    bool on;
    {
        std::lock_guard<std::mutex> g(g_bg_m);
        on = g_bam_on[ctx];
    }
    if (n_reads && (!bam || !rec_start || !off || !results)) return FPL_ERR_ARG;
    if (n_reads && (!seq_out || !qual_out) && !(on && !seq_out && !qual_out)) return FPL_ERR_ARG;
    if (ctx->q.size() >= FPL_MAX_IN_FLIGHT) return FPL_ERR_STATE;
    bg_log(std::to_string(ctx->device) + " bam " + std::to_string(n_reads) + " seq_out=" + (seq_out ? "1" : "0") + " gz=" + (on ? "1" : "0"));
    if (n_reads == 0) return fpl_process_batch_async(ctx, seq_out, qual_out, off, 0, results);
    std::unique_ptr<BamBatch> b(new BamBatch());
    b->bam = padded(bam, n_bytes);
    b->rec_start = rec_start;
    b->off = off;
    b->n = n_reads;
    if (!seq_out) {
        b->seq.resize((size_t)off[n_reads] + 1);
        b->qual.resize((size_t)off[n_reads] + 1);
        seq_out = b->seq.data();
        qual_out = b->qual.data();
    }
    decode(b->bam.data(), rec_start, off, n_reads, seq_out, qual_out);
    const int rc = fpl_process_batch_async(ctx, seq_out, qual_out, off, n_reads, results);
    if (rc == FPL_OK && on) {
        std::lock_guard<std::mutex> g(g_bg_m);
        g_batch[results] = std::move(b);
    }
    return rc;
}

extern "C" int fpl_decode_bam(int32_t device, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                              uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out) {
    (void)device;
    if (n_reads == 0) return FPL_OK;
    const std::vector<uint8_t> p = padded(bam, n_bytes);
    decode(p.data(), rec_start, off, n_reads, seq_out, qual_out);
    return FPL_OK;
}

extern "C" int fpl_wait_bam_gz(fpl_ctx* ctx, const uint8_t** gz, uint64_t* gz_len) {
    if (!ctx || !gz || !gz_len) return FPL_ERR_ARG;
    *gz = nullptr;
    *gz_len = 0;
    if (ctx->q.empty() || ctx->q.front().is_text) return FPL_ERR_STATE;
    const fpl_read_result* res = ctx->q.front().res;
    std::unique_ptr<BamBatch> b;
    {
        std::lock_guard<std::mutex> g(g_bg_m);
        auto it = g_batch.find(res);
        if (it != g_batch.end()) {
            b = std::move(it->second);
            g_batch.erase(it);
        }
    }
    const int rc = fpl_wait(ctx);
    if (rc != FPL_OK || !b) return rc;
    const uint64_t cap = 4 * b->off[b->n] + 600ull * b->n + 4096;
    std::string member((size_t)cap, '\0');
    uint64_t info[4] = {0, 0, 0, 0};
    {
        std::lock_guard<std::mutex> g(g_emu_m);
        if (emu_bamgz_emit(b->bam.data(), b->rec_start, b->off, res, b->n, (uint8_t*)&member[0], cap, info, nullptr, nullptr, 0) != 0)
            return FPL_ERR_STATE;
    }
    if (info[1] == 0) return FPL_OK;
    member.resize((size_t)info[1]);
    std::lock_guard<std::mutex> g(g_bg_m);
    std::string& keep = g_bam_member[g_bam_no[ctx]++ % (FPL_MAX_IN_FLIGHT + 1)][ctx];
    keep.swap(member);
    *gz = (const uint8_t*)keep.data();
    *gz_len = keep.size();
    g_bam_made[ctx]++;
    bg_log(std::to_string(ctx->device) + " gz " + std::to_string(info[0]) + " " + std::to_string(keep.size()));
    return FPL_OK;
}
