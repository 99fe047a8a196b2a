/*
 * gzip_stand_in.h -- TEST INFRASTRUCTURE ONLY (tests/stub_gz, tests/stub_bgzfout, tests/stub_bamout): the gzip entry points of
 * ABI v9 on the CPU, for a translation unit that has included ../stub/fpl_stub.cpp (its queue must be seen).  Independent of the
 * device coder, of the host's bgzf_into and of the host's fastq_to_bam_records: the batch's output is composed with the host's
 * formatter (fplh::format_batch over the text and the records) and deflated with zlib.  The including file chooses what the
 * library has beyond fpl_set_text_gzip, fpl_get_gzip_batches and fpl_wait_text_gz, which make one gzip member per batch:
 *   STAND_IN_FRAMING  fpl_set_gzip_framing: with FPL_GZIP_BGZF, BGZF blocks of 49 152 bytes each (the device's stripe, so a test
 *                     tells the stand-in's blocks from the host's 65 280-byte ones by their ISIZE)
 *   STAND_IN_RECORDS  fpl_set_gzip_records: with FPL_GZIP_BAM the text is turned into BAM records by the few lines of to_records()
 *                     before it is framed
 * The CLI finds these two calls by name, and tests rely on libraries that lack them: a library exports only what its file defines.
 * FPL_STUB_GZ_LOG=<file>: one line per batch made ("<device> <gz|bgzf|bam> <bytes deflated> <bytes> <blocks>", blocks 0 for a
 * plain member).
 */
#ifndef FPL_GZIP_STAND_IN_H
#define FPL_GZIP_STAND_IN_H
#include <ctype.h>
#include <zlib.h>

#include <algorithm>
#include <map>

#include "../../fastplong_amd/host/fastq.h"

namespace {
std::mutex g_gz_m;
std::map<fpl_ctx*, bool> g_on;                                  /* fpl_set_text_gzip */
std::map<fpl_ctx*, bool> g_bgzf;                                /* fpl_set_gzip_framing */
std::map<fpl_ctx*, bool> g_bam;                                 /* fpl_set_gzip_records */
std::map<fpl_ctx*, std::string> g_bytes[FPL_MAX_IN_FLIGHT + 1]; /* what fpl_wait_text_gz hands out stays valid as long as the records */
std::map<fpl_ctx*, unsigned> g_no;
std::map<fpl_ctx*, uint64_t> g_made;

/* zlib level 1 over [p, p + n): window_bits 15 + 16 a gzip member, -15 a raw stream */
bool zdeflate(const char* p, size_t n, int window_bits, std::string& out) {
    out.assign(compressBound(n) + 64, '\0');
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 1, Z_DEFLATED, window_bits, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    z.next_in = (Bytef*)p;
    z.avail_in = (uInt)n;
    z.next_out = (Bytef*)&out[0];
    z.avail_out = (uInt)out.size();
    const int zr = deflate(&z, Z_FINISH);
    out.resize(z.total_out);
    deflateEnd(&z);
    return zr == Z_STREAM_END;
}

/* o as BGZF blocks of 49 152 bytes, appended to bytes */
bool bgzf_frame(const std::string& o, std::string& bytes, unsigned long long& blocks) {
    const size_t S = 49152;
    for (size_t at = 0; at < o.size(); at += S, blocks++) {
        const size_t n = std::min(S, o.size() - at);
        std::string raw;
        if (!zdeflate(o.data() + at, n, -15, raw) || raw.size() + 26 > 65536) return false;
        const size_t bsize = raw.size() + 26 - 1;
        const unsigned char head[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (unsigned char)(bsize & 0xFF),
                                        (unsigned char)(bsize >> 8)};
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)o.data() + at, (uInt)n);
        unsigned char tail[8];
        for (int k = 0; k < 4; k++) tail[k] = (unsigned char)(crc >> (8 * k)), tail[4 + k] = (unsigned char)((uint32_t)n >> (8 * k));
        bytes.append((const char*)head, 18);
        bytes += raw;
        bytes.append((const char*)tail, 8);
    }
    return true;
}

#ifdef STAND_IN_RECORDS
/* formatted FASTQ text -> the records of README "BAM output", written from the rule's text and from nothing else */
std::string to_records(const std::string& fq) {
    std::string out;
    size_t at = 0;
    auto line = [&]() {
        const size_t e = fq.find('\n', at);
        std::string l = fq.substr(at, e == std::string::npos ? std::string::npos : e - at);
        at = e == std::string::npos ? fq.size() : e + 1;
        return l;
    };
    auto le32 = [&](uint32_t v) {
        for (int k = 0; k < 4; k++) out += (char)(v >> (8 * k));
    };
    const std::string letters = "=ACMGRSVTWYHKDBN";
    while (at < fq.size()) {
        std::string name = line(), seq = line();
        line();
        std::string qual = line();
        name = name.empty() ? name : name.substr(1);
        name = name.substr(0, std::min(name.find_first_of(" \t"), (size_t)254));
        if (name.empty()) name = "*";
        const uint32_t n = (uint32_t)seq.size();
        le32(32 + (uint32_t)name.size() + 1 + (n + 1) / 2 + n);
        le32(0xFFFFFFFFu), le32(0xFFFFFFFFu);
        le32(((uint32_t)name.size() + 1) | (4680u << 16));
        le32(4u << 16);
        le32(n);
        le32(0xFFFFFFFFu), le32(0xFFFFFFFFu), le32(0);
        out += name;
        out += '\0';
        for (uint32_t i = 0; i < n; i += 2) {
            unsigned b = 0;
            for (uint32_t k = i; k < i + 2 && k < n; k++) {
                const size_t c = letters.find((char)toupper((unsigned char)seq[k]));
                b |= (unsigned)(c == std::string::npos || seq[k] == 0 ? 15 : c) << (k == i ? 4 : 0);
            }
            out += (char)b;
        }
        for (uint32_t i = 0; i < n; i++) out += (char)(std::max<int>((unsigned char)qual[i], 33) - 33);
    }
    return out;
}
#endif
}  // namespace

extern "C" int fpl_set_text_gzip(fpl_ctx* ctx, int on) {
    if (!ctx) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_gz_m);
    g_on[ctx] = on != 0;
    return FPL_OK;
}

#ifdef STAND_IN_FRAMING
extern "C" int fpl_set_gzip_framing(fpl_ctx* ctx, int framing) {
    if (!ctx || (framing != FPL_GZIP_MEMBER && framing != FPL_GZIP_BGZF)) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_gz_m);
    g_bgzf[ctx] = framing == FPL_GZIP_BGZF;
    return FPL_OK;
}
#endif

#ifdef STAND_IN_RECORDS
extern "C" int fpl_set_gzip_records(fpl_ctx* ctx, int records) {
    if (!ctx || (records != FPL_GZIP_FASTQ && records != FPL_GZIP_BAM)) return FPL_ERR_ARG;
    std::lock_guard<std::mutex> g(g_gz_m);
    g_bam[ctx] = records == FPL_GZIP_BAM;
    return FPL_OK;
}
#endif

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
    bool on, framed, bam;
    {
        std::lock_guard<std::mutex> g(g_gz_m); /* (a map no setter of this library fills says false) */
        on = g_on[ctx];
        bam = g_bam[ctx];
        framed = g_bgzf[ctx] || bam; /* records are BGZF whatever the framing says */
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
#ifdef STAND_IN_RECORDS
    if (bam) o = to_records(o);
#endif
    std::string bytes;
    unsigned long long blocks = 0;
    if (!(framed ? bgzf_frame(o, bytes, blocks) : zdeflate(o.data(), o.size(), 15 + 16, bytes))) return FPL_ERR_STATE;
    std::lock_guard<std::mutex> g(g_gz_m);
    std::string& keep = g_bytes[g_no[ctx]++ % (FPL_MAX_IN_FLIGHT + 1)][ctx];
    keep.swap(bytes);
    *gz = (const uint8_t*)keep.data();
    *gz_len = keep.size();
    g_made[ctx]++;
    if (const char* lf = getenv("FPL_STUB_GZ_LOG"))
        if (FILE* f = fopen(lf, "a")) {
            fprintf(f, "%d %s %llu %llu %llu\n", ctx->device, bam ? "bam" : framed ? "bgzf" : "gz", (unsigned long long)o.size(),
                    (unsigned long long)keep.size(), blocks);
            fclose(f);
        }
    return FPL_OK;
}
#endif
