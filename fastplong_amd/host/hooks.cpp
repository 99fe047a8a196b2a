/*
 * hooks.cpp -- the C entry points the tests and bench.py reach the host's reader, writer and formatter through.
 */
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <condition_variable>
#include <mutex>

#include "bam.h"
#include "bam_comments.h"
#include "bam_out.h"
#include "bam_tags.h"
#include "../csrc/bam_out_rules.h"
#include "../csrc/bam_tag_rules.h"
#include "../csrc/fq_comment_rules.h"
#include "fastq.h"
#include "fq_comments.h"
#include "gzip.h"
#include "pool.h"

/* test-hook helpers */
namespace {
using fplh::Batch;
using fplh::ChunkedReader;

/* the records of t behind those of all (their names too when asked for) */
void append_batch(Batch& all, const Batch& t, bool names) {
    const size_t o = all.seq.size(), to = all.text.size();
    all.seq.resize_uninit(o + t.seq.size());
    all.qual.resize_uninit(o + t.seq.size());
    memcpy(all.seq.data() + o, t.seq.data(), t.seq.size());
    memcpy(all.qual.data() + o, t.qual.data(), t.seq.size());
    if (names) all.text.insert(all.text.end(), t.text.begin(), t.text.end());
    for (uint32_t i = 0; i < t.n(); i++) {
        all.off.push_back(o + t.off[i + 1]);
        if (!names) continue;
        all.name_off.push_back(to + t.name_off[i + 1]);
        all.name_len.push_back(t.name_len[i]);
        all.strand_len.push_back(t.strand_len[i]);
    }
}

/* s as a malloc'ed buffer the caller frees with fplh_free */
void hand_out(const std::string& s, char** out, uint64_t* len) {
    *out = (char*)malloc(s.size() + 1);
    memcpy(*out, s.data(), s.size());
    *len = s.size();
}

/* The file through a ChunkedReader that draws on a small pool of batches, as the CLI's Work objects are; every batch it hands
   out goes to `each`.  FPLH_CHUNK_MEM (test hook): the parsers take the file's bytes from a mapping, as they take inflated gzip
   members.  false: the file could not be opened. */
bool read_chunked(const char* path, uint64_t chunk_bytes, int threads, bool as_text, uint64_t* chunks_parsed_again,
                  const std::function<void(const Batch&, const fplh::MappedFile&)>& each) {
    const fplh::MappedFile file(path, 1, getenv("FPLH_CHUNK_MEM") != nullptr);
    if (file.fd < 0) return false;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Batch> owned((size_t)threads + 2);
    std::vector<Batch*> pool;
    for (Batch& b : owned) pool.push_back(&b);
    auto acquire = [&]() {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return !pool.empty(); });
        ChunkedReader::Item it;
        it.batch = pool.back();
        pool.pop_back();
        return it;
    };
    auto release = [&](ChunkedReader::Item it) {
        {
            std::lock_guard<std::mutex> g(mu);
            pool.push_back(it.batch);
        }
        cv.notify_all();
    };
    const char* mem = (const char*)file.data;
    ChunkedReader cr(mem ? -1 : file.fd, file.size, chunk_bytes, threads, acquire, release, mem, as_text);
    ChunkedReader::Item it;
    while (cr.next(it)) {
        each(*it.batch, file);
        release(it);
    }
    if (chunks_parsed_again) *chunks_parsed_again = cr.chunks_parsed_again();
    return true;
}

int format_hook(void* bv, const fpl_read_result* res, const fplh::FragmentList* fl, int threads, char** out, uint64_t* out_len, char** failed,
                uint64_t* failed_len) {
    std::vector<std::string> o, f;
    fplh::format_batch_parallel(*(Batch*)bv, res, threads, o, failed ? &f : nullptr, fl);
    std::string oo, ff;
    for (auto& x : o) oo += x;
    for (auto& x : f) ff += x;
    hand_out(oo, out, out_len);
    if (failed) hand_out(ff, failed, failed_len);
    return 0;
}
/* the host form as the CLI runs it: the BAM file at `path` read into ONE batch (BamReader), its decoded bases and qualities and
   its results (and, with n_frags != ~0u, the fragment list of a --break / --mask run) given by the caller; formatted in `threads`
   pieces, the sources derived (bam_tag_sources), the pieces converted (pieces_to_bam_records).  out / failed: the uncompressed
   records of --out / --failed_out; stats: four counts each.  -1: the file did not read to its end as one batch of n reads.
   mods: --keep_mods, with its four counts each in mod_stats; moves: --keep_moves, the same in move_stats */
int bam_tag_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n, const fpl_fragment* frags,
                 uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, char** out, uint64_t* out_len, char** failed,
                 uint64_t* failed_len, uint64_t* stats, bool mods, uint64_t* mod_stats, bool moves = false, uint64_t* move_stats = nullptr) {
    fplh::BamReader rd(path);
    if (!rd.ok()) return -1;
    Batch b;
    if (rd.fill(b, ~0ull, 0x3FFFFFFFu) != n || !rd.error().empty() || b.n() != n) return -1;
    if (b.seq.size()) {
        memcpy(b.seq.data(), seq, b.seq.size());
        memcpy(b.qual.data(), qual, b.seq.size());
    }
    fplh::FragmentList fl;
    const bool fragments = n_frags != ~0u;
    if (fragments) {
        fl.frags.assign(frags, frags + n_frags);
        fl.regs.assign(regs, regs + n_regs);
        fl.index(n);
    }
    std::vector<std::string> o, f;
    fplh::format_batch_parallel(b, res, threads, o, &f, fragments ? &fl : nullptr);
    std::vector<fplh::BamTagSrc> so, sf;
    fplh::bam_tag_sources(b, res, 0, n, fragments ? &fl : nullptr, false, so, mods, moves);
    fplh::bam_tag_sources(b, res, 0, n, fragments ? &fl : nullptr, true, sf, mods, moves);
    for (int k = 0; k < 8; k++) stats[k] = 0;
    if (mod_stats)
        for (int k = 0; k < 8; k++) mod_stats[k] = 0;
    if (move_stats)
        for (int k = 0; k < 8; k++) move_stats[k] = 0;
    fplh::pieces_to_bam_records(o, so, stats, mod_stats, move_stats);
    fplh::pieces_to_bam_records(f, sf, stats + 4, mod_stats ? mod_stats + 4 : nullptr, move_stats ? move_stats + 4 : nullptr);
    std::string oo, ff;
    for (auto& x : o) oo += x;
    for (auto& x : f) ff += x;
    hand_out(oo, out, out_len);
    hand_out(ff, failed, failed_len);
    return 0;
}
/* --comment_tags as the CLI runs it on the host: the same batch, formatted in `threads` pieces, the sources derived with mods on,
   the comments added (pieces_add_tag_comments).  out / failed: the text of --out / --failed_out; stats: four counts each.  -1: as
   above, -2: the selection is not one (fpl::bamcomment::make_selection) */
int bam_comment_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n, const fpl_fragment* frags,
                     uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, const char* tags, int n_tags, char** out,
                     uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats) {
    fplh::BamCommentSelection sel;
    if (!fpl::bamcomment::make_selection(tags, n_tags, sel)) return -2;
    fplh::BamReader rd(path);
    if (!rd.ok()) return -1;
    Batch b;
    if (rd.fill(b, ~0ull, 0x3FFFFFFFu) != n || !rd.error().empty() || b.n() != n) return -1;
    if (b.seq.size()) {
        memcpy(b.seq.data(), seq, b.seq.size());
        memcpy(b.qual.data(), qual, b.seq.size());
    }
    fplh::FragmentList fl;
    const bool fragments = n_frags != ~0u;
    if (fragments) {
        fl.frags.assign(frags, frags + n_frags);
        fl.regs.assign(regs, regs + n_regs);
        fl.index(n);
    }
    std::vector<std::string> o, f;
    fplh::format_batch_parallel(b, res, threads, o, &f, fragments ? &fl : nullptr);
    std::vector<fplh::BamTagSrc> so, sf;
    fplh::bam_tag_sources(b, res, 0, n, fragments ? &fl : nullptr, false, so, true);
    fplh::bam_tag_sources(b, res, 0, n, fragments ? &fl : nullptr, true, sf, true);
    for (int k = 0; k < 8; k++) stats[k] = 0;
    fplh::pieces_add_tag_comments(o, so, sel, stats);
    fplh::pieces_add_tag_comments(f, sf, sel, stats + 4);
    std::string oo, ff;
    for (auto& x : o) oo += x;
    for (auto& x : f) ff += x;
    hand_out(oo, out, out_len);
    hand_out(ff, failed, failed_len);
    return 0;
}
}  // namespace

extern "C" {
/* parse a FASTQ file into CSR arrays (one fill() of the given caps) */
void* fplh_batch_read(const char* path, uint64_t max_bases, uint32_t max_reads) {
    fplh::FastqReader rd(path);
    if (!rd.ok()) return nullptr;
    fplh::Batch* b = new fplh::Batch();
    rd.fill(*b, max_bases, max_reads);
    return b;
}
/* test hook: the whole file through repeated fill() calls of the given caps, concatenated */
void* fplh_batch_read_all(const char* path, uint64_t max_bases, uint32_t max_reads) {
    fplh::FastqReader rd(path);
    if (!rd.ok()) return nullptr;
    fplh::Batch* all = new fplh::Batch();
    all->start_offsets();
    for (;;) {
        fplh::Batch t;
        if (rd.fill(t, max_bases, max_reads) == 0) break;
        append_batch(*all, t, false);
    }
    return all;
}
/* the whole (regular, uncompressed) file through the chunk-parallel reader, concatenated */
void* fplh_batch_read_chunked(const char* path, uint64_t chunk_bytes, int threads, uint64_t* chunks_parsed_again) {
    fplh::Batch* all = new fplh::Batch();
    all->start_offsets();
    if (!read_chunked(path, chunk_bytes, threads, false, chunks_parsed_again, [&](const Batch& t, const fplh::MappedFile&) { append_batch(*all, t, true); })) {
        delete all;
        return nullptr;
    }
    return all;
}
/* test hook: the whole (regular, uncompressed) file through the chunk LOADER (text-backed batches, ChunkedReader as_text): the file
   offsets [begin, end) of every chunk's records, in input order, into ranges[2 k], ranges[2 k + 1]; returns the number of chunks
   that hold records (-1: the file could not be read; more than `cap` chunks: only the first `cap` are stored) */
int64_t fplh_text_chunk_ranges(const char* path, uint64_t chunk_bytes, int threads, uint64_t* ranges, uint64_t cap) {
    int64_t n = 0;
    uint64_t at = 0; /* (file offset of a chunk's text: where the one in front of it ended -- checked by the caller) */
    const bool read = read_chunked(path, chunk_bytes, threads, true, nullptr, [&](const Batch& t, const fplh::MappedFile& file) {
        /* the loader keeps the window's bytes [w0, w1): raw_begin counts from w0, which the batch does not say; the text
           itself does -- compare it with the file at the running offset (the ranges must be contiguous for a regular file) */
        uint64_t found = ~0ull;
        if (t.raw_len > 0) {
            std::vector<char> buf(t.raw_len);
            /* chunks follow one another: try the running offset first, then look ahead (junk lines between records) */
            for (uint64_t o = at; o + t.raw_len <= (uint64_t)file.size && found == ~0ull; o++) {
                if (pread(file.fd, buf.data(), t.raw_len, (off_t)o) != (ssize_t)t.raw_len) break;
                if (memcmp(buf.data(), t.raw.data() + t.raw_begin, t.raw_len) == 0) found = o;
                if (o - at > (1u << 16)) break;
            }
        }
        if ((uint64_t)n < cap) {
            ranges[2 * n] = found;
            ranges[2 * n + 1] = found == ~0ull ? ~0ull : found + t.raw_len;
        }
        if (found != ~0ull) at = found + t.raw_len;
        n++;
    });
    return read ? n : -1;
}
/* bench / test helper: a CSR batch as a FASTQ file ("@<prefix><i>" names, "+" strand lines); the text is composed on
   `threads` threads, slice by slice, and written in order.  0 on success. */
/* append != 0: the records go behind what the file holds (bench.py builds its N-GPU input out of N copies of a batch, each
   with a prefix of its own) */
int fplh_write_fastq_ex(const char* path, const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint32_t n,
                        const char* prefix, int threads, int append) {
    FILE* f = fopen(path, append ? "ab" : "wb");
    if (!f) return -1;
    if (threads < 1) threads = 1;
    const std::string pre = prefix ? prefix : "r";
    const uint32_t per_round = 65536u * (uint32_t)threads; /* bounds the text held in memory */
    int rc = 0;
    for (uint32_t r0 = 0; r0 < n && rc == 0; r0 += per_round) {
        const uint32_t r1 = (uint32_t)std::min<uint64_t>(n, (uint64_t)r0 + per_round);
        std::vector<std::string> parts((size_t)threads);
        fplh::parallel_run(threads, [&](int t) {
            const uint32_t a = r0 + (uint32_t)((uint64_t)(r1 - r0) * t / threads), b = r0 + (uint32_t)((uint64_t)(r1 - r0) * (t + 1) / threads);
            std::string& s = parts[t];
            s.reserve((size_t)(2 * (off[b] - off[a]) + (uint64_t)(b - a) * (pre.size() + 20)));
            for (uint32_t i = a; i < b; i++) {
                s += '@';
                s += pre;
                s += std::to_string(i);
                s += '\n';
                s.append((const char*)seq + off[i], (size_t)(off[i + 1] - off[i]));
                s += "\n+\n";
                s.append((const char*)qual + off[i], (size_t)(off[i + 1] - off[i]));
                s += '\n';
            }
        });
        for (auto& s : parts)
            if (!s.empty() && fwrite(s.data(), 1, s.size(), f) != s.size()) rc = -2;
    }
    if (fclose(f) != 0) rc = -2;
    return rc;
}
int fplh_write_fastq(const char* path, const uint8_t* seq, const uint8_t* qual, const uint64_t* off, uint32_t n,
                     const char* prefix, int threads) {
    return fplh_write_fastq_ex(path, seq, qual, off, n, prefix, threads, 0);
}
/* test hook: read the whole file; 1 (and the message) when the input could not be read / decompressed to its end */
int fplh_read_error(const char* path, char* msg, int msg_len) {
    fplh::FastqReader rd(path);
    if (!rd.ok()) return -1;
    for (;;) {
        fplh::Batch t;
        if (rd.fill(t, 64u << 20, 0x3FFFFFFFu) == 0) break;
    }
    if (!rd.input_error()) return 0;
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", rd.input_error_text().c_str());
    return 1;
}
/* gzip members inflated on the worker pool since the last call */
uint64_t fplh_gz_members(void) { return fplh::GzMembers::delivered.exchange(0); }
/* the inflated text of a gzip file in anonymous memory (fplh::gunzip_members_to_memory), given back with fplh_gunzip_release */
char* fplh_gunzip_to_memory(const char* path, int threads, uint64_t max_bytes, uint64_t* size_out, uint64_t* reserved) {
    return fplh::gunzip_members_to_memory(path, threads, max_bytes, size_out, reserved);
}
/* test hook: fplh::bgzf_into -> a malloc'ed buffer the caller frees with fplh_free (NULL and 0 for empty input) */
int fplh_bgzf_into(const char* in, uint64_t n, int level, char** out, uint64_t* out_len) {
    std::string s(in ? in : "", (size_t)n), o;
    fplh::bgzf_into(s, level, o);
    *out_len = o.size();
    *out = o.empty() ? nullptr : (char*)malloc(o.size());
    if (*out) memcpy(*out, o.data(), o.size());
    return 0;
}
/* test hooks: fplh::fastq_to_bam_records and fplh::bam_header_bytes -> malloc'ed buffers (fplh_free) */
int fplh_fastq_to_bam_records(const char* in, uint64_t n, char** out, uint64_t* out_len) {
    std::string s(in ? in : "", (size_t)n), o;
    fplh::fastq_to_bam_records(s, o);
    *out_len = o.size();
    *out = (char*)malloc(o.size() + 1);
    if (*out) memcpy(*out, o.data(), o.size());
    return *out ? 0 : -1;
}
void fplh_bam_base_table(uint8_t* t) { fpl::bamout::base_table(t); }
int fplh_bam_header_bytes(char** out, uint64_t* out_len) {
    const std::string& h = fplh::bam_header_bytes();
    *out_len = h.size();
    *out = (char*)malloc(h.size());
    if (*out) memcpy(*out, h.data(), h.size());
    return *out ? 0 : -1;
}
/* test hooks of --keep_tags.  _header_rg: the file header with the @RG lines of an input header's text (mode 0) or with `text`
   itself as the lines (mode 1); _walk: the shared rule's walk of a region (prefix, kept, positional, whole); _region: where the
   region of the record at rec lies */
int fplh_bam_header_rg(const char* text, uint64_t n, int mode, char** out, uint64_t* out_len) {
    const std::string t(text ? text : "", (size_t)n);
    hand_out(fplh::bam_header_bytes(mode ? t : fplh::bam_read_group_lines(t)), out, out_len);
    return 0;
}
void fplh_bam_tag_walk(const uint8_t* p, uint64_t len, uint64_t* out) {
    const fpl::bamtag::Walk w = fpl::bamtag::walk(p, len, fpl::bamtag::ByteScan());
    out[0] = w.prefix, out[1] = w.kept, out[2] = w.positional, out[3] = w.whole;
}
void fplh_bam_tag_region(const uint8_t* rec, uint64_t* at, uint64_t* len) { fpl::bamtag::region(rec, *at, *len); }
/* the host form as the CLI runs it (bam_tag_form above); _mod_form: with --keep_mods, and its four counts each in mod_stats */
int fplh_bam_tag_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n,
                      const fpl_fragment* frags, uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, char** out,
                      uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats) {
    return bam_tag_form(path, seq, qual, res, n, frags, n_frags, regs, n_regs, threads, out, out_len, failed, failed_len, stats, false, nullptr);
}
int fplh_bam_mod_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n,
                      const fpl_fragment* frags, uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, char** out,
                      uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats, uint64_t* mod_stats) {
    return bam_tag_form(path, seq, qual, res, n, frags, n_frags, regs, n_regs, threads, out, out_len, failed, failed_len, stats, true, mod_stats);
}
/* _move_form: with --keep_moves, and with --keep_mods beside it where mods != 0; four counts each in mod_stats and move_stats */
int fplh_bam_move_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n,
                       const fpl_fragment* frags, uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, char** out,
                       uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats, int mods, uint64_t* mod_stats, int moves,
                       uint64_t* move_stats) {
    return bam_tag_form(path, seq, qual, res, n, frags, n_frags, regs, n_regs, threads, out, out_len, failed, failed_len, stats, mods != 0, mod_stats,
                        moves != 0, move_stats);
}
/* test hooks of --comment_tags.  _form: the host form as the CLI runs it (bam_comment_form above; tags: 2 * n_tags bytes, n_tags -1:
   every field); _text: the rule's text of the tag bytes p[0, len) under a selection, and its three counts (fields, bytes, left
   out); _list: the CLI's reading of a LIST -> its number of tags (-1: every field), -2: malformed */
int fplh_bam_comment_form(const char* path, const uint8_t* seq, const uint8_t* qual, const fpl_read_result* res, uint32_t n,
                          const fpl_fragment* frags, uint32_t n_frags, const fpl_region* regs, uint32_t n_regs, int threads, const char* tags,
                          int n_tags, char** out, uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats) {
    return bam_comment_form(path, seq, qual, res, n, frags, n_frags, regs, n_regs, threads, tags, n_tags, out, out_len, failed, failed_len, stats);
}
int fplh_bam_comment_text(const uint8_t* p, uint64_t len, const char* tags, int n_tags, char** out, uint64_t* out_len, uint64_t* counts) {
    fplh::BamCommentSelection sel;
    if (!fpl::bamcomment::make_selection(tags, n_tags, sel)) return -2;
    struct Sink {
        std::string s;
        void put(const char* q, uint32_t n) { s.append(q, n); }
        void copy(const uint8_t* q, uint64_t n) { s.append((const char*)q, (size_t)n); }
        uint64_t size() const { return s.size(); }
    } sink;
    const fpl::bamcomment::Counts c = fpl::bamcomment::comment_text(p, len, sel, fpl::bamtag::ByteScan(), sink);
    counts[0] = c.fields, counts[1] = c.bytes, counts[2] = c.left_out;
    hand_out(sink.s, out, out_len);
    return 0;
}
int fplh_comment_tag_list(const char* list) {
    fplh::BamCommentSelection sel;
    return fplh::parse_comment_tags(list ? list : "", sel) ? sel.n : -2;
}
/* test hooks of --reindex_comments.  _form: the host form as the CLI runs it on a batch read from FASTQ text (fplh_batch_read): formatted
   in `threads` pieces, the sources derived (fq_comment_sources), the name lines rewritten (pieces_reindex_comments); n_frags != ~0u: the
   fragment list of a --break / --mask run.  out / failed: the text of --out / --failed_out; stats: five counts each.  _line: the
   rule's line for one output read (fpl::fqcomment::line_text) and its five counts */
int fplh_fq_comment_form(void* bv, const fpl_read_result* res, const fpl_fragment* frags, uint32_t n_frags, const fpl_region* regs, uint32_t n_regs,
                         int threads, char** out, uint64_t* out_len, char** failed, uint64_t* failed_len, uint64_t* stats) {
    const Batch& b = *(Batch*)bv;
    fplh::FragmentList fl;
    const bool fragments = n_frags != ~0u;
    if (fragments) {
        fl.frags.assign(frags, frags + n_frags);
        fl.regs.assign(regs, regs + n_regs);
        fl.index(b.n());
    }
    std::vector<std::string> o, f;
    fplh::format_batch_parallel(b, res, threads, o, &f, fragments ? &fl : nullptr);
    std::vector<fplh::FqCommentSrc> so, sf;
    fplh::fq_comment_sources(b, res, 0, b.n(), fragments ? &fl : nullptr, false, so);
    fplh::fq_comment_sources(b, res, 0, b.n(), fragments ? &fl : nullptr, true, sf);
    for (int k = 0; k < 10; k++) stats[k] = 0;
    fplh::pieces_reindex_comments(o, so, stats);
    fplh::pieces_reindex_comments(f, sf, stats + 5);
    std::string oo, ff;
    for (auto& x : o) oo += x;
    for (auto& x : f) ff += x;
    hand_out(oo, out, out_len);
    hand_out(ff, failed, failed_len);
    return 0;
}
int fplh_fq_comment_line(const uint8_t* fmt, uint64_t fmt_len, const uint8_t* line, uint64_t len, const uint8_t* bases, uint64_t l_seq, uint64_t s,
                         uint64_t n, int changed, int failed, int fragment_mode, char** out, uint64_t* out_len, uint64_t* counts) {
    struct Sink {
        std::string s;
        void put(const char* q, uint32_t k) { s.append(q, k); }
        void copy(const uint8_t* q, uint64_t k) { s.append((const char*)q, (size_t)k); }
    } sink;
    fpl::fqcomment::Counts c = {0, 0, 0, 0, 0};
    fpl::fqcomment::line_text(fmt, fmt_len, line, len, bases, l_seq, s, n, changed != 0, failed != 0, fragment_mode != 0, sink, c);
    counts[0] = c.reindexed, counts[1] = c.lost, counts[2] = c.kept, counts[3] = c.cut, counts[4] = c.left;
    hand_out(sink.s, out, out_len);
    return 0;
}
int fplh_have_libdeflate(void) { return fplh::have_libdeflate() ? 1 : 0; }
/* the single-member lane's inflater (fplh::set_gzip_inflater) and its counts */
void fplh_set_gzip_inflater(fplh::GzipInflateFn fn, void* user, uint64_t window_bytes) { fplh::set_gzip_inflater(fn, user, window_bytes); }
void fplh_gzip_inflater_counts(uint64_t* windows, uint64_t* refused) { fplh::gzip_inflater_counts(windows, refused); }
void fplh_gunzip_release(char* base, uint64_t reserved) {
    if (base) munmap(base, (size_t)reserved);
}
uint32_t fplh_batch_n(void* b) { return ((fplh::Batch*)b)->n(); }
uint64_t fplh_batch_bytes(void* b) { return ((fplh::Batch*)b)->seq.size(); }
const uint8_t* fplh_batch_seq(void* b) { return ((fplh::Batch*)b)->seq.data(); }
const uint8_t* fplh_batch_qual(void* b) { return ((fplh::Batch*)b)->qual.data(); }
const uint64_t* fplh_batch_off(void* b) { return ((fplh::Batch*)b)->off.data(); }
void fplh_batch_free(void* b) { delete (fplh::Batch*)b; }
/* format a batch from result records: malloc'ed buffers the caller frees with fplh_free; _fragments: with a --break / --mask
   fragment list (n_frags records sorted by read / seq_no, their regions) */
int fplh_format_batch(void* bv, const fpl_read_result* res, char** out, uint64_t* out_len, char** failed,
                      uint64_t* failed_len) {
    return format_hook(bv, res, nullptr, 1, out, out_len, failed, failed_len); /* (one slice: format_batch's text) */
}
int fplh_format_batch_fragments(void* bv, const fpl_read_result* res, const fpl_fragment* frags, uint32_t n_frags,
                                const fpl_region* regs, uint32_t n_regs, int threads, char** out, uint64_t* out_len,
                                char** failed, uint64_t* failed_len) {
    fplh::FragmentList fl;
    fl.frags.assign(frags, frags + n_frags);
    fl.regs.assign(regs, regs + n_regs);
    fl.index(((fplh::Batch*)bv)->n());
    return format_hook(bv, res, &fl, threads, out, out_len, failed, failed_len);
}
int fplh_format_batch_parallel(void* bv, const fpl_read_result* res, int threads, char** out, uint64_t* out_len,
                               char** failed, uint64_t* failed_len) {
    return format_hook(bv, res, nullptr, threads, out, out_len, failed, failed_len);
}
void fplh_free(void* p) { free(p); }
}
