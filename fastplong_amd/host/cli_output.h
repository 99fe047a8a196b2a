/*
 * cli_output.h -- the files a run writes its reads to: --out, --failed_out, or --split*'s numbered files.
 * Part of cli.cpp's translation unit.
 */
#ifndef FPLH_CLI_OUTPUT_H
#define FPLH_CLI_OUTPUT_H

#include "bam_comments.h"
#include "bam_out.h"
#include "bam_tags.h"
#include "cli_options.h"
#include "fq_comments.h"
#include "gzip.h"
#include "pool.h"
#include "split.h"

/* Outputs are plain files; a name ending in .gz gets gzip members (-z level), one per formatted slice,
   deflated on the formatter threads and concatenated by the writer: any gzip reader takes that as one stream.
   A name ending in .bam gets unaligned BAM (README "BAM output"): the header's BGZF block, every slice's text turned into
   records (bam_out.h) and framed as BGZF blocks, the EOF block */
struct OutFile {
    FILE* f = nullptr;
    bool gz = false;
    bool bgzf = false; /* --bgzf: the .gz is BGZF blocks, ended by the EOF block */
    bool bam = false;  /* *.bam: BAM records in BGZF blocks (gz and bgzf are set too), the header in front */
    bool wrote = false;
    /* FPLH_PARALLEL_WRITE (measurement hook): the pieces of a batch written side by side at their offsets (pwrite from
       the worker pool; nothing goes through the FILE's buffer then).  Measured on the GPU box into tmpfs: no gain -- one
       thread copies into the page cache at 5.5-6 GB/s, fifteen pwrite()s side by side, or fifteen memcpy()s into a mapped
       window of the file, fill it at the same 5.5-6 GB/s: what bounds a single output file is the kernel's insertion of
       fresh pages into that file's page cache, not the copy.  So the plain path stays the default. */
    bool positional = false;
    uint64_t pos = 0;
    explicit operator bool() const { return f != nullptr; }

    static OutFile open(const string& path, bool bgzf = false) {
        OutFile o;
        if (path.empty()) return o;
        o.bam = ends_with_bam(path);
        o.gz = o.bam || ends_with_gz(path);
        o.bgzf = o.bam || (o.gz && bgzf);
        o.f = fopen(path.c_str(), "wb");
        if (!o.f) error_exit("Failed to write: " + path);
        struct stat st;
        o.positional = getenv("FPLH_PARALLEL_WRITE") && fstat(fileno(o.f), &st) == 0 && S_ISREG(st.st_mode);
        return o;
    }
    /* *.bam: the header's block, before the first piece (a file no read reaches is this block and the EOF block) */
    /* readGroups: --keep_tags, the input's @RG lines (a header past 65 280 bytes takes several blocks, which hold nothing else) */
    void write_bam_header(int gzLevel, const string* readGroups = nullptr) {
        if (!f || !bam) return;
        string h;
        fplh::bgzf_into(readGroups ? fplh::bam_header_bytes(*readGroups) : fplh::bam_header_bytes(), gzLevel, h);
        if (positional ? pwrite(fileno(f), h.data(), h.size(), 0) != (ssize_t)h.size() : fwrite(h.data(), 1, h.size(), f) != h.size())
            error_exit("write failed");
        pos = h.size();
    }
    void write_pieces(const vector<string>& pieces) {
        if (positional) { /* input order by construction: the offsets are the running sum of the pieces' sizes */
            vector<uint64_t> at(pieces.size());
            for (size_t i = 0; i < pieces.size(); i++) {
                at[i] = pos;
                pos += pieces[i].size();
                if (!pieces[i].empty()) wrote = true;
            }
            std::atomic<bool> bad{false};
            const int fd = fileno(f);
            fplh::parallel_run((int)pieces.size(), [&](int i) {
                const char* p = pieces[i].data();
                size_t left = pieces[i].size();
                uint64_t off = at[i];
                while (left > 0) {
                    const ssize_t w = pwrite(fd, p, left, (off_t)off);
                    if (w < 0 && errno == EINTR) continue;
                    if (w <= 0) {
                        bad = true;
                        return;
                    }
                    p += w;
                    off += (uint64_t)w;
                    left -= (size_t)w;
                }
            });
            if (bad) error_exit("write failed");
            return;
        }
        for (auto& piece : pieces)
            if (!piece.empty()) {
                if (fwrite(piece.data(), 1, piece.size(), f) != piece.size()) error_exit("write failed");
                wrote = true;
            }
    }
    void close(int gzLevel) {
        if (!f) return;
        if (bgzf) { /* (a file no read reached is exactly this block) */
            const string& e = fplh::bgzf_eof();
            if (positional ? pwrite(fileno(f), e.data(), e.size(), (off_t)pos) != (ssize_t)e.size() /* (the FILE's own position is still 0) */
                           : fwrite(e.data(), 1, e.size(), f) != e.size())
                error_exit("write failed");
        } else if (gz && !wrote) { /* an empty .gz still has to be a gzip stream */
            const string e = fplh::gzip_member(string(), gzLevel);
            if (fwrite(e.data(), 1, e.size(), f) != e.size()) error_exit("write failed");
        }
        /* the buffered tail goes out here: a full disk shows up as a failing flush / close */
        if (f == stdout ? (fflush(stdout) != 0 || ferror(stdout)) : (fclose(f) != 0)) error_exit("write failed");
    }
};

/* --keep_tags: what the host's converter counted (bam_out.h), over every formatter thread */
static std::atomic<uint64_t> g_bamTagStats[4];
/* --keep_mods: the same for its four counts */
static std::atomic<uint64_t> g_bamModStats[4];
/* --keep_moves: the same */
static std::atomic<uint64_t> g_bamMoveStats[4];
/* --comment_tags: what the host's form counted (bam_comments.h) */
static std::atomic<uint64_t> g_bamCommentStats[4];
/* --reindex_comments: the five counts of the host's form (fq_comments.h) */
static std::atomic<uint64_t> g_fqCommentStats[5];

struct Outputs {
    OutFile fout, ffail;
    bool keepTags = false; /* --keep_tags: a .bam output's records carry their input record's auxiliary fields */
    bool keepMods = false; /* --keep_mods: ... with MM / ML / MN re-indexed where the record is trimmed or split */
    bool keepMoves = false; /* --keep_moves: ... with the move table and ts re-indexed in the same way */
    const fplh::BamCommentSelection* comments = nullptr; /* --comment_tags: the FASTQ outputs' name lines carry the selected fields */
    bool reindexComments = false; /* --reindex_comments: the FASTQ outputs' name lines carry the input's comments, re-indexed */
    int gzLevel = 4;
    bool bgzf = false; /* --bgzf: the pieces are framed by bgzf_into */
    fplh::SplitOutput* split = nullptr; /* --split / --split_by_lines: the workers' private writers take the passing reads */
    bool gatherOut = false;             /* --out is written as gather lists over the batches' own arrays (build_gather) */

    /* --comment_tags: the fields behind the name lines of a batch's formatted pieces, in front of the deflate (src: bam_tag_sources
       with mods on, over all pieces) */
    void comment_pieces(vector<string>& pieces, const vector<fplh::BamTagSrc>& src) const {
        uint64_t st[4] = {0, 0, 0, 0};
        fplh::pieces_add_tag_comments(pieces, src, *comments, st);
        for (int k = 0; k < 4; k++) g_bamCommentStats[k] += st[k];
    }
    /* --reindex_comments: the name lines of a batch's formatted pieces rewritten, in front of the deflate (src: fq_comment_sources,
       over all pieces) */
    void reindex_pieces(vector<string>& pieces, const vector<fplh::FqCommentSrc>& src) const {
        uint64_t st[5] = {0, 0, 0, 0, 0};
        fplh::pieces_reindex_comments(pieces, src, st);
        for (int k = 0; k < 5; k++) g_fqCommentStats[k] += st[k];
    }
    bool any_gz() const { return (fout && fout.gz) || (ffail && ffail.gz); }
    /* the pieces as `file` takes them (in parallel; pieces stay below 4 GiB: one slice of a batch) */
    /* tags: --keep_tags, the sources of the records of ALL pieces together, in their order (bam_tags.h) */
    void gzip_pieces(vector<string>& pieces, const OutFile& file, const vector<fplh::BamTagSrc>* tags = nullptr) const {
        const int level = gzLevel;
        const bool blocks = file.bgzf, records = file.bam;
        if (records && tags) {
            uint64_t st[4] = {0, 0, 0, 0}, ms[4] = {0, 0, 0, 0}, vs[4] = {0, 0, 0, 0};
            fplh::pieces_to_bam_records(pieces, *tags, st, ms, vs);
            for (int k = 0; k < 4; k++) g_bamTagStats[k] += st[k], g_bamModStats[k] += ms[k], g_bamMoveStats[k] += vs[k];
        }
        fplh::parallel_run((int)pieces.size(), [&](int i) {
            if (pieces[i].empty()) return;
            if (records && !tags) {
                string rec;
                fplh::fastq_to_bam_records(pieces[i], rec);
                pieces[i].swap(rec);
            }
            if (blocks) fplh::bgzf_into(pieces[i], level, pieces[i]);
            else fplh::gzip_into(pieces[i], level, pieces[i]);
        });
    }
    void close() {
        fout.close(gzLevel);
        ffail.close(gzLevel);
    }
};

static Outputs open_outputs(const Options& opt, const string& bamReadGroups = string()) {
    Outputs o;
    /* with --split* the reference never calls initOutput (src/seprocessor.cpp:65-67): no single --out file and no
       --failed_out either; the workers' private writers take the passing reads */
    o.bgzf = opt.bgzf;
    o.fout = OutFile::open(opt.splitEnabled ? string() : opt.out, opt.bgzf);
    o.ffail = OutFile::open(opt.splitEnabled ? string() : opt.failedOut, opt.bgzf);
    if (opt.toStdout) o.fout.f = stdout, o.fout.gz = false, o.fout.bgzf = false, o.fout.bam = false, o.fout.positional = false;
    o.gzLevel = min(9, max(1, opt.compression));
    o.keepTags = opt.keepTags;
    o.keepMods = opt.keepMods;
    o.keepMoves = opt.keepMoves;
    o.comments = opt.commentTags ? &opt.commentSel : nullptr;
    o.reindexComments = opt.reindexComments;
    o.fout.write_bam_header(o.gzLevel, opt.keepTags ? &bamReadGroups : nullptr);
    o.ffail.write_bam_header(o.gzLevel, opt.keepTags ? &bamReadGroups : nullptr);
    if (opt.splitEnabled)
        o.split = new fplh::SplitOutput(opt.out, opt.splitDigits, opt.workers, opt.splitByLines, opt.splitNumber, opt.splitSize, o.gzLevel, opt.bgzf);
    /* Plain --out alone that is NOT a regular file -- a pipe into an aligner or a compressor (--stdout, /dev/stdout), /dev/null --
       is written as gather lists over the batches' own arrays (build_gather): nothing is formatted.  Into a regular file the
       one writer thread's copy into the page cache is the bottleneck either way (18 GB: 2.9 s from formatted pieces, 3.6 s
       from eight small entries per read), so files keep the pieces the formatter threads put together side by side.
       FPLH_NO_GATHER / FPLH_GATHER_FILES: measurement hooks */
    /* (--comment_tags, --reindex_comments: the comments go into formatted text) */
    o.gatherOut = o.fout && !o.fout.gz && !o.ffail && !opt.fragmentMode && !o.split && !o.comments && !o.reindexComments && !getenv("FPLH_NO_GATHER");
    if (o.gatherOut && !getenv("FPLH_GATHER_FILES")) {
        struct stat ost;
        if (fstat(fileno(o.fout.f), &ost) == 0 && S_ISREG(ost.st_mode)) o.gatherOut = false;
    }
    if (o.gatherOut) fflush(o.fout.f); /* (from here on the descriptor is written directly) */
    return o;
}

#endif
