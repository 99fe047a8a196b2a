/*
 * fastq.h -- the host keeps the FASTQ reader/writer role of the reference
 * (src/fastqreader.cpp:219-347, src/writer.cpp, Read::appendToString* src/read.cpp:119-173) but
 * re-shaped for the device: records are parsed straight into CSR batches (all bases
 * concatenated, all qualities concatenated, byte offsets), names and strand lines stay on the
 * host, and output is formatted from the per-read result records.
 */
#ifndef FPLH_FASTQ_H
#define FPLH_FASTQ_H

#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "batch.h"
#include "fastplong_amd.h"

namespace fplh {

class GzMembers; /* gzip.h: a gzip file that is a concatenation of members, inflated on several threads */

/* Plain or gzip FASTQ (zlib).  Line splitting follows FastqReader::getLine: a line ends at
 * '\r' or '\n', "\r\n" counts once; records whose header does not start with '@' are skipped
 * line by line; a malformed record ends the input (src/fastqreader.cpp:326-341). */
class FastqReader {
   public:
    explicit FastqReader(const std::string& path);
    /* the same reader over bytes already in memory (parse_chunk): no refill; at_eof = the bytes end the input */
    FastqReader(const char* data, size_t len, bool at_eof);
    ~FastqReader();

    /* Chunk-parallel reading of a regular, uncompressed file: the file is cut at fixed byte offsets and a record
     * belongs to the chunk its '@' falls into, so any number of threads can parse different chunks at the same
     * time.  A chunk that does not start the file has to GUESS where its first record begins (the first '@' line at
     * or behind the cut whose third line starts with '+' and whose second and fourth lines are equally long); the
     * caller checks every guess against what the chunk in front of it reports as the next record (ChunkInfo::next)
     * and parses the chunk again with exact = true when they differ, so the records are always those the
     * sequential reader finds.  Reads [a, b) of the file behind fd (plus the tail of the last record) into
     * `window`, appends the records to `out`. */
    struct ChunkInfo {
        static constexpr uint64_t NONE = ~0ull;
        uint64_t first = NONE; /* file offset of the first record taken, NONE when the chunk holds none */
        uint64_t next = NONE;  /* file offset at which the next record starts: the first '@' line behind the last
                                  record taken that lies at or behind b (NONE after the end of input / a bad record) */
        int status = 0;        /* 0 = more input follows, 2 = end of input reached, 3 = malformed record, 4 = read error (message in err) */
        std::string err;
    };
    /* (mem != nullptr: the input's bytes [0, file_size) are in memory there and are parsed in place; fd is not used) */
    static bool parse_chunk(int fd, uint64_t file_size, uint64_t a, uint64_t b, bool exact, std::vector<char>& window,
                            Batch& out, ChunkInfo& info, int threads, const char* mem = nullptr);
    /* The same chunk as TEXT for the device to parse (Batch::raw): the bytes [a - 1, b + slack) are read into out.raw and only
     * the two ends are looked at -- the first record of this chunk and the first record of the next, both by the guess
     * parse_chunk makes -- so the records of the text are exactly those parse_chunk(.., exact = false) would take.  No line
     * in between is scanned and no base copied a second time. */
    static bool load_chunk_text(int fd, uint64_t file_size, uint64_t a, uint64_t b, uint64_t chunk_bytes, Batch& out, ChunkInfo& info,
                                const char* mem = nullptr);
    bool ok() const { return fp_ != nullptr; }
    /* append records until the batch holds >= max_bases bases or max_reads reads; returns the
     * number of records appended (0 at end of input) */
    uint32_t fill(Batch& b, uint64_t max_bases, uint32_t max_reads);
    bool malformed() const { return malformed_; }
    /* decompression / read errors end the input like the end of the file does, but are remembered: the reference
       aborts there (error_exit in src/fastqreader.cpp:92-137), so the caller must not report success */
    bool input_error() const { return !io_error_.empty(); }
    const std::string& input_error_text() const { return io_error_; }
    /* offset, in the (uncompressed) input, of the byte behind the last record handed out */
    uint64_t consumed() const { return pulled_ - (len_ - pos_); }

    void set_copy_threads(int t) { copy_threads_ = t < 1 ? 1 : t; }

   private:
    struct Line {
        const char* p;
        size_t n;
    };
    struct Rec {
        Line name, seq, strand, qual;
        size_t end; /* window position behind the record's last line terminator */
    };
    /* The input is scanned in place (one SIMD pass for both terminators) in one large window that is refilled
     * behind the unconsumed tail: by gzread for gzip and pipes, by parallel pread for a regular uncompressed
     * file (whose window grows to hold a whole batch, so that the scan can be split over threads too).  fill() first only LOCATES the records of a stretch of the window, then copies their
     * lines into the batch on copy_threads_ threads.  scan_line: 1 = a line, 0 = the window ends inside the
     * line and more input exists, -1 = end of input with nothing left. */
    int scan_line(size_t& pos, Line& ln) const;
    int scan_records(size_t& pos, size_t start_limit, uint64_t& bases, uint64_t max_bases, uint32_t& reads,
                     uint32_t max_reads, std::vector<Rec>& recs, std::string& err) const;
    size_t next_at_line(size_t from) const;
    /* the guess of where records start (scan_parallel, parse_chunk, load_chunk_text): HEADER_CUT = the window ends inside the
       four lines while the input goes on */
    enum Header { HEADER_NO, HEADER_YES, HEADER_CUT };
    Header header_at(size_t cand) const;
    size_t line_start(size_t pos) const;
    void scan_parallel(uint64_t& bases, uint64_t max_bases, uint32_t& reads, uint32_t max_reads, std::vector<Rec>& recs);
    bool pull(); /* stream mode: keep [pos_, len_), read more behind it (growing the window when a record fills it) */
    void copy_records(Batch& b, const std::vector<Rec>& recs) const;
    void* fp_ = nullptr;       /* gzFile (gzip, pipes) or a non-null token (regular file, fd_ / members_) */
    GzMembers* members_ = nullptr; /* multi-member gzip file: parallel inflate */
    const char* win_ = nullptr; /* the window: buf_.data() */
    std::vector<char> buf_;
    int fd_ = -1;              /* regular uncompressed file: refilled with parallel pread */
    uint64_t file_size_ = 0, file_pos_ = 0, pulled_ = 0;
    size_t pos_ = 0, len_ = 0;
    int copy_threads_ = 1;
    size_t parse_min_ = 8u << 20; /* smallest piece worth a scanning thread (FPLH_PARSE_MIN: test hook) */
    bool eof_ = false, malformed_ = false;
    bool mem_ = false; /* memory mode: the window is the caller's */
    std::string io_error_, path_;
};

/* The chunk-parallel reader built on FastqReader::parse_chunk: `threads` parser threads take chunks of
 * `chunk_bytes` in file order, each into a Batch it obtains from `acquire` (blocking; the caller's pool bounds how far
 * the parsers run ahead); next() hands the non-empty batches back in input order after checking every chunk's guessed
 * start against its predecessor (a chunk whose guess was wrong is parsed again from the known offset, on the calling
 * thread), and returns the batches it does not pass on through `release`.  The records are exactly those the
 * sequential FastqReader finds (tests/test_host_io.py::test_chunked_reader_equals_sequential). */
class ChunkedReader {
   public:
    struct Item {
        Batch* batch = nullptr;
        void* token = nullptr; /* the caller's handle for the batch (e.g. the Work object it lives in) */
    };
    /* as_text: the parsers only LOAD their chunks (FastqReader::load_chunk_text, text-backed batches) */
    ChunkedReader(int fd, uint64_t file_size, uint64_t chunk_bytes, int threads, std::function<Item()> acquire,
                  std::function<void(Item)> release, const char* mem = nullptr, bool as_text = false);
    ~ChunkedReader();
    /* the next batch in input order; false at the end of the input (or behind a malformed record / read error) */
    bool next(Item& out);
    const std::string& malformed_text() const { return malformed_; } /* "" or the reference's message for a bad record */
    const std::string& io_error_text() const { return io_error_; }
    /* input offset below which no parser will look again (the chunks in front of the one the sequencer took last): the
       owner of an in-memory input may give those pages back */
    uint64_t dead_below() const;
    uint64_t chunks_parsed_again() const { return n_redo_; }
    double redo_seconds() const { return t_redo_; }
    double busiest_parser_seconds() const;

   private:
    struct Impl;
    Impl* d_;
    std::string malformed_, io_error_;
    uint64_t n_redo_ = 0;
    double t_redo_ = 0;
};


/* --break / --mask: the outcome list of a batch (fpl_get_fragments: sorted by read, then seq_no) and where
 * each read's records start */
struct FragmentList {
    std::vector<fpl_fragment> frags;
    std::vector<fpl_region> regs;
    std::vector<uint32_t> first; /* n + 1: fragments of read i are [first[i], first[i+1]) */
    void index(uint32_t n_reads);
};

/* Serialize what src/seprocessor.cpp:265-281 writes for one batch: passing fragments to `out`
 * (name with the split prefix when the read was broken), and -- when failed != nullptr -- the
 * trimmed read with its tag for reads that produced exactly one fragment and failed. */
void format_batch(const Batch& b, const fpl_read_result* res, std::string& out, std::string* failed);
/* the same for reads [first, last) only (appends) */
void format_range(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, std::string& out,
                  std::string* failed, const FragmentList* fl = nullptr);
/* the same on `threads` host threads: piece t of outs / faileds holds the text of the t-th slice of the
 * batch, so writing the pieces in order gives format_batch's output */
void format_batch_parallel(const Batch& b, const fpl_read_result* res, int threads, std::vector<std::string>& outs,
                           std::vector<std::string>* faileds, const FragmentList* fl = nullptr);

}  // namespace fplh
#endif
