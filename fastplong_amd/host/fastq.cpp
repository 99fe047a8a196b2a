#include "fastq.h"

#include <fcntl.h>
#include <immintrin.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <iostream>
#include <map>
#include <mutex>
#include <thread>

#include "gzip.h"
#include "pool.h"
#include "timing.h"

using namespace std;

namespace fplh {

/* index of the first '\n' or '\r' in p[0, n), or n: one pass for both terminators */
static size_t find_eol_sse2(const char* p, size_t n) {
    const __m128i nl = _mm_set1_epi8('\n'), cr = _mm_set1_epi8('\r');
    size_t i = 0;
    for (; i + 16 <= n; i += 16) {
        const __m128i v = _mm_loadu_si128((const __m128i*)(p + i));
        const int m = _mm_movemask_epi8(_mm_or_si128(_mm_cmpeq_epi8(v, nl), _mm_cmpeq_epi8(v, cr)));
        if (m) return i + (size_t)__builtin_ctz((unsigned)m);
    }
    for (; i < n; i++)
        if (p[i] == '\n' || p[i] == '\r') return i;
    return n;
}
__attribute__((target("avx2"))) static size_t find_eol_avx2(const char* p, size_t n) {
    const __m256i nl = _mm256_set1_epi8('\n'), cr = _mm256_set1_epi8('\r');
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        const __m256i a = _mm256_loadu_si256((const __m256i*)(p + i)), b = _mm256_loadu_si256((const __m256i*)(p + i + 32));
        const unsigned ma = (unsigned)_mm256_movemask_epi8(_mm256_or_si256(_mm256_cmpeq_epi8(a, nl), _mm256_cmpeq_epi8(a, cr)));
        const unsigned mb = (unsigned)_mm256_movemask_epi8(_mm256_or_si256(_mm256_cmpeq_epi8(b, nl), _mm256_cmpeq_epi8(b, cr)));
        if (ma | mb) return i + (size_t)__builtin_ctzll((unsigned long long)ma | ((unsigned long long)mb << 32));
    }
    return i + find_eol_sse2(p + i, n - i);
}
static size_t find_eol(const char* p, size_t n) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    return avx2 ? find_eol_avx2(p, n) : find_eol_sse2(p, n);
}

/* the reference's words for a gzip stream that ends early / does not decode (src/fastqreader.cpp:92-137) */
static string gz_error_text(int zerr, const string& path) {
    return zerr == Z_BUF_ERROR ? string("igzip: unexpected eof") : "igzip: encountered while decompressing file: " + path;
}

FastqReader::FastqReader(const string& path) {
    path_ = path;
    size_t cap = 32u << 20;
    bool allow_map = true;
    if (const char* e = getenv("FPLH_READ_WINDOW")) /* test hook: tiny windows exercise the refill paths */
        if (atol(e) > 0) {
            cap = (size_t)atol(e);
            allow_map = false;
        }
    if (const char* e = getenv("FPLH_PARSE_MIN"))
        if (atol(e) > 0) parse_min_ = (size_t)atol(e);
    if (const char* e = getenv("FPLH_PARSE_THREADS"))
        if (atol(e) > 0) copy_threads_ = (int)atol(e);
    if (path != "/dev/stdin" && allow_map) { /* a regular file that is not gzip: parallel pread into the window */
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd >= 0) {
            struct stat st;
            unsigned char magic[2] = {0, 0};
            if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && pread(fd, magic, 2, 0) == 2 &&
                !(magic[0] == 0x1f && magic[1] == 0x8b)) {
                fd_ = fd;
                file_size_ = (uint64_t)st.st_size;
                fp_ = this;
            } else {
                close(fd);
            }
        }
    }
    if (fd_ < 0 && path != "/dev/stdin" && allow_map && !getenv("FPLH_NO_GZ_MEMBERS")) {
        members_ = GzMembers::open(path, max(copy_threads_, 16)); /* inflate is compute-bound: more workers than the memory-bound phases use */
        if (members_) fp_ = this;
    }
    if (fd_ < 0 && !members_) {
        /* gzopen reads plain files transparently */
        fp_ = path == "/dev/stdin" ? (void*)gzdopen(0, "rb") : (void*)gzopen(path.c_str(), "rb");
        if (fp_) gzbuffer((gzFile)fp_, 1 << 20);
    }
    buf_.resize(cap);
    win_ = buf_.data();
}

FastqReader::FastqReader(const char* data, size_t len, bool at_eof) {
    mem_ = true;
    fp_ = this;
    win_ = data;
    len_ = len;
    pulled_ = len;
    eof_ = at_eof;
}

FastqReader::~FastqReader() {
    if (mem_) return;
    if (fd_ >= 0) close(fd_);
    else if (members_) delete members_;
    else if (fp_) gzclose((gzFile)fp_);
}

/* pread until dst[0 .. n) holds the file's bytes from `at`; false: the file ended (or failed) before that */
static bool pread_full(int fd, char* dst, size_t n, uint64_t at) {
    for (size_t x = 0; x < n;) {
        const ssize_t r = pread(fd, dst + x, n - x, (off_t)(at + x));
        if (r <= 0) return false;
        x += (size_t)r;
    }
    return true;
}
/* the same on T pool threads, each its slice of the range */
static bool pread_sliced(int fd, char* dst, size_t n, uint64_t at, int T) {
    std::atomic<bool> ok{true};
    parallel_run(T, [&](int t) {
        const size_t a = n / T * t, e = t == T - 1 ? n : n / T * (t + 1);
        if (!pread_full(fd, dst + a, e - a, at + a)) ok = false;
    });
    return ok;
}

bool FastqReader::pull() {
    if (eof_ || !fp_ || mem_) return false;
    if (pos_ > 0) {
        memmove(buf_.data(), buf_.data() + pos_, len_ - pos_);
        len_ -= pos_;
        pos_ = 0;
    } else if (len_ == buf_.size()) {
        buf_.resize(buf_.size() * 2); /* one record is larger than the window */
    }
    win_ = buf_.data();
    if (fd_ >= 0) { /* regular file: every thread preads its slice of the free part of the window */
        const size_t want = (size_t)min<uint64_t>(buf_.size() - len_, file_size_ - file_pos_);
        const int T = (int)max<size_t>(1, min<size_t>((size_t)copy_threads_, want / (4u << 20)));
        if (!pread_sliced(fd_, buf_.data() + len_, want, file_pos_, T)) {
            eof_ = true; /* (truncated underneath us: stop with what was read so far, and say so) */
            io_error_ = "reading " + path_ + " failed (file truncated while it was being read?)";
            return true;
        }
        len_ += want;
        pulled_ += want;
        file_pos_ += want;
        if (file_pos_ >= file_size_) eof_ = true;
        return true;
    }
    if (members_) {
        const size_t n = members_->read(buf_.data() + len_, buf_.size() - len_);
        if (n == 0) eof_ = true;
        if (members_->error()) {
            eof_ = true;
            io_error_ = gz_error_text(members_->error(), path_);
        }
        len_ += n;
        pulled_ += n;
        return true;
    }
    while (len_ < buf_.size()) { /* gzread returns short counts on pipes */
        const size_t want = min<size_t>(buf_.size() - len_, 1u << 30);
        const int n = gzread((gzFile)fp_, buf_.data() + len_, (unsigned)want);
        if (n <= 0) {
            eof_ = true;
            int errnum = Z_OK;
            gzerror((gzFile)fp_, &errnum);
            if (n < 0 || (errnum != Z_OK && errnum != Z_STREAM_END)) io_error_ = gz_error_text(errnum == Z_OK ? Z_ERRNO : errnum, path_);
            break;
        }
        len_ += (size_t)n;
        pulled_ += (uint64_t)n;
    }
    return true;
}

/* FastqReader::getLine, src/fastqreader.cpp:219-312: a line ends at '\r' or '\n', "\r\n" counts once */
int FastqReader::scan_line(size_t& pos, Line& ln) const {
    if (pos >= len_) return eof_ ? -1 : 0;
    const char* b = win_ + pos;
    const size_t avail = len_ - pos;
    const size_t e = find_eol(b, avail);
    if (e == avail) { /* no terminator in the window */
        if (!eof_) return 0;
        ln = Line{b, avail};
        pos = len_;
        return 1;
    }
    size_t next = pos + e + 1;
    if (b[e] == '\r') { /* swallow the '\n' of "\r\n": needs the byte after it */
        if (next >= len_ && !eof_) return 0;
        if (next < len_ && win_[next] == '\n') next++;
    }
    ln = Line{b, e};
    pos = next;
    return 1;
}

/* append the located records to the batch: offsets first, then the line copies on copy_threads_ threads */
void FastqReader::copy_records(Batch& b, const vector<Rec>& recs) const {
    const size_t n0 = b.n(), nr = recs.size();
    if (nr == 0) return;
    const size_t base0 = b.seq.size(), text0 = b.text.size();
    uint64_t bases = base0, text = text0;
    b.off.reserve(n0 + nr + 1);
    for (const Rec& r : recs) {
        bases += r.seq.n;
        text += r.name.n + r.strand.n;
        b.off.push_back(bases);
        b.name_off.push_back(text);
        b.name_len.push_back((uint32_t)r.name.n);
        b.strand_len.push_back((uint32_t)r.strand.n);
    }
    b.seq.resize_uninit(bases);
    b.qual.resize_uninit(bases);
    b.text.resize(text);
    auto work = [&](size_t first, size_t last) {
        for (size_t i = first; i < last; i++) {
            const Rec& r = recs[i];
            const uint64_t o = b.off[n0 + i], t = b.name_off[n0 + i];
            memcpy(b.seq.data() + o, r.seq.p, r.seq.n);
            memcpy(b.qual.data() + o, r.qual.p, r.qual.n);
            memcpy(b.text.data() + t, r.name.p, r.name.n);
            memcpy(b.text.data() + t + r.name.n, r.strand.p, r.strand.n);
        }
    };
    const int T = (bases - base0) < (8u << 20) ? 1 : copy_threads_;
    if (T <= 1) {
        work(0, nr);
        return;
    }
    vector<size_t> cut(T + 1, nr);
    cut[0] = 0;
    for (int t = 0; t < T - 1; t++) { /* slices of about equal numbers of bases */
        const uint64_t want = base0 + (bases - base0) / T * (t + 1);
        const size_t last = (size_t)(std::lower_bound(b.off.begin() + n0 + 1, b.off.begin() + n0 + 1 + nr, want) -
                                     (b.off.begin() + n0 + 1)) + 1;
        cut[t + 1] = min(max(last, cut[t]), nr);
    }
    parallel_run(T, [&](int t) { work(cut[t], cut[t + 1]); });
}

/* Locate records starting at `pos` (a line start) while they START before `start_limit` and the running totals
 * stay below the caps; `pos` ends behind the last record taken (skipped non-'@' lines in front of a taken record
 * are consumed too).  Returns 0 = stopped at a cap / the limit, 1 = the window ran out inside a record (stream
 * mode: pull and call again), 2 = end of input, 3 = malformed record at `pos` (message in `err`). */
int FastqReader::scan_records(size_t& pos, size_t start_limit, uint64_t& bases, uint64_t max_bases, uint32_t& reads,
                              uint32_t max_reads, vector<Rec>& recs, string& err) const {
    const Line none = {nullptr, 0};
    while (bases < max_bases && reads < max_reads) {
        /* one record = the next line that starts with '@' (src/fastqreader.cpp:316-319) and the three lines after
           it; lines missing at the end of the input read as empty, as getLine() does */
        Rec rc = {none, none, none, none, 0};
        size_t p = pos, rec_start = pos;
        int r;
        for (;;) {
            rec_start = p;
            r = scan_line(p, rc.name);
            if (r <= 0) break;
            if (rc.name.n > 0 && rc.name.p[0] == '@') break;
            pos = p; /* a skipped line is consumed for good */
        }
        if (r == 0) return 1;
        if (r < 0) return 2;
        if (rec_start >= start_limit) return 0; /* belongs to the next stretch */
        Line* rest[3] = {&rc.seq, &rc.strand, &rc.qual};
        for (int k = 0; k < 3; k++) {
            r = scan_line(p, *rest[k]);
            if (r == 0) return 1; /* the record continues beyond the window: restart it after reading more */
            if (r < 0) *rest[k] = none;
        }
        if (rc.strand.n == 0 || rc.strand.p[0] != '+') {
            err = string(rc.name.p, rc.name.n) + "\nExpected '+', got " + string(rc.strand.p ? rc.strand.p : "", rc.strand.n) +
                  "\nYour FASTQ may be invalid, please check the tail of your FASTQ file\n";
            return 3;
        }
        if (rc.qual.n != rc.seq.n) {
            err = "ERROR: sequence and quality have different length:\n" + string(rc.name.p, rc.name.n) + "\n" +
                  string(rc.seq.p ? rc.seq.p : "", rc.seq.n) + "\n" + string(rc.strand.p, rc.strand.n) + "\n" +
                  string(rc.qual.p ? rc.qual.p : "", rc.qual.n) +
                  "\nYour FASTQ may be invalid, please check the tail of your FASTQ file\n";
            return 3;
        }
        pos = p;
        rc.end = p;
        recs.push_back(rc);
        bases += rc.seq.n;
        reads++;
    }
    return 0;
}

static std::atomic<uint64_t> g_parallel_records{0}; /* records taken from the multi-threaded scan (test hook) */

/* first position >= from that starts a line beginning with '@' (what the sequential scan would take next) */
size_t FastqReader::next_at_line(size_t from) const {
    size_t p = from;
    Line ln;
    for (;;) {
        const size_t at = p;
        const int r = scan_line(p, ln);
        if (r <= 0) return len_;
        if (ln.n > 0 && ln.p[0] == '@') return at;
    }
}

/* Does a record header validate at `cand` (an '@' line): its third line starts with '+', its second and fourth are equally long */
FastqReader::Header FastqReader::header_at(size_t cand) const {
    Line l[4];
    for (int k = 0; k < 4; k++) {
        const int r = scan_line(cand, l[k]);
        if (r != 1) return r == 0 ? HEADER_CUT : HEADER_NO;
    }
    return l[2].n > 0 && l[2].p[0] == '+' && l[1].n == l[3].n ? HEADER_YES : HEADER_NO;
}

/* `pos`, or the start of the next line when pos lies inside one (finish the line we fell into) */
size_t FastqReader::line_start(size_t pos) const {
    Line ln;
    if (pos > 0 && win_[pos - 1] != '\n' && win_[pos - 1] != '\r') scan_line(pos, ln);
    return pos;
}

/* Regular files: the stretch of the window that should hold the rest of the batch is cut into one piece per thread.
 * A thread starts at the first line in its piece that looks like a record header ('@' line whose third line
 * starts with '+' and whose second and fourth lines are equally long) and locates the records that start in its
 * piece.  The pieces are then joined in order, but only while thread k's first record is exactly the '@' line the
 * sequential scan would have taken after thread k-1's last record: anything else (a quality line that passed for
 * a header, junk between records, a malformed record) ends the join there and the sequential scan carries on, so
 * the result never differs from the one-thread reader's. */
void FastqReader::scan_parallel(uint64_t& bases, uint64_t max_bases, uint32_t& reads, uint32_t max_reads, vector<Rec>& recs) {
    const uint64_t want = max_bases - bases;
    size_t stretch = (size_t)min<uint64_t>(len_ - pos_, want * 2 + want / 8 + (1u << 20));
    const int T = (int)min<size_t>((size_t)copy_threads_, stretch / parse_min_);
    if (T < 2) return;
    const size_t piece = stretch / T;
    struct Part {
        vector<Rec> recs;
        size_t first = 0, end = 0; /* start of the first record, position behind the last one */
        uint64_t bases = 0;
        uint32_t reads = 0;
        int rc = 0;
    };
    vector<Part> parts(T);
    parallel_run(T, [&](int k) {
        {
            Part& pt = parts[k];
            const size_t lo = pos_ + (size_t)k * piece, hi = k == T - 1 ? pos_ + stretch : lo + piece;
            size_t p = lo;
            if (k > 0) { /* find a header that validates */
                Line ln;
                size_t q = line_start(lo);
                for (;;) {
                    const size_t cand = next_at_line(q);
                    if (cand >= hi) {
                        pt.first = pt.end = hi;
                        pt.rc = -1; /* no record starts in this piece */
                        return;
                    }
                    if (header_at(cand) == HEADER_YES) {
                        p = cand;
                        break;
                    }
                    q = cand;
                    scan_line(q, ln); /* not a header: move past this line */
                }
            }
            pt.first = next_at_line(p);
            size_t pos = p;
            string err;
            pt.rc = scan_records(pos, hi, pt.bases, ~0ull, pt.reads, 0xFFFFFFFFu, pt.recs, err);
            pt.end = pos;
        }
    });
    /* join in order while the pieces line up with the sequential scan */
    for (int k = 0; k < T; k++) {
        Part& pt = parts[k];
        if (pt.rc == -1) continue; /* (empty piece: the next one must still line up with pos_) */
        if (next_at_line(pos_) != pt.first || pt.recs.empty()) return;
        for (const Rec& r : pt.recs) {
            if (bases >= max_bases || reads >= max_reads) return;
            recs.push_back(r);
            g_parallel_records++;
            bases += r.seq.n;
            reads++;
            pos_ = r.end;
        }
        if (pt.rc != 0) return; /* end of input or a malformed record: the sequential scan reports it */
    }
}

bool FastqReader::parse_chunk(int fd, uint64_t file_size, uint64_t a, uint64_t b, bool exact, vector<char>& window,
                              Batch& out, ChunkInfo& info, int threads, const char* mem) {
    info = ChunkInfo();
    out.start_offsets();
    if (a >= file_size) {
        info.status = 2;
        return true;
    }
    if (b > file_size) b = file_size;
    const uint64_t w0 = (exact || a == 0) ? a : a - 1; /* (a guessing chunk looks at the byte in front of the cut) */
    if (threads < 1) threads = 1;
    for (uint64_t slack = 4u << 20;; slack *= 4) { /* the last record may run past b: read on, more if it has to be */
        const double t_begin = now_s();
        const uint64_t w1 = min<uint64_t>(file_size, b + slack);
        const size_t n = (size_t)(w1 - w0);
        const char* wp = mem ? mem + w0 : nullptr; /* the bytes [w0, w1): in place when the input is in memory */
        if (!mem) {
            if (window.size() < n) window.resize(n);
            wp = window.data();
            const int T = (int)max<size_t>(1, min<size_t>((size_t)threads, n / (8u << 20)));
            if (!pread_sliced(fd, window.data(), n, w0, T)) {
                info.status = 4;
                info.err = "reading the input failed (file truncated while it was being read?)";
                return false;
            }
        }
        const double t_read = now_s();
        FastqReader m(wp, n, w1 >= file_size);
        m.copy_threads_ = threads;
        size_t pos = (size_t)(a - w0);
        if (!exact && a > 0) { /* the first header at or behind the cut that validates (see scan_parallel) */
            Line ln;
            pos = m.line_start(pos);
            for (;;) {
                const size_t cand = m.next_at_line(pos);
                if (cand >= n) {
                    pos = n;
                    break;
                }
                if (m.header_at(cand) == HEADER_YES || cand >= (size_t)(b - w0)) { /* (beyond the chunk nothing is taken anyway) */
                    pos = cand;
                    break;
                }
                pos = cand;
                m.scan_line(pos, ln); /* not a header: move past this line */
            }
        }
        vector<Rec> recs;
        uint64_t bases = 0;
        uint32_t reads = 0;
        string err;
        const int rc = m.scan_records(pos, (size_t)(b - w0), bases, ~0ull, reads, 0xFFFFFFFFu, recs, err);
        if (rc == 1) continue; /* the window ends inside a record although the file goes on */
        if (!recs.empty()) info.first = w0 + (uint64_t)(recs[0].name.p - wp);
        const double t_scan = now_s();
        m.copy_records(out, recs);
        if (g_timing) {
            const double t_copy = now_s();
            g_chunk_us[0].fetch_add((uint64_t)((t_read - t_begin) * 1e6));
            g_chunk_us[1].fetch_add((uint64_t)((t_scan - t_read) * 1e6));
            g_chunk_us[2].fetch_add((uint64_t)((t_copy - t_scan) * 1e6));
        }
        if (rc == 0) info.next = w0 + pos;
        else if (rc == 2) info.status = 2;
        else {
            info.status = 3;
            info.err = err;
        }
        return true;
    }
}

bool FastqReader::load_chunk_text(int fd, uint64_t file_size, uint64_t a, uint64_t b, uint64_t chunk_bytes, Batch& out, ChunkInfo& info,
                                  const char* mem) {
    info = ChunkInfo();
    out.text_backed = true;
    out.raw_begin = out.raw_len = 0;
    if (a >= file_size) {
        info.status = 2;
        return true;
    }
    if (b > file_size) b = file_size;
    const uint64_t w0 = a == 0 ? 0 : a - 1; /* (the guess looks at the byte in front of the cut) */
    for (uint64_t slack = 4u << 20;; slack *= 4) {
        const uint64_t w1 = min<uint64_t>(file_size, b + slack);
        const size_t n = (size_t)(w1 - w0);
        out.raw.resize_uninit(n);
        char* wp = (char*)out.raw.data();
        if (mem) {
            memcpy(wp, mem + w0, n);
        } else if (!pread_full(fd, wp, n, w0)) {
            info.status = 4;
            info.err = "reading the input failed (file truncated while it was being read?)";
            return false;
        }
        FastqReader m(wp, n, w1 >= file_size);
        /* The first header at or behind `pos` that VALIDATES (its third line starts with '+', its second and fourth are equally
           long).  parse_chunk's guess stops at the first candidate beyond its chunk, valid or not, because it takes nothing from
           there anyway and the sequencer puts a wrong announcement right; here the position IS the end of this chunk's text and the
           start of the next one's, so both are searched to the end -- through a read of any length (the window grows).
           short_of_window: the search ran into the end of the window although the file goes on */
        bool short_of_window = false;
        auto find_header = [&](size_t pos) -> size_t {
            Line ln;
            pos = m.line_start(pos);
            for (;;) {
                const size_t cand = m.next_at_line(pos);
                if (cand >= n) {
                    if (w1 < file_size) short_of_window = true;
                    return n;
                }
                const Header h = m.header_at(cand);
                if (h == HEADER_CUT) { /* the window ends inside these four lines and the file goes on */
                    short_of_window = true;
                    return n;
                }
                if (h == HEADER_YES) return cand;
                pos = cand;
                m.scan_line(pos, ln); /* not a header: move past this line */
            }
        };
        size_t first = (size_t)(a - w0), next = n;
        if (a > 0) first = find_header(first);
        if (!short_of_window && b < file_size) next = first >= (size_t)(b - w0) ? first : find_header((size_t)(b - w0));
        if (short_of_window) continue;
        if (first > next) first = next;
        if (first >= (size_t)(b - w0) && b < file_size) first = next; /* no record STARTS in this chunk */
        out.raw_begin = first;
        out.raw_len = next - first;
        if (out.raw_len > 0) info.first = w0 + first;
        if (b >= file_size) info.status = 2; /* the end of the input */
        else info.next = w0 + next;
        return true;
    }
}

struct TimingDump {
    ~TimingDump() {
        if (!g_timing) return;
        fprintf(stderr, "reader phases: refill %.3f s, locate %.3f s, copy %.3f s\n", g_t_pull, g_t_scan, g_t_copy);
        fprintf(stderr, "chunk parsers (summed over threads): read %.3f s, locate %.3f s, copy %.3f s; page-locked allocations %.3f s for %.2f GB\n",
                g_chunk_us[0].load() * 1e-6, g_chunk_us[1].load() * 1e-6, g_chunk_us[2].load() * 1e-6,
                g_alloc_seconds_x1000.load() * 1e-6, g_alloc_bytes.load() * 1e-9);
    }
} g_timing_dump;

uint32_t FastqReader::fill(Batch& b, uint64_t max_bases, uint32_t max_reads) {
    b.start_offsets();
    uint32_t added = 0;
    vector<Rec> recs;
    uint64_t bases = b.seq.size();
    uint32_t reads = b.n();
    bool end = false;
    while (!end && !malformed_ && bases < max_bases && reads < max_reads) {
        recs.clear();
        if (fd_ >= 0 && max_bases < (1ull << 40) && !eof_) { /* have the stretch this batch needs in the window */
            const uint64_t want = max_bases - bases;
            const size_t stretch = (size_t)min<uint64_t>(file_size_ - (file_pos_ - (len_ - pos_)), want * 2 + want / 8 + (1u << 20));
            if (len_ - pos_ < stretch) {
                if (buf_.size() < stretch + (16u << 20)) { /* grow the window once (it is reused for every batch) */
                    vector<char> nb(stretch + (16u << 20));
                    memcpy(nb.data(), buf_.data() + pos_, len_ - pos_);
                    len_ -= pos_;
                    pos_ = 0;
                    buf_.swap(nb);
                    win_ = buf_.data();
                }
                const double t0 = now_s();
                pull();
                g_t_pull += now_s() - t0;
            }
        }
        const double t1 = now_s();
        /* (only when the batch is cut by bases: with a small read cap the stretch to scan cannot be sized) */
        if (fd_ >= 0 && copy_threads_ > 1 && max_bases < (1ull << 40) && max_reads - reads >= (1u << 24))
            scan_parallel(bases, max_bases, reads, max_reads, recs);
        /* locate the (remaining) records of the current window sequentially */
        string err;
        const int rc = scan_records(pos_, len_, bases, max_bases, reads, max_reads, recs, err);
        const double t2 = now_s();
        copy_records(b, recs); /* before the window moves */
        g_t_scan += t2 - t1;
        g_t_copy += now_s() - t2;
        added += (uint32_t)recs.size();
        if (rc == 3) {
            cerr << err;
            malformed_ = true;
        } else if (rc == 2) {
            end = true;
        } else if (rc == 1 && !pull()) {
            end = true;
        }
    }
    return added;
}

struct ChunkedReader::Impl {
    int fd;
    const char* mem = nullptr;
    uint64_t file_size, chunk_bytes, n_chunks;
    std::function<Item()> acquire;
    std::function<void(Item)> release;
    struct Parsed {
        Item item;
        FastqReader::ChunkInfo info;
    };
    mutex take_mu, parsed_mu;
    condition_variable parsed_cv;
    map<uint64_t, Parsed> parsed;
    uint64_t next_chunk = 0, seq_chunk = 0, expected = 0;
    bool stop = false, done = false;
    vector<std::thread> threads;
    vector<double> busy;
    vector<char> window; /* of the calling thread, for chunks that are parsed again */
    bool as_text = false;
};

ChunkedReader::ChunkedReader(int fd, uint64_t file_size, uint64_t chunk_bytes, int threads, std::function<Item()> acquire,
                             std::function<void(Item)> release, const char* mem, bool as_text) {
    d_ = new Impl;
    d_->fd = fd;
    d_->mem = mem;
    d_->as_text = as_text;
    d_->file_size = file_size;
    d_->chunk_bytes = chunk_bytes ? chunk_bytes : 1;
    d_->n_chunks = (file_size + d_->chunk_bytes - 1) / d_->chunk_bytes;
    d_->acquire = acquire;
    d_->release = release;
    if (threads < 1) threads = 1;
    d_->busy.assign(threads, 0.0);
    for (int t = 0; t < threads; t++)
        d_->threads.emplace_back([this, t]() {
            Impl& D = *d_;
            vector<char> window;
            for (;;) {
                /* a batch first, then the chunk number: chunk numbers are only ever handed to threads that already
                   hold a batch, so the lowest chunk not yet parsed never waits behind later chunks for one (the
                   batches of the chunks in front of it are on their way through the caller's pipeline and come back) */
                Impl::Parsed ps;
                uint64_t k;
                {
                    lock_guard<mutex> g(D.take_mu);
                    if (D.stop || D.next_chunk >= D.n_chunks) break;
                }
                ps.item = D.acquire(); /* may block; not under the lock */
                if (!ps.item.batch) break;
                {
                    lock_guard<mutex> g(D.take_mu);
                    if (D.stop || D.next_chunk >= D.n_chunks) {
                        D.release(ps.item);
                        break;
                    }
                    k = D.next_chunk++;
                }
                ps.item.batch->clear();
                const double t0 = now_s();
                if (D.as_text)
                    FastqReader::load_chunk_text(D.fd, D.file_size, k * D.chunk_bytes, (k + 1) * D.chunk_bytes, D.chunk_bytes,
                                                 *ps.item.batch, ps.info, D.mem);
                else
                    FastqReader::parse_chunk(D.fd, D.file_size, k * D.chunk_bytes, (k + 1) * D.chunk_bytes, false, window,
                                             *ps.item.batch, ps.info, 1, D.mem);
                D.busy[t] += now_s() - t0;
                {
                    lock_guard<mutex> g(D.parsed_mu);
                    D.parsed[k] = std::move(ps);
                }
                D.parsed_cv.notify_all();
            }
        });
}

ChunkedReader::~ChunkedReader() {
    {
        lock_guard<mutex> g(d_->take_mu);
        d_->stop = true;
    }
    for (auto& t : d_->threads) t.join();
    for (auto& kv : d_->parsed) d_->release(kv.second.item);
    delete d_;
}

uint64_t ChunkedReader::dead_below() const {
    return d_->seq_chunk >= 2 ? (d_->seq_chunk - 2) * d_->chunk_bytes : 0; /* (seq_chunk - 1 was taken last; one chunk of margin) */
}

double ChunkedReader::busiest_parser_seconds() const {
    double m = 0;
    for (double x : d_->busy) m = max(m, x);
    return m;
}

bool ChunkedReader::next(Item& out) {
    Impl& D = *d_;
    while (!D.done && D.seq_chunk < D.n_chunks) {
        const uint64_t k = D.seq_chunk++;
        Impl::Parsed ps;
        {
            unique_lock<mutex> g(D.parsed_mu);
            D.parsed_cv.wait(g, [&] { return D.parsed.count(k) > 0; });
            ps = std::move(D.parsed[k]);
            D.parsed.erase(k);
        }
        const uint64_t a = k * D.chunk_bytes, b = (k + 1) * D.chunk_bytes;
        const bool has = ps.info.first != FastqReader::ChunkInfo::NONE;
        /* the chunk's first record must be the one its predecessor announced */
        const bool ok = k == 0 || (has ? ps.info.first == D.expected : (ps.info.status == 0 && ps.info.next == D.expected));
        if (!ok) { /* the guess was wrong (or there was nothing to find): parse again from the known start */
            const double t0 = now_s();
            ps.item.batch->clear();
            if (D.expected >= b) { /* the record in front runs across this whole chunk */
                ps.info = FastqReader::ChunkInfo();
                ps.info.next = D.expected;
                ps.item.batch->start_offsets();
            } else {
                const int hw = effective_cpus();
                FastqReader::parse_chunk(D.fd, D.file_size, max(a, D.expected), b, true, D.window, *ps.item.batch, ps.info,
                                         max(1, min(8, hw / 2)), D.mem);
            }
            t_redo_ += now_s() - t0;
            n_redo_++;
        }
        D.expected = ps.info.next;
        if (ps.info.status == 3) malformed_ = ps.info.err;
        if (ps.info.status == 4) io_error_ = ps.info.err;
        if (ps.info.status != 0) { /* end of input, or a malformed record / a read error ends it */
            D.done = true;
            lock_guard<mutex> g(D.take_mu);
            D.stop = true;
        }
        if (ps.item.batch->has_records()) {
            out = ps.item;
            return true;
        }
        D.release(ps.item);
    }
    return false;
}

}  // namespace fplh

extern "C" uint64_t fplh_parallel_records(void) { return fplh::g_parallel_records.exchange(0); } /* (test hook: since the last call) */
