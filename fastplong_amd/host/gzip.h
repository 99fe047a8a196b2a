/*
 * gzip.h -- gzip members: written for the output files (libdeflate, the library the reference's Writer uses; zlib without it),
 * and read -- one member at a time, a file of many members on the worker pool, a file of one member in one piece or window by
 * window through the device's inflater.
 */
#ifndef FPLH_GZIP_H
#define FPLH_GZIP_H

#include <stdint.h>
#include <stdlib.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <string>
#include <vector>

#include "fastplong_amd.h"

namespace fplh {

/* "ERROR: <msg>" and exit(-1) like the reference (src/util.h:270-273), for this library's writers */
[[noreturn]] __attribute__((visibility("hidden"))) void error_exit(const std::string& msg);

/* one complete gzip member holding `in` (any gzip reader takes a concatenation of members as one stream).  Whole-buffer
 * work: libdeflate does it (the library the reference's Writer uses, src/writer.cpp:110-133; loaded at run time when
 * the system has libdeflate.so.0), zlib otherwise. */
void gzip_into(const std::string& in, int level, std::string& out);
std::string gzip_member(const std::string& in, int level);
/* The same text as BGZF blocks (the container bgzip, samtools and this project's device readers take block by block): `in` cut
 * every BGZF_PIECE bytes (htslib's size), each piece deflated raw at `level` by the library gzip_into would use and framed with
 * the 18-byte header (BC extra field, BSIZE), CRC-32 and ISIZE of that piece; a piece that would not fit 65 536 - 26 bytes is
 * stored instead.  Empty input gives no bytes.  out may be the input itself.  A BGZF FILE ends with bgzf_eof(). */
constexpr size_t BGZF_PIECE = 65280;
void bgzf_into(const std::string& in, int level, std::string& out);
const std::string& bgzf_eof(); /* the 28-byte empty block */
/* bytes without std::vector's zero fill (an inflate target is overwritten anyway, and its size is a guess) */
struct RawBuf {
    char* p = nullptr;
    size_t n = 0, cap = 0;
    RawBuf() = default;
    RawBuf(const RawBuf&) = delete;
    RawBuf& operator=(const RawBuf&) = delete;
    RawBuf(RawBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr, o.n = o.cap = 0; }
    RawBuf& operator=(RawBuf&& o) noexcept {
        swap(o);
        return *this;
    }
    ~RawBuf() { free(p); }
    void swap(RawBuf& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(cap, o.cap);
    }
    void reserve(size_t c) {
        if (c > cap) {
            p = (char*)realloc(p, c);
            cap = c;
        }
    }
    void release() {
        free(p);
        p = nullptr;
        n = cap = 0;
    }
    char* data() { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    void clear() { n = 0; }
};
/* the gzip member that starts at in[0]: inflated into out, *consumed = its compressed length.  hint = a guess of the
   inflated size (0 = none).  1 = a whole member, 0 = not a (complete, undamaged) member, 2 = it inflates to more than
   cap bytes */
int gunzip_member(const unsigned char* in, size_t in_len, RawBuf& out, size_t cap, size_t* consumed, size_t hint = 0);
bool have_libdeflate();
/* one whole member straight into caller-owned memory (libdeflate only): 1 = done (*consumed input bytes, *produced output
   bytes), 2 = out_cap is too small, 0 = damaged / truncated, -1 = libdeflate is not there */
int gunzip_member_into(const unsigned char* in, size_t in_len, char* out, size_t out_cap, size_t* consumed, size_t* produced);

/* A regular file opened for reading and, when `map` is set and it holds at least min_size bytes, mapped (data stays nullptr
   otherwise; fd < 0: it could not be opened).  The destructor unmaps and closes what is still held. */
struct MappedFile {
    int fd = -1;
    const unsigned char* data = nullptr;
    size_t size = 0;
    MappedFile(const char* path, size_t min_size, bool map = true);
    ~MappedFile();
    MappedFile(const MappedFile&) = delete;
    MappedFile& operator=(const MappedFile&) = delete;
    int release_fd() { /* the descriptor becomes the caller's (gzdopen, whose gzclose closes it) */
        const int f = fd;
        fd = -1;
        return f;
    }
};

/* Gzip input made of several members.
 * One deflate stream cannot be inflated in parallel, but a gzip FILE is often a concatenation of members: bgzip
 * blocks, `cat` of the per-chunk files sequencers write, the 4 MiB flushes of fastp / fastplong, the slices of this
 * host's own writer.  Members start with 1f 8b 08 and a flag byte whose top three bits are zero; that pattern
 * also occurs inside compressed data, so a candidate only counts once a member that starts there has been inflated
 * to its end with a good CRC (zlib checks it) AND the chain of members starting at offset 0 lands on it.  Batches
 * of candidates are inflated speculatively on the worker pool; the chain walk then keeps what lines up and drops
 * the rest.  A member that inflates to more than 512 MiB (a plain `gzip` of a whole run) is not buffered:
 * from there on the file is streamed through zlib as before. */
class GzMembers {
   public:
    static std::atomic<uint64_t> delivered; /* members handed to the parser since the last fplh_gz_members() (test hook) */
    static GzMembers* open(const std::string& path, int threads);
    ~GzMembers();
    /* next bytes of the inflated stream; 0 = end of input */
    size_t read(char* dst, size_t n);
    /* The next members of the chain, inflated (at most `threads` of them at a time), in file order; false when the chain
       cannot be followed this way any further -- the end of the input (`*at_end`), or a member that is too large to
       buffer / damaged (the caller goes back to the stream) */
    bool next_group(std::vector<RawBuf>& out, bool* at_end);
    int error() const { return err_; } /* zlib's code when the stream turned out damaged or truncated, else 0 */

   private:
    struct Result {
        RawBuf out;
        size_t end = 0; /* file offset behind the member's trailer */
        int state = 0;  /* 1 = a whole member, 2 = too large to buffer, -1 = not a member */
    };
    GzMembers(const std::string& path, int threads) : file_(path.c_str(), 64), base_(file_.data), size_(file_.size), threads_(std::max(1, threads)) {}
    static bool looks_like_header(const unsigned char* p) { return p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && (p[3] & 0xE0) == 0; }
    bool member_at_pos() const { return pos_ < size_ && size_ - pos_ >= 18 && looks_like_header(base_ + pos_); }
    void find_candidates();
    void inflate_at(size_t off, Result& r) const;
    void inflate_ahead(bool with_pos); /* the candidates at and behind pos_ that are not done, on the pool (with_pos: pos_ in front) */
    void advance_to(size_t end);       /* the chain took the member that ends at `end` */
    bool next_member();                /* make the member at pos_ current; false at the end of the input */
    MappedFile file_;
    const unsigned char* base_;
    size_t size_, pos_ = 0, cur_off_ = 0;
    int threads_;
    size_t cap_ = 512ull << 20; /* largest inflated member that is buffered */
    std::vector<size_t> cands_;
    std::map<size_t, Result> done_;
    RawBuf cur_;
    gzFile stream_ = nullptr;
    int err_ = 0;
};

/* --device_inflate for a one-member .gz: the single-member lane of gunzip_members_to_memory hands the member's deflate payload
 * to `fn` (fpl_inflate_gzip, or a test's stand-in) window by window -- window_bytes of compressed data from the byte of the bit
 * where the window before ended, the last 32 KiB of text as the dictionary, the text straight into the lane's destination.  THE
 * HOST STAYS THE JUDGE: the member's CRC-32 and size are checked here, from the windows' CRCs folded with crc32_combine.  A window
 * that is refused, a call that fails or a window that hardly advances: zlib inflates from that window's start bit to the member's
 * end (inflatePrime + inflateSetDictionary).  A trailer that does not agree: the whole member goes through the host lane, as
 * without the hook.  fn == nullptr takes the hook out.  window_bytes 0: 32 MiB. */
typedef int (*GzipInflateFn)(void* user, const uint8_t* comp, uint64_t comp_bytes, uint64_t start_bit, const uint8_t* dict, uint32_t dict_len,
                             uint8_t* out, uint64_t out_cap, uint32_t chunk_bytes, fpl_gzip_window* res);
void set_gzip_inflater(GzipInflateFn fn, void* user, uint64_t window_bytes = 0);
/* windows handed to the hook since the last call (0: the hook was not used), and how many of them the host inflated */
void gzip_inflater_counts(uint64_t* windows, uint64_t* refused);

/* multi-member gzip -> the inflated text in anonymous memory (gzip.cpp); nullptr when that does not apply */
char* gunzip_members_to_memory(const std::string& path, int threads, uint64_t max_bytes, uint64_t* size_out, uint64_t* reserved);

}  // namespace fplh
#endif
