#include "gzip.h"

#include <dlfcn.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <iostream>

#include "pool.h"

using namespace std;

namespace fplh {

void error_exit(const string& msg) { /* src/util.h:270-273 */
    cerr << "ERROR: " << msg << endl;
    exit(-1);
}

/* libdeflate, loaded on first use (its API is a handful of C functions; declared here, the image ships the library
   without a header on the default include path) */
namespace {
struct Deflate {
    void* lib = nullptr;
    void* (*alloc_compressor)(int) = nullptr;
    size_t (*gzip_compress)(void*, const void*, size_t, void*, size_t) = nullptr;
    size_t (*gzip_compress_bound)(void*, size_t) = nullptr;
    size_t (*deflate_compress)(void*, const void*, size_t, void*, size_t) = nullptr; /* (raw: bgzf_into; zlib without it) */
    void (*free_compressor)(void*) = nullptr;
    void* (*alloc_decompressor)() = nullptr;
    int (*gzip_decompress_ex)(void*, const void*, size_t, void*, size_t, size_t*, size_t*) = nullptr;
    void (*free_decompressor)(void*) = nullptr;
    Deflate() {
        if (getenv("FPLH_NO_LIBDEFLATE")) return; /* test hook: the zlib paths */
        for (const char* name : {"libdeflate.so.0", "libdeflate.so", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0"}) {
            lib = dlopen(name, RTLD_NOW);
            if (lib) break;
        }
        if (!lib) return;
        alloc_compressor = (decltype(alloc_compressor))dlsym(lib, "libdeflate_alloc_compressor");
        gzip_compress = (decltype(gzip_compress))dlsym(lib, "libdeflate_gzip_compress");
        gzip_compress_bound = (decltype(gzip_compress_bound))dlsym(lib, "libdeflate_gzip_compress_bound");
        deflate_compress = (decltype(deflate_compress))dlsym(lib, "libdeflate_deflate_compress");
        free_compressor = (decltype(free_compressor))dlsym(lib, "libdeflate_free_compressor");
        alloc_decompressor = (decltype(alloc_decompressor))dlsym(lib, "libdeflate_alloc_decompressor");
        gzip_decompress_ex = (decltype(gzip_decompress_ex))dlsym(lib, "libdeflate_gzip_decompress_ex");
        free_decompressor = (decltype(free_decompressor))dlsym(lib, "libdeflate_free_decompressor");
        if (!alloc_compressor || !gzip_compress || !gzip_compress_bound || !free_compressor || !alloc_decompressor ||
            !gzip_decompress_ex || !free_decompressor)
            lib = nullptr;
    }
};
const Deflate& deflate_lib() {
    static const Deflate d;
    return d;
}
/* one compressor / decompressor per thread and level (they are not thread-safe, and allocating one costs more than a
   small member) */
struct ThreadCodec {
    void* comp = nullptr;
    int level = -1;
    void* decomp = nullptr;
    ~ThreadCodec() {
        const Deflate& d = deflate_lib();
        if (comp) d.free_compressor(comp);
        if (decomp) d.free_decompressor(decomp);
    }
};
}  // namespace

bool have_libdeflate() { return deflate_lib().lib != nullptr; }

/* The deflated bytes go through a buffer the calling thread keeps (the pool's workers are persistent): dozens of
   threads allocating and releasing multi-megabyte strings per slice spend their time in the kernel's address-space
   lock instead. */
void gzip_into(const string& in, int level, string& out) {
    static thread_local vector<char> scratch;
    const Deflate& d = deflate_lib();
    if (d.lib) {
        static thread_local ThreadCodec tc;
        if (!tc.comp || tc.level != level) {
            if (tc.comp) d.free_compressor(tc.comp);
            tc.comp = d.alloc_compressor(level);
            tc.level = level;
            if (!tc.comp) error_exit("libdeflate_alloc_compressor failed");
        }
        const size_t bound = d.gzip_compress_bound(tc.comp, in.size());
        if (scratch.size() < bound) scratch.resize(bound);
        const size_t n = d.gzip_compress(tc.comp, in.data(), in.size(), scratch.data(), bound);
        if (n == 0) error_exit("libdeflate_gzip_compress failed");
        out.assign(scratch.data(), n);
        return;
    }
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) error_exit("deflateInit2 failed");
    const size_t bound = deflateBound(&zs, (uLong)in.size()) + 64;
    if (scratch.size() < bound) scratch.resize(bound);
    zs.next_in = (Bytef*)in.data();
    zs.avail_in = (uInt)in.size();
    zs.next_out = (Bytef*)scratch.data();
    zs.avail_out = (uInt)bound;
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) error_exit("deflate failed");
    const size_t n = zs.total_out;
    deflateEnd(&zs);
    out.assign(scratch.data(), n); /* (when out is the input itself: shrinks inside its own allocation) */
}

const string& bgzf_eof() {
    static const string e("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00", 28);
    return e;
}
void bgzf_into(const string& in, int level, string& out) {
    constexpr size_t HEAD = 18, TAIL = 8, MAX_BLOCK = 65536, ROOM = MAX_BLOCK - HEAD - TAIL;
    static thread_local string blocks; /* (the calling thread's, like gzip_into's scratch) */
    blocks.clear();
    const size_t n_pieces = (in.size() + BGZF_PIECE - 1) / BGZF_PIECE;
    blocks.reserve(in.size() / 2 + n_pieces * (HEAD + TAIL + 5) + 64);
    const Deflate& d = deflate_lib();
    const bool use_lib = d.lib && d.deflate_compress;
    static thread_local ThreadCodec tc;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (use_lib) {
        if (!tc.comp || tc.level != level) {
            if (tc.comp) d.free_compressor(tc.comp);
            tc.comp = d.alloc_compressor(level);
            tc.level = level;
            if (!tc.comp) error_exit("libdeflate_alloc_compressor failed");
        }
    } else if (n_pieces && deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) {
        error_exit("deflateInit2 failed");
    }
    unsigned char body[ROOM];
    for (size_t at = 0; at < in.size(); at += BGZF_PIECE) {
        const unsigned char* src = (const unsigned char*)in.data() + at;
        const size_t n = min(BGZF_PIECE, in.size() - at);
        size_t m = 0;
        if (use_lib) {
            m = d.deflate_compress(tc.comp, src, n, body, ROOM); /* (0: it does not fit) */
        } else {
            deflateReset(&zs);
            zs.next_in = (Bytef*)src, zs.avail_in = (uInt)n;
            zs.next_out = body, zs.avail_out = (uInt)ROOM;
            if (deflate(&zs, Z_FINISH) == Z_STREAM_END) m = ROOM - zs.avail_out;
        }
        if (m == 0) { /* one final stored block: 5 + 65 280 bytes always fit */
            body[0] = 1;
            body[1] = (unsigned char)(n & 0xFF), body[2] = (unsigned char)(n >> 8);
            body[3] = (unsigned char)(~n & 0xFF), body[4] = (unsigned char)((~n >> 8) & 0xFF);
            memcpy(body + 5, src, n);
            m = 5 + n;
        }
        const size_t bsize = HEAD + m + TAIL - 1;
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, (uInt)n);
        const unsigned char head[HEAD] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (unsigned char)(bsize & 0xFF), (unsigned char)(bsize >> 8)};
        unsigned char tail[TAIL];
        for (int k = 0; k < 4; k++) tail[k] = (unsigned char)(crc >> (8 * k)), tail[4 + k] = (unsigned char)((uint32_t)n >> (8 * k));
        blocks.append((const char*)head, HEAD);
        blocks.append((const char*)body, m);
        blocks.append((const char*)tail, TAIL);
    }
    if (!use_lib && n_pieces) deflateEnd(&zs);
    out.assign(blocks);
}

int gunzip_member_into(const unsigned char* in, size_t in_len, char* out, size_t out_cap, size_t* consumed, size_t* produced) {
    const Deflate& d = deflate_lib();
    if (!d.lib) return -1;
    static thread_local ThreadCodec tc;
    if (!tc.decomp) tc.decomp = d.alloc_decompressor();
    if (!tc.decomp) return -1;
    size_t used = 0, made = 0;
    const int rc = d.gzip_decompress_ex(tc.decomp, in, in_len, out, out_cap, &used, &made);
    if (rc == 0) {
        if (consumed) *consumed = used;
        if (produced) *produced = made;
        return 1;
    }
    return rc == 3 ? 2 : 0;
}

int gunzip_member(const unsigned char* in, size_t in_len, RawBuf& out, size_t cap, size_t* consumed, size_t hint) {
    const Deflate& d = deflate_lib();
    out.clear();
    if (d.lib) {
        static thread_local ThreadCodec tc;
        if (!tc.decomp) tc.decomp = d.alloc_decompressor();
        if (!tc.decomp) return 0;
        /* the member's own trailer says how long it inflates to (mod 2^32), but where the member ends is what is being
           found out: start from the caller's guess and grow (a wrong guess costs one more pass over the member) */
        /* (untouched pages of a generous buffer cost nothing, a second pass over the member does) */
        size_t guess = min<size_t>(cap, max<size_t>(64u << 20, hint));
        for (;;) {
            out.reserve(guess);
            size_t used = 0, produced = 0;
            const int rc = d.gzip_decompress_ex(tc.decomp, in, in_len, out.p, guess, &used, &produced);
            if (rc == 0) {
                out.n = produced;
                if (consumed) *consumed = used;
                return 1;
            }
            if (rc != 3) { /* bad data / truncated */
                out.release();
                return 0;
            }
            if (guess >= cap) { /* LIBDEFLATE_INSUFFICIENT_SPACE at the cap */
                out.release();
                return 2;
            }
            guess = min(cap, guess * 2);
        }
    }
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return 0;
    zs.next_in = (Bytef*)in;
    size_t in_left = in_len;
    out.reserve(min<size_t>(max<size_t>(4u << 20, hint), cap));
    size_t produced = 0;
    int state = 0;
    for (;;) {
        if (zs.avail_in == 0 && in_left > 0) {
            zs.avail_in = (uInt)min<size_t>(in_left, 1u << 30);
            in_left -= zs.avail_in;
        }
        if (produced == out.cap) {
            if (out.cap >= cap) {
                state = 2;
                break;
            }
            out.reserve(min(cap, out.cap * 2));
        }
        zs.next_out = (Bytef*)out.p + produced;
        zs.avail_out = (uInt)min<size_t>(out.cap - produced, 1u << 30);
        const uInt before = zs.avail_out;
        const int rc = inflate(&zs, Z_NO_FLUSH);
        produced += before - zs.avail_out;
        if (rc == Z_STREAM_END) {
            state = 1;
            if (consumed) *consumed = (size_t)((const unsigned char*)zs.next_in - in);
            break;
        }
        if (rc != Z_OK || (zs.avail_in == 0 && in_left == 0 && zs.avail_out != 0)) break; /* bad data / truncated */
    }
    inflateEnd(&zs);
    if (state == 1) out.n = produced;
    else out.release();
    return state;
}
string gzip_member(const string& in, int level) {
    string o;
    gzip_into(in, level, o);
    return o;
}

MappedFile::MappedFile(const char* path, size_t min_size, bool map) {
    fd = ::open(path, O_RDONLY);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(release_fd());
        return;
    }
    size = (size_t)st.st_size;
    if (!map || !S_ISREG(st.st_mode) || size < min_size || size == 0) return;
    void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m != MAP_FAILED) data = (const unsigned char*)m;
}
MappedFile::~MappedFile() {
    if (data) munmap((void*)data, size);
    if (fd >= 0) close(fd);
}

static uint32_t le32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

/* `span` bytes of anonymous memory for inflated text: address space only, pages are touched as the text arrives; nullptr: none */
static char* map_text(uint64_t span) {
    char* base = (char*)mmap(nullptr, (size_t)span, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) return nullptr;
    madvise(base, (size_t)span, MADV_HUGEPAGE); /* (one fault per 2 MiB instead of per 4 KiB as the text arrives) */
    return base;
}

std::atomic<uint64_t> GzMembers::delivered{0};

GzMembers* GzMembers::open(const string& path, int threads) {
    GzMembers* g = new GzMembers(path, threads);
    if (g->base_) {
        if (const char* e = getenv("FPLH_GZ_MEMBER_CAP")) /* test hook */
            if (atol(e) > 0) g->cap_ = (size_t)atol(e);
        g->find_candidates();
    }
    if (g->cands_.size() < 2 || g->cands_[0] != 0) { /* not to be had, one member (or not gzip): nothing to gain */
        delete g;
        return nullptr;
    }
    return g;
}

GzMembers::~GzMembers() {
    if (stream_) gzclose(stream_);
}

size_t GzMembers::read(char* dst, size_t n) {
    size_t got = 0;
    while (got < n) {
        if (stream_) {
            const int r = gzread(stream_, dst + got, (unsigned)min<size_t>(n - got, 1u << 30));
            if (r <= 0) {
                int errnum = Z_OK;
                gzerror(stream_, &errnum);
                if (r < 0 || (errnum != Z_OK && errnum != Z_STREAM_END)) err_ = errnum == Z_OK ? Z_ERRNO : errnum;
                break;
            }
            got += (size_t)r;
            continue;
        }
        if (cur_off_ < cur_.size()) {
            const size_t k = min(n - got, cur_.size() - cur_off_);
            memcpy(dst + got, cur_.data() + cur_off_, k);
            cur_off_ += k;
            got += k;
            continue;
        }
        if (!next_member()) break;
    }
    return got;
}

void GzMembers::inflate_ahead(bool with_pos) {
    vector<size_t> todo;
    for (auto c = std::lower_bound(cands_.begin(), cands_.end(), pos_); c != cands_.end() && (int)todo.size() < threads_; ++c)
        if (!done_.count(*c)) todo.push_back(*c);
    if (with_pos && (todo.empty() || todo[0] != pos_)) todo.insert(todo.begin(), pos_);
    vector<Result> res(todo.size());
    parallel_run((int)todo.size(), [&](int i) { inflate_at(todo[i], res[i]); });
    for (size_t i = 0; i < todo.size(); i++) done_[todo[i]] = std::move(res[i]);
}

void GzMembers::advance_to(size_t end) {
    for (auto d = done_.begin(); d != done_.end();) /* speculative results the chain has passed */
        d = d->first < end ? done_.erase(d) : std::next(d);
    pos_ = end;
    delivered++;
}

bool GzMembers::next_group(vector<RawBuf>& out, bool* at_end) {
    out.clear();
    *at_end = false;
    if (stream_) return false;
    if (!member_at_pos()) {
        *at_end = true;
        return false;
    }
    inflate_ahead(!done_.count(pos_));
    for (;;) {
        auto it = done_.find(pos_);
        if (it == done_.end()) break;
        if (it->second.state != 1) return !out.empty(); /* (the next call reports the member that cannot be taken) */
        const size_t end = it->second.end;
        out.emplace_back(std::move(it->second.out));
        advance_to(end);
    }
    if (out.empty()) { /* pos_ is there and cannot be taken */
        auto it = done_.find(pos_);
        if (it != done_.end() && it->second.state != 1) return false;
    }
    return !out.empty();
}

void GzMembers::find_candidates() {
    const int T = (int)max<size_t>(1, min<size_t>((size_t)threads_, size_ / (4u << 20)));
    vector<vector<size_t>> found(T);
    parallel_run(T, [&](int t) {
        const size_t lo = size_ / T * t, hi = t == T - 1 ? size_ : size_ / T * (t + 1);
        const unsigned char* p = base_ + lo;
        const unsigned char* e = base_ + min(hi, size_ - 18); /* header 10 + trailer 8 at least */
        while (p < e) {
            p = (const unsigned char*)memchr(p, 0x1f, (size_t)(e - p));
            if (!p) break;
            if (looks_like_header(p)) found[t].push_back((size_t)(p - base_));
            p++;
        }
    });
    for (auto& v : found) cands_.insert(cands_.end(), v.begin(), v.end());
}

void GzMembers::inflate_at(size_t off, Result& r) const { /* (libdeflate when the system has it, else zlib: gunzip_member) */
    size_t used = 0;
    /* a first guess of the inflated size: four times the distance to the next candidate header */
    auto nx = std::upper_bound(cands_.begin(), cands_.end(), off);
    const size_t span = (nx == cands_.end() ? size_ : *nx) - off;
    const int st = gunzip_member(base_ + off, size_ - off, r.out, cap_, &used, span * 4 + (64u << 10));
    r.state = st == 1 ? 1 : (st == 2 ? 2 : -1);
    r.end = off + used;
}

bool GzMembers::next_member() {
    cur_.clear();
    cur_off_ = 0;
    for (;;) {
        if (!member_at_pos()) return false; /* end, or trailing bytes zlib ignores too */
        auto it = done_.find(pos_);
        if (it == done_.end()) { /* inflate the next candidates at and behind pos_ that are not there yet */
            inflate_ahead(true);
            it = done_.find(pos_);
        }
        Result& r = it->second;
        if (r.state == 2 || r.state == -1) {
            /* too large to buffer (or damaged: let zlib report it the usual way): stream the rest */
            done_.clear();
            if (lseek(file_.fd, (off_t)pos_, SEEK_SET) < 0) return false;
            stream_ = gzdopen(file_.fd, "rb");
            if (stream_) {
                file_.release_fd();
                gzbuffer(stream_, 1 << 20);
            } else {
                err_ = Z_ERRNO;
            }
            return stream_ != nullptr;
        }
        cur_.swap(r.out);
        advance_to(r.end);
        if (!cur_.empty()) return true; /* (an empty member: go on to the next) */
    }
}

/* A gzip file made of several members -> its inflated text in anonymous memory, so that the chunk-parallel reader can
 * take it like a mapped file (the members are inflated on `threads` workers and copied into place side by side; address
 * space for `max_bytes` is reserved up front, pages are only touched as the text arrives).  nullptr when the file is not
 * of that kind, a member cannot be buffered or checked, or the text would take more than `max_bytes`: the caller then
 * reads the input through the sequential stream as before.  The caller owns the mapping (`*reserved` bytes). */
/* A gzip file that is ONE member (a plain `gzip` of a whole run): no two workers can share a deflate stream, but libdeflate
 * inflates a whole member 2.3 times faster than zlib streams it, and the text can then be parsed by all the chunk parsers.
 * The member's trailer gives its inflated size modulo 4 GiB; the candidates size, size + 4 GiB, ... are tried in turn (a
 * wrong one fails with "no space" at the end of the output).  nullptr: not a single clean member, no libdeflate, or more
 * text than max_bytes. */
static GzipInflateFn g_gzip_inflate = nullptr;
static void* g_gzip_inflate_user = nullptr;
static uint64_t g_gzip_window = 32ull << 20;
static std::atomic<uint64_t> g_gzip_windows{0}, g_gzip_refused{0};
void set_gzip_inflater(GzipInflateFn fn, void* user, uint64_t window_bytes) {
    g_gzip_inflate = fn;
    g_gzip_inflate_user = user;
    g_gzip_window = window_bytes ? window_bytes : 32ull << 20;
}
void gzip_inflater_counts(uint64_t* windows, uint64_t* refused) {
    *windows = g_gzip_windows.exchange(0);
    *refused = g_gzip_refused.exchange(0);
}

/* where the deflate payload of the gzip member at in[0 .. n) starts (RFC 1952: FEXTRA, FNAME, FCOMMENT, FHCRC); 0: no such header */
static size_t gzip_payload_start(const unsigned char* in, size_t n) {
    if (n < 18 || in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || (in[3] & 0xE0)) return 0;
    const unsigned flg = in[3];
    size_t p = 10;
    if (flg & 4) {
        if (p + 2 > n) return 0;
        p += 2 + ((size_t)in[p] | ((size_t)in[p + 1] << 8));
    }
    for (unsigned bit : {8u, 16u})
        if (flg & bit) {
            while (p < n && in[p]) p++;
            p++;
        }
    if (flg & 2) p += 2;
    return p + 8 <= n ? p : 0;
}

/* zlib from bit `bit` of the payload in[0 .. n) to the end of the stream, text_made bytes of text in front of out (the last 32 KiB
   of them are the dictionary); true: the final block ended, *end_byte is the byte behind it and *made the bytes written */
static bool inflate_rest_on_host(const unsigned char* in, size_t n, uint64_t bit, char* text, uint64_t text_made, uint64_t cap, size_t* end_byte,
                                 uint64_t* made) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    size_t at = (size_t)(bit >> 3);
    bool ok = at < n;
    if (ok && (bit & 7)) {
        ok = inflatePrime(&zs, 8 - (int)(bit & 7), in[at] >> (bit & 7)) == Z_OK;
        at++;
    }
    const uint64_t dl = std::min<uint64_t>(text_made, 32768);
    if (ok && dl) ok = inflateSetDictionary(&zs, (const Bytef*)(text + text_made - dl), (uInt)dl) == Z_OK;
    uint64_t done = 0;
    int rc = Z_OK;
    while (ok && rc != Z_STREAM_END) {
        if (zs.avail_in == 0) {
            zs.next_in = (Bytef*)(in + at);
            zs.avail_in = (uInt)std::min<size_t>(n - at, 1u << 30);
            at += zs.avail_in;
        }
        zs.next_out = (Bytef*)(text + text_made + done);
        const uInt room = (uInt)std::min<uint64_t>(cap - done, 1u << 30);
        zs.avail_out = room;
        const uInt fed = zs.avail_in;
        rc = inflate(&zs, Z_NO_FLUSH);
        done += room - zs.avail_out;
        if (rc != Z_OK && rc != Z_STREAM_END) ok = false;
        else if (rc == Z_OK && fed == zs.avail_in && room == zs.avail_out && (fed == 0 || room == 0)) ok = false; /* out of input or of room */
    }
    if (ok) {
        *end_byte = at - zs.avail_in;
        *made = done;
    }
    inflateEnd(&zs);
    return ok;
}

/* The member at in[0 .. fsize) through the hook into text[0 .. want); true: `want` bytes whose CRC-32 and size are the trailer's,
   *used the byte behind the trailer. */
static bool gunzip_member_on_device(const unsigned char* in, size_t fsize, char* text, uint64_t want, size_t* used) {
    const size_t p0 = gzip_payload_start(in, fsize);
    if (!p0) return false;
    const unsigned char* pay = in + p0;
    const size_t pn = fsize - p0;
    uint64_t bit = 0, made = 0;
    uLong crc = crc32(0L, Z_NULL, 0);
    size_t end_byte = 0;
    bool final_seen = false;
    while (!final_seen) {
        const size_t at = (size_t)(bit >> 3);
        if (at >= pn) return false;
        const size_t wlen = (size_t)std::min<uint64_t>(pn - at, g_gzip_window);
        const uint64_t dl = std::min<uint64_t>(made, 32768);
        fpl_gzip_window r;
        memset(&r, 0, sizeof(r));
        g_gzip_windows++;
        const int rc = g_gzip_inflate(g_gzip_inflate_user, pay + at, wlen, bit & 7, dl ? (const uint8_t*)text + made - dl : nullptr, (uint32_t)dl,
                                      (uint8_t*)text + made, want - made, 0, &r);
        const bool taken = rc == 0 && r.status == FPL_GZIP_OK && r.out_bytes <= want - made && r.end_bit > (bit & 7) && r.end_bit <= 8 * (uint64_t)wlen &&
                           (r.final_block || wlen == pn - at || (r.end_bit >> 3) * 16 >= wlen); /* (it got somewhere) */
        if (!taken) {
            g_gzip_refused++;
            uint64_t rest = 0;
            if (!inflate_rest_on_host(pay, pn, bit, text, made, want - made, &end_byte, &rest)) return false;
            for (uint64_t k = 0; k < rest; k += 1u << 30)
                crc = crc32(crc, (const Bytef*)text + made + k, (uInt)std::min<uint64_t>(rest - k, 1u << 30));
            made += rest;
            break;
        }
        crc = crc32_combine(crc, r.crc32, (z_off_t)r.out_bytes);
        made += r.out_bytes;
        bit = 8 * (uint64_t)at + r.end_bit;
        if (r.final_block) {
            final_seen = true;
            end_byte = (size_t)((bit + 7) >> 3);
        }
    }
    if (end_byte + 8 > pn || made != want) return false;
    const unsigned char* t = pay + end_byte;
    if (le32(t) != (uint32_t)crc || le32(t + 4) != (uint32_t)made) return false;
    *used = p0 + end_byte + 8;
    return true;
}

static char* gunzip_single_to_memory(const string& path, uint64_t max_bytes, uint64_t* size_out, uint64_t* reserved) {
    const MappedFile file(path.c_str(), 18);
    if (!file.data) return nullptr;
    const unsigned char* in = file.data;
    const size_t fsize = file.size;
    char* result = nullptr;
    if (in[0] == 0x1f && in[1] == 0x8b && in[2] == 8) {
        /* where the member ends: at the end of the file -- or, when zero bytes trail it (zlib ignores padding behind the last
           member: so does this), 0..3 bytes behind the last non-zero byte (the size field itself may end in zero bytes).  The
           likeliest end is tried first -- the file's own when fewer than four zero bytes trail it, else the last non-zero
           byte's (a size field whose top byte is zero means a text within 16 MiB of a multiple of 4 GiB) -- and a member that
           is followed by another one ends the attempt */
        size_t tail = fsize;
        while (tail > 18 && in[tail - 1] == 0 && (fsize < 4096 || tail > fsize - 4096)) tail--;
        size_t ends[5];
        int n_ends = 0;
        const bool padded = fsize - tail >= 4; /* four zero bytes at the very end: padding, or a text of k * 4 GiB */
        if (!padded) ends[n_ends++] = fsize;
        for (int pad = 0; pad < 4 && tail < fsize; pad++)
            if (tail + (size_t)pad < fsize) ends[n_ends++] = tail + (size_t)pad;
        if (padded) ends[n_ends++] = fsize;
        /* The candidate ends only say how much text to make room for (the size field in front of them).  The inflate itself
           always gets the whole file: it stops where the member really ends (`used`, trailer checked) -- so a member with
           padding behind it is accepted from the FIRST attempt that had room for its text, instead of being inflated again for
           every guess of where the padding starts.  At most four attempts in all: every one is a full pass over the file. */
        uint64_t wants[12];
        int n_wants = 0;
        for (int e = 0; e < n_ends; e++) {
            const size_t end = ends[e];
            if (end < 18) continue;
            const uint64_t isize = le32(in + end - 4);
            for (uint64_t want = isize; want <= max_bytes && n_wants < 12; want += 1ull << 32) {
                bool seen = want == 0;
                for (int k = 0; k < n_wants; k++) seen = seen || wants[k] == want;
                if (!seen) wants[n_wants++] = want;
                if (want - isize >= (1ull << 32)) break; /* (one wrap per candidate: a text beyond 8 GiB of a guess is the next guess's) */
            }
        }
        int attempts = 0;
        for (int k = 0; k < n_wants && !result && attempts < 4; k++) {
            const uint64_t want = wants[k];
            const uint64_t span = want + (4u << 20);
            char* base = map_text(span);
            if (!base) break;
            size_t used = 0, made = 0;
            attempts++;
            /* --device_inflate: the first guess through the hook; whatever it does not carry to a trailer that agrees is done again
               below, as without it */
            int rc = 0;
            if (g_gzip_inflate && k == 0 && gunzip_member_on_device(in, fsize, base, want, &used)) {
                rc = 1;
                made = (size_t)want;
            } else {
                rc = gunzip_member_into(in, fsize, base, (size_t)want, &used, &made);
            }
            if (rc == 1 && made > 0) {
                /* a whole member.  Zero padding may follow (zlib ignores it: so does this); anything else is another member --
                   not for this lane */
                size_t z = used;
                while (z < fsize && in[z] == 0) z++;
                if (z == fsize) {
                    result = base;
                    *size_out = made;
                    *reserved = span;
                    break;
                }
                munmap(base, (size_t)span);
                break;
            }
            munmap(base, (size_t)span);
            if (rc != 2) break; /* damaged, or no libdeflate: the streaming reader reports it / takes over */
            /* rc == 2: more text than this guess made room for: the next one */
        }
    }
    return result;
}

char* gunzip_members_to_memory(const string& path, int threads, uint64_t max_bytes, uint64_t* size_out, uint64_t* reserved) {
    /* The size field at the end of the file belongs to its LAST member.  When it says "at least as much text as the whole file
       has bytes", the file is almost certainly one member: that lane first (bytes that look like a member header inside the
       compressed data would otherwise send it through the member chain, whose size guesses for a member this large cost
       several passes).  Otherwise the chain first, the single-member lane if the chain finds only one. */
    bool single_first = false;
    {
        const MappedFile file(path.c_str(), 18);
        if (file.data) single_first = le32(file.data + file.size - 4) >= file.size;
    }
    if (single_first)
        if (char* one = gunzip_single_to_memory(path, max_bytes, size_out, reserved)) return one;
    GzMembers* g = GzMembers::open(path, threads);
    if (!g) return single_first ? nullptr : gunzip_single_to_memory(path, max_bytes, size_out, reserved);
    const uint64_t span = max_bytes + (4u << 20);
    char* base = map_text(span);
    if (!base) {
        delete g;
        return nullptr;
    }
    uint64_t total = 0;
    bool ok = true, at_end = false;
    vector<RawBuf> group;
    while (ok && g->next_group(group, &at_end)) {
        vector<uint64_t> at(group.size());
        for (size_t i = 0; i < group.size(); i++) {
            at[i] = total;
            total += group[i].n;
        }
        if (total > max_bytes) {
            ok = false;
            break;
        }
        parallel_run((int)group.size(), [&](int i) {
            memcpy(base + at[i], group[i].p, group[i].n);
            group[i].release();
        });
    }
    if (!at_end || g->error()) ok = false;
    delete g;
    if (!ok || total == 0) {
        munmap(base, (size_t)span);
        return nullptr;
    }
    *size_out = total;
    *reserved = span;
    return base;
}

}  // namespace fplh
