#include "bam.h"

#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>

#include "gzip.h"
#include "pool.h"
#include "../csrc/bam_rules.h"
#include "../csrc/bam_tag_rules.h"

using namespace std;

namespace fplh {

namespace {

namespace rule = fpl::bamrule; /* the record checks, shared with the device's walk (csrc/bam_walk.h) */

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

/* BSIZE + 1 of the BGZF block header at p (n bytes available, >= 18); 0: not a BGZF block */
uint32_t bgzf_block_len(const uint8_t* p, size_t n) {
    if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
    const uint32_t xlen = rd16(p + 10);
    if (n < 12 + (size_t)xlen) return 0;
    for (uint32_t k = 0; k + 4 <= xlen;) {
        const uint8_t* f = p + 12 + k;
        const uint32_t slen = rd16(f + 2);
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && k + 6 <= xlen) {
            const uint32_t len = rd16(f + 4) + 1;
            return len >= 12 + xlen + 8 ? len : 0;
        }
        k += 4 + slen;
    }
    return 0;
}

/* where the deflate payload of the block starts: behind the member's header -- 10 bytes, the extra field, and, which BGZF does not
   allow but some writers set, a name, a comment, a header CRC (libdeflate skips them too); 0: the header runs into the trailer */
uint32_t bgzf_payload_offset(const uint8_t* blk, uint32_t len) {
    uint32_t hdr = 12 + rd16(blk + 10);
    for (const uint8_t f : {(uint8_t)8, (uint8_t)16})
        if (blk[3] & f) {
            while (hdr < len - 8 && blk[hdr]) hdr++;
            hdr++;
        }
    if (blk[3] & 2) hdr += 2;
    return hdr > len - 8 ? 0 : hdr;
}

/* one BGZF block -> exactly isize bytes at out, its CRC checked (libdeflate checks the trailer itself; zlib: raw inflate + crc32) */
bool inflate_block(const uint8_t* blk, uint32_t len, uint32_t isize, uint8_t* out) {
    size_t used = 0, made = 0;
    const int rc = gunzip_member_into(blk, len, (char*)out, isize, &used, &made);
    if (rc >= 0) return rc == 1 && made == isize && used == len;
    static thread_local z_stream* zs = nullptr;
    if (!zs) {
        zs = new z_stream;
        memset(zs, 0, sizeof(*zs));
        if (inflateInit2(zs, -15) != Z_OK) {
            delete zs;
            zs = nullptr;
            return false;
        }
    } else {
        inflateReset(zs);
    }
    const uint32_t hdr = bgzf_payload_offset(blk, len);
    if (!hdr) return false;
    zs->next_in = (Bytef*)(blk + hdr);
    zs->avail_in = len - hdr - 8;
    uint8_t dummy = 0;
    zs->next_out = isize ? out : &dummy;
    zs->avail_out = isize ? isize : 1;
    if (inflate(zs, Z_FINISH) != Z_STREAM_END || zs->total_out != isize) return false;
    return (uint32_t)crc32(0L, isize ? out : &dummy, isize) == rd32(blk + len - 8);
}

}  // namespace

bool is_bam_file(const string& path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return false;
    /* the first blocks until 4 bytes are inflated (a writer may cut blocks as small as it likes; 16 blocks at most are looked at) */
    vector<uint8_t> buf(65536 + 64), out;
    uint64_t pos = 0;
    for (int k = 0; k < 16 && out.size() < 4; k++) {
        const ssize_t n = pread(fd, buf.data(), buf.size(), (off_t)pos);
        if (n < 18) break;
        const uint32_t len = bgzf_block_len(buf.data(), (size_t)n);
        if (!len || len > (size_t)n) break;
        const uint32_t isize = rd32(buf.data() + len - 4);
        if (isize > 65536) break;
        const size_t at = out.size();
        out.resize(at + isize);
        if (!inflate_block(buf.data(), len, isize, out.data() + at)) break;
        pos += len;
    }
    close(fd);
    return out.size() >= 4 && memcmp(out.data(), "BAM\1", 4) == 0;
}

BamReader::BamReader(const string& path) : path_(path) {
    fd_ = open(path.c_str(), O_RDONLY);
    struct stat st;
    if (fd_ >= 0 && fstat(fd_, &st) == 0) file_size_ = (uint64_t)st.st_size;
}

BamReader::~BamReader() {
    if (fd_ >= 0) close(fd_);
}

bool BamReader::read_comp(uint64_t off, uint64_t len) {
    if (inflate_fn_) { /* the same rule over the page-locked buffer: pread puts the file's bytes where the upload reads them */
        const uint64_t size = pin_comp_.size();
        if (off >= comp_off_ && off + len <= comp_off_ + size) return true;
        uint64_t have = 0;
        if (off >= comp_off_ && off < comp_off_ + size) {
            have = comp_off_ + size - off;
            memmove(pin_comp_.data(), pin_comp_.data() + (off - comp_off_), (size_t)have);
        }
        const uint64_t want = min<uint64_t>(max<uint64_t>(2 * len, 4u << 20), file_size_ - off);
        if (want < len) return false;
        pin_comp_.resize_uninit((size_t)have); /* (a grow copies what the buffer holds) */
        pin_comp_.resize_uninit((size_t)want);
        comp_off_ = off;
        uint64_t got = have;
        while (got < want) {
            const ssize_t r = pread(fd_, pin_comp_.data() + got, (size_t)(want - got), (off_t)(off + got));
            if (r <= 0) {
                pin_comp_.resize_uninit((size_t)got);
                return false;
            }
            got += (uint64_t)r;
        }
        return true;
    }
    if (off >= comp_off_ && off + len <= comp_off_ + comp_.size()) return true;
    /* keep [off, end of what is there), read the rest behind it: at least twice what the window asked for (fewer, larger reads) */
    vector<uint8_t> keep;
    if (off >= comp_off_ && off < comp_off_ + comp_.size()) keep.assign(comp_.begin() + (ptrdiff_t)(off - comp_off_), comp_.end());
    const uint64_t want = min<uint64_t>(max<uint64_t>(2 * len, 4u << 20), file_size_ - off);
    if (want < len) return false;
    comp_.swap(keep);
    const uint64_t have = comp_.size();
    comp_.resize(want);
    comp_off_ = off;
    uint64_t got = have;
    while (got < want) {
        const ssize_t r = pread(fd_, comp_.data() + got, (size_t)(want - got), (off_t)(off + got));
        if (r <= 0) {
            comp_.resize(got);
            return false;
        }
        got += (uint64_t)r;
    }
    return true;
}

bool BamReader::next_blocks(uint64_t want, vector<Block>& out) {
    out.clear();
    uint64_t sum = 0, pos = comp_end_;
    while (pos < file_size_ && (out.empty() || sum < want)) {
        const uint64_t head = min<uint64_t>(18 + 256, file_size_ - pos);
        if (!read_comp(comp_end_, pos + head - comp_end_)) {
            err_ = "reading the BAM input failed: " + path_;
            return false;
        }
        const uint8_t* p = comp_data() + (pos - comp_off_);
        const uint32_t len = bgzf_block_len(p, (size_t)head);
        if (!len) {
            err_ = "BAM input: no BGZF block at file offset " + to_string(pos) + " (damaged or not a BAM file)";
            return false;
        }
        if (pos + len > file_size_) {
            err_ = "BAM input: the BGZF block at file offset " + to_string(pos) + " is cut short (truncated file)";
            return false;
        }
        if (!read_comp(comp_end_, pos + len - comp_end_)) {
            err_ = "reading the BAM input failed: " + path_;
            return false;
        }
        p = comp_data() + (pos - comp_off_);
        const uint32_t isize = rd32(p + len - 4);
        if (isize > 65536) {
            err_ = "BAM input: the BGZF block at file offset " + to_string(pos) + " has a bad size";
            return false;
        }
        out.push_back(Block{pos, len, isize});
        last_was_eof_block_ = len == 28 && isize == 0;
        sum += isize;
        pos += len;
    }
    return true;
}

bool BamReader::walk(Batch& b, uint64_t max_bytes, uint32_t max_reads, uint64_t max_bases, uint32_t& got) {
    const uint8_t* base = b.bam.data();
    const uint64_t size = b.bam.size();
    need_ = 0;
    if (!header_done_) { /* magic, l_text, text, n_ref, n_ref x (l_name, name, l_ref) */
        uint64_t p = 0;
        auto have = [&](uint64_t n) {
            if (p <= size && size - p >= n) return true;
            need_ = p + n - wpos_;
            return false;
        };
        if (!have(8)) return true;
        if (memcmp(base, "BAM\1", 4) != 0) {
            err_ = "BAM input: the inflated stream does not start with BAM\\1";
            return false;
        }
        p = 8 + (uint64_t)rd32(base + 4);
        if (!have(4)) return true;
        const uint32_t n_ref = rd32(base + p);
        p += 4;
        for (uint32_t r = 0; r < n_ref; r++) {
            if (!have(4)) return true;
            p += 4 + (uint64_t)rd32(base + p);
            if (!have(4)) return true;
            p += 4;
        }
        header_done_ = true;
        header_text_.assign((const char*)base + 8, (size_t)rd32(base + 4));
        wpos_ = p;
    }
    for (;;) {
        if (got >= max_reads || (got > 0 && wpos_ >= max_bytes) || b.off.back() >= max_bases) return true;
        const uint64_t avail = size - wpos_;
        if (avail < 4) {
            need_ = 4;
            return true;
        }
        const uint8_t* r = base + wpos_;
        const uint32_t bs = rd32(r);
        auto fail = [&](const string& what, bool with_name) {
            string name;
            if (with_name) {
                const uint32_t ln = r[4 + 8];
                name.assign((const char*)r + 36, strnlen((const char*)r + 36, ln));
            }
            err_ = "BAM record " + to_string(rec_no_) + (with_name ? " (" + name + ")" : string()) + ": " + what;
            return false;
        };
        if (!rule::block_size_ok(bs)) return fail("block_size " + to_string(bs) + " does not agree with its fields", false);
        /* the fixed fields first: a damaged block_size must fail here, not make the reader inflate what it claims (up to 4 GiB) */
        if (avail < 36) {
            need_ = 36;
            return true;
        }
        const rule::Fields f = rule::fields(r);
        const uint32_t l_name = f.l_name, n_cigar = f.n_cigar, flag = f.flag, l_seq = f.l_seq;
        /* (tags may follow the fields, but not more than MAX_TAG_BYTES + 16 bytes for every byte of them) */
        if (!rule::fields_ok(f))
            return fail("block_size " + to_string(bs) + " does not agree with its fields",
                        l_name >= 1 && 32 + (uint64_t)l_name <= bs && avail >= 36 + (uint64_t)l_name);
        if (avail < 4 + (uint64_t)bs) {
            need_ = 4 + (uint64_t)bs;
            return true;
        }
        const uint8_t* name = r + 36;
        const uint8_t* qual = name + l_name + 4 * (size_t)n_cigar + (l_seq + 1) / 2;
        if (rule::skipped(flag)) { /* secondary / supplementary: not part of the twin */
            wpos_ += 4 + (uint64_t)bs;
            rec_no_++;
            continue;
        }
        if (rule::paired(flag)) return fail("flag 0x1 (paired-end) -- fastplong is single-end", true);
        if (rule::no_qualities(f, l_seq ? qual[0] : 0)) return fail("no qualities (the first quality byte is 0xFF)", true);
        if (check_tags_) {
            uint64_t at, len;
            fpl::bamtag::region(r, at, len);
            if (!fpl::bamtag::walk(r + at, len, fpl::bamtag::ByteScan()).whole) return fail("the auxiliary fields do not parse", true);
        }
        const size_t nl = strnlen((const char*)name, l_name - 1);
        const size_t t = b.text.size();
        b.text.resize(t + 1 + nl + 1);
        b.text[t] = '@';
        memcpy(b.text.data() + t + 1, name, nl);
        b.text[t + 1 + nl] = '+';
        b.name_off.push_back(t + 1 + nl + 1);
        b.name_len.push_back((uint32_t)(1 + nl));
        b.strand_len.push_back(1);
        b.rec_start.push_back(wpos_);
        b.off.push_back(b.off.back() + l_seq);
        wpos_ += 4 + (uint64_t)bs;
        rec_no_++;
        got++;
    }
}

uint32_t BamReader::fill(Batch& b, uint64_t max_bytes, uint32_t max_reads, uint64_t max_bases) {
    if (done_ || !err_.empty() || max_reads == 0 || fd_ < 0) return 0;
    b.bam_backed = true;
    if (b.off.empty()) {
        b.off.push_back(0);
        b.name_off.push_back(0);
    }
    if (b.n() > 0) { /* (one BamReader batch at a time: appending to a filled batch is not supported) */
        err_ = "BamReader::fill: the batch is not empty";
        return 0;
    }
    b.bam.clear();
    b.rec_start.clear();
    /* room for the batch up front (a page-locked buffer grows by copying); a caller without a byte bound (the evaluator's prefix:
       max_bytes ~0) starts with one window and grows */
    b.bam.reserve(carry_.size() + (max_bytes < (1ull << 40) ? max_bytes : window_) + (128u << 10));
    b.bam.resize_uninit(carry_.size());
    if (!carry_.empty()) memcpy(b.bam.data(), carry_.data(), carry_.size());
    carry_.clear();
    wpos_ = 0;
    uint32_t got = 0;
    vector<Block> blocks;
    const int threads = max(1, effective_cpus());
    for (;;) {
        if (!walk(b, max_bytes, max_reads, max_bases, got)) return 0;
        if (got >= max_reads || (got > 0 && wpos_ >= max_bytes) || b.off.back() >= max_bases) break;
        const uint64_t size = b.bam.size();
        /* the next window: what the batch still takes (a window at most), and at least what the record in hand needs */
        uint64_t want = min<uint64_t>(window_, max_bytes > size ? max_bytes - size : 1);
        /* with an inflater: everything the batch still takes, so that one call carries as many blocks as the batch allows (a
           caller without a byte bound keeps the window) */
        if (inflate_fn_ && max_bytes < (1ull << 40)) want = max_bytes > size ? max_bytes - size : 1;
        if (need_ > size - wpos_) want = max<uint64_t>(want, need_ - (size - wpos_));
        if (!next_blocks(want, blocks)) return 0;
        if (blocks.empty()) { /* end of the file */
            done_ = true;
            if (size > wpos_ || !header_done_) {
                err_ = header_done_ ? "BAM input: the file ends inside record " + to_string(rec_no_) + " (truncated)"
                                    : string("BAM input: the file ends inside the header (truncated)");
                return 0;
            }
            if (!last_was_eof_block_) warn_ = "WARNING: the BAM input has no BGZF EOF block at its end (truncated file?)";
            break;
        }
        uint64_t add = 0;
        vector<uint64_t> at(blocks.size());
        for (size_t i = 0; i < blocks.size(); i++) {
            at[i] = size + add;
            add += blocks[i].isize;
        }
        b.bam.reserve(size + add);
        b.bam.resize_uninit(size + add);
        uint8_t* dst = b.bam.data();
        const uint8_t* src = comp_data();
        const uint64_t src_off = comp_off_;
        /* the blocks the host inflates: all of them, or with an inflater those it did not vouch for (and the empty ones, which
           need no device but keep the host's check of their bytes) */
        vector<uint32_t> todo;
        bool all = true;
        if (inflate_fn_) {
            const uint64_t w0 = blocks.front().file_off, w1 = blocks.back().file_off + blocks.back().len;
            dev_desc_.clear();
            vector<uint32_t> which;
            for (size_t i = 0; i < blocks.size(); i++) {
                const Block& k = blocks[i];
                const uint32_t hdr = k.isize ? bgzf_payload_offset(src + (k.file_off - src_off), k.len) : 0;
                if (!hdr) {
                    todo.push_back((uint32_t)i);
                    continue;
                }
                const uint8_t* blk = src + (k.file_off - src_off);
                dev_desc_.push_back(fpl_bgzf_block{k.file_off - w0 + hdr, at[i] - size, k.len - hdr - 8, k.isize, rd32(blk + k.len - 8), 1u});
                which.push_back((uint32_t)i);
            }
            const bool ran = dev_desc_.empty() || inflate_fn_(inflate_user_, src + (w0 - src_off), w1 - w0, dev_desc_.data(), (uint32_t)dev_desc_.size(),
                                                              dst + size, add) == 0;
            for (size_t k = 0; k < which.size(); k++) {
                if (ran && dev_desc_[k].status == 0) {
                    dev_blocks_++;
                } else {
                    todo.push_back(which[k]);
                    if (ran) refused_blocks_++;
                }
            }
            all = false;
        }
        const size_t n_todo = all ? blocks.size() : todo.size();
        std::atomic<int64_t> bad{-1};
        const int T = (int)min<size_t>(n_todo, (size_t)threads);
        auto work = [&](int t) {
            for (size_t j = (size_t)t; j < n_todo; j += (size_t)T) {
                const size_t i = all ? j : (size_t)todo[j];
                const Block& k = blocks[i];
                if (!inflate_block(src + (k.file_off - src_off), k.len, k.isize, dst + at[i])) {
                    int64_t cur = bad.load();
                    while ((cur < 0 || (int64_t)k.file_off < cur) && !bad.compare_exchange_weak(cur, (int64_t)k.file_off)) {
                    }
                }
            }
        };
        if (T == 1) work(0);
        else if (T > 1) parallel_run(T, work);
        if (bad.load() >= 0) {
            err_ = "BAM input: the BGZF block at file offset " + to_string(bad.load()) + " has a bad CRC or size";
            return 0;
        }
        comp_end_ = blocks.back().file_off + blocks.back().len;
    }
    carry_.assign(b.bam.data() + wpos_, b.bam.data() + b.bam.size());
    b.bam.resize_uninit(wpos_);
    b.seq.resize_uninit(b.off.back());
    b.qual.resize_uninit(b.off.back());
    return got;
}

}  // namespace fplh

namespace {
struct BamAll {
    vector<uint8_t> bytes;
    vector<uint64_t> rec, off{0};
    string names, err, warn, header;
    uint32_t batches = 0;
    uint64_t on_device = 0, refused = 0;
};
}  // namespace

extern "C" {
int fplh_is_bam(const char* path) { return fplh::is_bam_file(path) ? 1 : 0; }

void* fplh_bam_read_all(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes) {
    return fplh_bam_read_all_with(path, chunk_bytes, max_reads, window_bytes, nullptr, nullptr);
}
uint64_t fplh_bam_all_device(void* h) { return ((BamAll*)h)->on_device; }
uint64_t fplh_bam_all_refused(void* h) { return ((BamAll*)h)->refused; }

static void* bam_read_all(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes, fplh::BgzfInflateFn fn,
                          void* user, bool check_tags) {
    fplh::BamReader rd(path);
    if (!rd.ok()) return nullptr;
    rd.set_inflater(fn, user);
    rd.set_check_tags(check_tags);
    if (window_bytes) rd.set_window_bytes(window_bytes);
    BamAll* a = new BamAll;
    for (;;) {
        fplh::Batch b;
        const uint32_t got = rd.fill(b, chunk_bytes, max_reads ? max_reads : ~0u);
        if (got == 0) break;
        a->batches++;
        const uint64_t base = a->bytes.size();
        a->bytes.insert(a->bytes.end(), b.bam.begin(), b.bam.end());
        for (uint32_t i = 0; i < got; i++) {
            a->rec.push_back(base + b.rec_start[i]);
            a->off.push_back(a->off.back() + (b.off[i + 1] - b.off[i]));
            a->names.append(b.name_ptr(i), b.name_len[i]);
            a->names.push_back('\n');
        }
    }
    a->err = rd.error();
    a->warn = rd.warning();
    a->header = rd.header_text();
    a->on_device = rd.blocks_on_device();
    a->refused = rd.blocks_refused();
    return a;
}
void* fplh_bam_read_all_with(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes, fplh::BgzfInflateFn fn,
                             void* user) {
    return bam_read_all(path, chunk_bytes, max_reads, window_bytes, fn, user, false);
}
void* fplh_bam_read_all_tags(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes) {
    return bam_read_all(path, chunk_bytes, max_reads, window_bytes, nullptr, nullptr, true);
}
const char* fplh_bam_all_header(void* h, uint64_t* n) {
    *n = ((BamAll*)h)->header.size();
    return ((BamAll*)h)->header.data();
}
uint32_t fplh_bam_all_n(void* h) { return (uint32_t)((BamAll*)h)->rec.size(); }
uint32_t fplh_bam_all_batches(void* h) { return ((BamAll*)h)->batches; }
const uint8_t* fplh_bam_all_bytes(void* h, uint64_t* n) {
    *n = ((BamAll*)h)->bytes.size();
    return ((BamAll*)h)->bytes.data();
}
const uint64_t* fplh_bam_all_rec(void* h) { return ((BamAll*)h)->rec.data(); }
const uint64_t* fplh_bam_all_off(void* h) { return ((BamAll*)h)->off.data(); }
const char* fplh_bam_all_names(void* h, uint64_t* n) {
    *n = ((BamAll*)h)->names.size();
    return ((BamAll*)h)->names.data();
}
const char* fplh_bam_all_error(void* h) { return ((BamAll*)h)->err.c_str(); }
const char* fplh_bam_all_warning(void* h) { return ((BamAll*)h)->warn.c_str(); }
void fplh_bam_all_free(void* h) { delete (BamAll*)h; }
}
