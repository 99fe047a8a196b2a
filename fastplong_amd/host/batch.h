/*
 * batch.h -- the CSR batch the host hands to the device, and the page-locked byte array it is made of.
 */
#ifndef FPLH_BATCH_H
#define FPLH_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fplh {

/* growable byte array without the zero fill of std::vector::resize (batches are hundreds of megabytes and
 * every byte is overwritten by the parser's copy threads).  The memory comes from a process-wide allocator pair the
 * host may replace ONCE, before the first batch exists: the CLI installs fpl_host_alloc / fpl_host_free, so that the
 * CSR arrays are page-locked and the GPU's DMA engines read them in place (no staging copy). */
class ByteBuf {
   public:
    typedef void* (*AllocFn)(size_t);
    typedef void (*FreeFn)(void*);
    static void set_allocator(AllocFn a, FreeFn f);
    /* ... and carve the usual buffers out of ONE allocation of n_blocks x block_bytes made right away (page-locking
       memory is slow and does not scale over threads: 24 parser threads allocating their first batches spent 13 s in
       it for 5 GB); a buffer that needs more than a block, or finds none free, falls back to the allocator */
    static void set_arena(size_t block_bytes, size_t n_blocks);
    static void release_arena(); /* give the arena back (no buffer of it may be used afterwards) */
    ByteBuf() = default;
    ByteBuf(const ByteBuf&) = delete;
    ByteBuf& operator=(const ByteBuf&) = delete;
    ~ByteBuf();
    uint8_t* data() { return p_; }
    const uint8_t* data() const { return p_; }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    void clear() { n_ = 0; }
    const uint8_t* begin() const { return p_; }
    const uint8_t* end() const { return p_ + n_; }
    void reserve(size_t c);
    void resize_uninit(size_t n) {
        reserve(n);
        n_ = n;
    }
   private:
    uint8_t* p_ = nullptr;
    size_t n_ = 0, cap_ = 0;
};

struct Batch {
    ByteBuf seq, qual;                /* CSR payload handed to fpl_process_batch */
    std::vector<uint64_t> off;        /* n + 1 */
    std::vector<char> text;           /* name and strand lines, back to back */
    std::vector<uint64_t> name_off;   /* n + 1 offsets into text for names   */
    std::vector<uint32_t> name_len, strand_len; /* strand line follows the name in `text` */
    /* A TEXT-BACKED batch (--device_parse): `raw` holds a stretch of the file as it lies there, raw[raw_begin, raw_begin +
       raw_len) are whole records; the DEVICE finds them (fpl_process_text_async) and the caller then fills off / name_len /
       strand_len and `line` (four per read: where its name, bases, '+' line and qualities start in raw) from what comes
       back -- no base is copied on the host, the output is formatted out of raw. */
    ByteBuf raw;
    uint64_t raw_begin = 0, raw_len = 0;
    std::vector<uint32_t> line;
    bool text_backed = false;
    /* A BAM-BACKED batch (host/bam.h): `bam` holds inflated BAM records as they lie in the file, rec_start where each read's
       record starts in it; off / names are filled by the host's walk, seq / qual are sized for the bases and receive them from
       the device (fpl_process_bam_async), after which the batch is an ordinary CSR batch. */
    ByteBuf bam;
    std::vector<uint64_t> rec_start;
    bool bam_backed = false;
    uint32_t n() const { return off.empty() ? 0 : (uint32_t)(off.size() - 1); }
    bool has_records() const { return n() > 0 || (text_backed && raw_len > 0); }
    /* the four lines of read i, whichever form the batch has */
    const char* name_ptr(uint32_t i) const { return text_backed ? (const char*)raw.data() + line[4 * (size_t)i] : text.data() + name_off[i]; }
    const char* strand_ptr(uint32_t i) const {
        return text_backed ? (const char*)raw.data() + line[4 * (size_t)i + 2] : text.data() + name_off[i] + name_len[i];
    }
    const uint8_t* seq_ptr(uint32_t i) const { return text_backed ? raw.data() + line[4 * (size_t)i + 1] : seq.data() + off[i]; }
    const uint8_t* qual_ptr(uint32_t i) const { return text_backed ? raw.data() + line[4 * (size_t)i + 3] : qual.data() + off[i]; }
    /* text-backed: off / name_len / strand_len from the line starts the device found (n records, offsets relative to
       raw_begin as fpl_wait_text hands them out) */
    void adopt_lines(const uint32_t* line_starts, uint32_t n_records);
    /* off / name_off of a batch that is about to take CSR records start with 0 */
    void start_offsets() {
        if (off.empty()) {
            off.push_back(0);
            name_off.push_back(0);
        }
    }
    void clear();
};

}  // namespace fplh
#endif
