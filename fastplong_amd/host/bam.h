/*
 * bam.h -- unaligned BAM (uBAM) input: ONT's basecaller and PacBio's hifi_reads.bam.
 *
 * A BAM is BGZF: gzip members of at most 64 KiB of output, each of which says in its header how long it is (BSIZE) and in its
 * trailer how much it inflates to (ISIZE).  The reader streams the file in windows of blocks, inflates a window's blocks side
 * by side on the worker pool -- or hands the window to an inflater (set_inflater: the device, csrc/bgzf_inflate.h) and inflates
 * only what that refuses -- straight into the batch's (page-locked) record buffer, and walks the records on one thread --
 * about 24 bytes of each: block_size, the name, flag and l_seq.  The bases and qualities are never touched on the host: the
 * device decodes them (fpl_process_bam_async, fastplong_amd/csrc/bam_decode.h).
 *
 * What a record becomes is its `samtools fastq` twin (README "BAM input"): secondary (0x100) and supplementary (0x800) records
 * are skipped; the name line is "@<read_name>", the third line "+".  Errors end the input: a paired record (0x1), a record
 * without qualities (first quality byte 0xFF), a block_size that disagrees with the record's fields, a file cut inside a
 * record, a BGZF block with a bad CRC or size.  A missing EOF block is only a warning.
 */
#ifndef FPLH_BAM_H
#define FPLH_BAM_H

#include <stdint.h>

#include <string>
#include <vector>

#include "batch.h"
#include "fastplong_amd.h"

namespace fplh {

/* gzip magic, a BGZF "BC" extra field, and "BAM\1" at the start of the inflated bytes */
bool is_bam_file(const std::string& path);

/* An inflater the reader may hand its windows to: the C-ABI's fpl_inflate_bgzf with its handle as `user` (the host library does not
 * link the device library; the CLI looks the call up).  comp / blocks / out as for that call; returns 0 when it ran -- blocks[i].status
 * then says which blocks it vouches for (0) --, anything else when it could not. */
typedef int (*BgzfInflateFn)(void* user, const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                             uint64_t out_bytes);

class BamReader {
   public:
    explicit BamReader(const std::string& path);
    ~BamReader();
    BamReader(const BamReader&) = delete;
    BamReader& operator=(const BamReader&) = delete;
    bool ok() const { return fd_ >= 0; }
    /* Append records to b (a BAM-backed batch: b.bam, b.rec_start, b.off, the names; b.seq / b.qual sized for the decoded
       bases) until it holds >= max_bytes of inflated record bytes or max_reads records.  Returns the records appended; 0 at the
       end of the input or at an error (error()).  max_bases: no record is taken once the batch holds that many bases (the
       evaluator's "while (records < READ_LIMIT && bases < BASE_LIMIT)"). */
    uint32_t fill(Batch& b, uint64_t max_bytes, uint32_t max_reads, uint64_t max_bases = ~0ull);
    const std::string& error() const { return err_; }
    const std::string& warning() const { return warn_; } /* "" or the missing-EOF-block warning (set at the end of the input) */
    bool at_end() const { return done_; }
    uint64_t compressed_pulled() const { return comp_end_; } /* file bytes of the blocks inflated so far */
    uint64_t file_size() const { return file_size_; }
    uint64_t records_seen() const { return rec_no_; } /* records walked, skipped ones included */
    /* With an inflater set, a window is everything the batch still takes, read into page-locked memory and handed to fn in one
       call.  Every block fn does not vouch for -- and every block, when fn fails -- is inflated by the host as without an inflater:
       the host's verdict on a block is the verdict, and the error texts are the same.  fn == nullptr: the host path alone. */
    void set_inflater(BgzfInflateFn fn, void* user) {
        if ((fn != nullptr) != (inflate_fn_ != nullptr)) { /* the file bytes in hand lie in the other buffer: read again */
            comp_.clear();
            pin_comp_.clear();
            comp_off_ = comp_end_;
        }
        inflate_fn_ = fn;
        inflate_user_ = user;
    }
    uint64_t blocks_on_device() const { return dev_blocks_; }     /* blocks the inflater vouched for */
    uint64_t blocks_refused() const { return refused_blocks_; }   /* blocks it was given and the host inflated again */
    /* --keep_tags: the walk also walks the auxiliary fields of every record it does not skip (csrc/bam_tag_rules.h); a record
       whose fields do not parse to the end of the record ends the input like every other damaged record */
    void set_check_tags(bool on) { check_tags_ = on; }
    /* the header's text (l_text bytes), known once the first fill has walked the header; "" before */
    const std::string& header_text() const { return header_text_; }
    /* test hook: inflated bytes per window (default 8 MiB; at least one block is always taken) */
    void set_window_bytes(uint64_t w) { window_ = w ? w : 1; }

   private:
    struct Block {
        uint64_t file_off; /* where the block starts in the file */
        uint32_t len;      /* BSIZE + 1 */
        uint32_t isize;
    };
    bool next_blocks(uint64_t want, std::vector<Block>& out); /* the blocks of the next window (false: error) */
    bool read_comp(uint64_t off, uint64_t len);               /* the buffer holds file bytes [comp_off_, comp_off_ + comp_size()) */
    /* the file bytes in hand: comp_, or with an inflater pin_comp_ (page-locked: the inflater's upload reads it in place) */
    const uint8_t* comp_data() const { return inflate_fn_ ? pin_comp_.data() : comp_.data(); }
    uint64_t comp_size() const { return inflate_fn_ ? pin_comp_.size() : comp_.size(); }
    bool walk(Batch& b, uint64_t max_bytes, uint32_t max_reads, uint64_t max_bases, uint32_t& got);
    int fd_ = -1;
    std::string path_, err_, warn_;
    uint64_t file_size_ = 0;
    uint64_t comp_end_ = 0;  /* file offset behind the last block taken */
    uint64_t comp_off_ = 0;  /* file offset of comp_[0] */
    std::vector<uint8_t> comp_;
    std::vector<uint8_t> carry_; /* inflated bytes behind the last whole record of the previous batch */
    uint64_t window_ = 8u << 20;
    uint64_t wpos_ = 0;      /* walk position in the current batch's b.bam */
    uint64_t need_ = 0;      /* bytes from wpos_ the walk needs before it can go on */
    bool header_done_ = false;
    bool check_tags_ = false;
    std::string header_text_;
    bool last_was_eof_block_ = false;
    bool done_ = false;
    uint64_t rec_no_ = 0;
    BgzfInflateFn inflate_fn_ = nullptr;
    void* inflate_user_ = nullptr;
    ByteBuf pin_comp_;                     /* with an inflater: what comp_ is without one, in page-locked memory */
    std::vector<fpl_bgzf_block> dev_desc_; /* its descriptors */
    uint64_t dev_blocks_ = 0, refused_blocks_ = 0;
};

}  // namespace fplh

extern "C" {
int fplh_is_bam(const char* path);
/* test hook: the whole file through BamReader with batches of chunk_bytes / max_reads and windows of window_bytes.  Returns a
   handle (fplh_bam_all_*), NULL when the file cannot be opened; the error and warning texts are in the handle. */
void* fplh_bam_read_all(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes);
/* the same with an inflater (BamReader::set_inflater); fplh_bam_all_device / _refused: the reader's two block counts */
void* fplh_bam_read_all_with(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes, fplh::BgzfInflateFn fn,
                             void* user);
uint64_t fplh_bam_all_device(void* h);
uint64_t fplh_bam_all_refused(void* h);
uint32_t fplh_bam_all_n(void* h);          /* records emitted */
uint32_t fplh_bam_all_batches(void* h);    /* batches they came in */
const uint8_t* fplh_bam_all_bytes(void* h, uint64_t* n); /* each batch's record bytes, back to back */
const uint64_t* fplh_bam_all_rec(void* h);  /* record starts in those bytes */
const uint64_t* fplh_bam_all_off(void* h);  /* n + 1 output offsets */
const char* fplh_bam_all_names(void* h, uint64_t* n); /* the name lines ("@name"), each followed by '\n' */
const char* fplh_bam_all_error(void* h);
const char* fplh_bam_all_warning(void* h);
/* the same reader with set_check_tags(true); fplh_bam_all_header: the header's text as the reader took it */
void* fplh_bam_read_all_tags(const char* path, uint64_t chunk_bytes, uint32_t max_reads, uint64_t window_bytes);
const char* fplh_bam_all_header(void* h, uint64_t* n);
void fplh_bam_all_free(void* h);
}
#endif
