/*
 * fastplong_amd.h -- C-ABI of the MI355X-native per-read hot path.
 *
 * The reference (OpenGene/fastplong v0.4.1) has no plugin/FFI interface; the seam this
 * library replaces is the C++ call
 *     bool SingleEndProcessor::processSingleEnd(ReadPack*, ThreadConfig*)
 *         (reference src/seprocessor.h:30, body src/seprocessor.cpp:180-329)
 * together with the per-thread accumulators it updates (Stats x2 + FilterResult,
 * src/threadconfig.h:16-59) and the serial merge that follows the join
 * (Stats::merge src/stats.cpp:1013-1082, FilterResult::merge src/filterresult.cpp:28-61).
 *
 * Shape of the replacement: the caller hands over a *batch* of variable-length reads in CSR
 * form (all bases concatenated, all quality bytes concatenated, n+1 byte offsets) and gets
 * back one fixed-size record per read (bounds of the surviving fragment(s) + filter code)
 * while all additive counters stay resident on the device until fpl_get_counters().
 * Bases are never written back: the host slices its own copy using the returned offsets.
 *
 * Conventions: plain C types only; the caller owns every buffer it passes in; functions
 * return 0 or a negative FPL_ERR_* code and never call exit(); one context per device, one
 * batch in flight per context; contexts on different devices may be driven from different
 * threads.  There is no CPU fallback: fpl_create() fails with FPL_ERR_NO_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef FASTPLONG_AMD_H
#define FASTPLONG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPL_ABI_VERSION 10

/* limits */
#define FPL_MAX_ADAPTER_LEN 255 /* longest adapter the device path accepts            */
#define FPL_MAX_ADAPTERS 1024   /* start + end + FASTA adapters                      */
#define FPL_END_WINDOW 200      /* WINDOW,      reference src/adaptertrimmer.cpp:169,239 */
#define FPL_PATTERN_LEN 16      /* PATTERN_LEN, reference src/adaptertrimmer.cpp:170,240 */

/* filter result codes, reference src/common.h:43-50 */
#define FPL_PASS_FILTER 0
#define FPL_FAIL_N_BASE 12
#define FPL_FAIL_LENGTH 16
#define FPL_FAIL_TOO_LONG 17
#define FPL_FAIL_QUALITY 20
#define FPL_FAIL_COMPLEXITY 24
#define FPL_FILTER_RESULT_TYPES 32

/* error codes */
#define FPL_OK 0
#define FPL_ERR_ARG (-1)       /* null pointer / inconsistent argument                  */
#define FPL_ERR_NO_DEVICE (-2) /* no usable HIP device: this library has no CPU path    */
#define FPL_ERR_HIP (-3)       /* a HIP runtime call failed (see fpl_last_error)        */
#define FPL_ERR_ADAPTER (-4)   /* adapter longer than FPL_MAX_ADAPTER_LEN / too many    */
#define FPL_ERR_CAPACITY (-5)  /* read longer than the context's max_cycles capacity    */
#define FPL_ERR_STATE (-6)     /* call not valid in the current state                   */

/*
 * Options the path reads.  Field-for-field mirror of the parts of the reference's `Options`
 * that processSingleEnd and its callees consult (src/options.h:56-184); defaults in
 * fpl_options_default() are the reference CLI defaults (src/main.cpp:27-103).
 */
typedef struct fpl_options {
    /* TrimmingOptions, src/options.h:149-161: -f / -t */
    int32_t trim_front;
    int32_t trim_tail;
    /* QualityCutOptions, src/options.h:69-98: --cut_front/--cut_tail and their windows */
    int32_t cut_front;        /* enabledFront */
    int32_t cut_tail;         /* enabledTail  */
    int32_t cut_front_window; /* windowSizeFront 1..1000 */
    int32_t cut_front_quality; /* qualityFront, phred (not +33) */
    int32_t cut_tail_window;
    int32_t cut_tail_quality;
    /* PolyXTrimmerOptions, src/options.h:57-66: -x / --poly_x_min_len */
    int32_t polyx;
    int32_t polyx_min_len;
    /* AdapterOptions, src/options.h:126-147: -A, -d, --trimming_extension */
    int32_t adapter_enabled;
    double ed_max;            /* distance_threshold: round(ed_max*len) is done in double on the host */
    int32_t trimming_extension;
    /* QualityFilteringOptions, src/options.h:163-184: -Q -q -u -n --n_base_limit -m */
    int32_t qual_filter;      /* enabled */
    int32_t qualified_qual;   /* qualifiedQual as the raw ASCII char (phred+33), '0' = Q15 */
    int32_t unqualified_percent_limit;
    int32_t n_base_limit;     /* 1000000 means "no limit" (src/filter.cpp:46) */
    int32_t n_base_percent_limit;
    int32_t avg_qual_req;     /* -m, 0 = off */
    /* ReadLengthFilteringOptions, src/options.h:186-200: -L -l --length_limit */
    int32_t length_filter;    /* enabled */
    int32_t required_length;
    int32_t max_length;       /* 0 = no limit */
    /* LowComplexityFilterOptions, src/options.h:43-53: -y -Y (integer percent 0..100;
       the reference stores percent/100.0 and compares doubles -- equivalent) */
    int32_t complexity_filter;
    int32_t complexity_percent;
    /* LowQualityBreakOptions / MaskOptions, src/options.h:20-44: -b --break_window_size --break_mean_quality,
       -N --mask_window_size --mask_mean_quality (src/main.cpp:65-73,207-215); qualities are phred (not +33).
       With either enabled the per-read record cannot hold the outcome any more: see fpl_fragment. */
    int32_t break_enabled;
    int32_t break_window;
    int32_t break_quality;
    int32_t mask_enabled;
    int32_t mask_window;
    int32_t mask_quality;
} fpl_options;

typedef struct fpl_adapter {
    const char* seq; /* raw bytes, not NUL-terminated */
    int32_t len;
} fpl_adapter;

/*
 * One record per input read, written in input order.  Everything a writer needs to do what
 * src/seprocessor.cpp:265-281 does (serialize passing fragments; tag failed reads) without
 * touching the bases again.  All positions are byte offsets relative to the start of the
 * ORIGINAL read.  36 bytes.
 *
 *  dropped = 1 : Filter::trimAndCut returned NULL (src/filter.cpp:137-139,165,197,221): the
 *                read is counted in the pre-filter statistics and nowhere else.
 *  r1_start/r1_len : the read after trimAndCut + polyX + adapter end trims ("r1"); this is
 *                what --failed_out receives when exactly one fragment exists and it fails.
 *  n_frag 0..2 : fragments after the middle-adapter split (Read::breakByGap,
 *                src/read.cpp:192-215); kind 0 = unsplit r1, 1 = "split-by-adapter-left-",
 *                2 = "split-by-adapter-right-".
 *  code[i]     : Filter::passFilter result for fragment i (FPL_PASS_FILTER / FPL_FAIL_*).
 *  median_q_pre: per-read median quality char of the original read (Stats::statRead,
 *                src/stats.cpp:352-363); 0 when the read is empty.
 *  median_q_post[i]: same for fragment i, valid only when code[i] == FPL_PASS_FILTER.
 */
typedef struct fpl_read_result {
    uint32_t r1_start;
    uint32_t r1_len;
    uint32_t frag_start[2];
    uint32_t frag_len[2];
    uint8_t n_frag;
    uint8_t dropped;
    uint8_t code[2];
    uint8_t kind[2];
    uint8_t median_q_pre;
    uint8_t median_q_post[2];
    uint8_t reserved[3];
} fpl_read_result;

/*
 * --break / --mask (src/seprocessor.cpp:234-262) turn a read into any number of output reads, some of whose
 * bases are replaced by N.  When fpl_options.break_enabled or mask_enabled is set, fpl_read_result keeps
 * r1_start / r1_len / dropped / median_q_pre, n_frag saturates at 255 and its fragment fields are zero;
 * the fragments come as a list of these records (fpl_fragment_counts / fpl_get_fragments after each batch),
 * sorted by (read, seq_no) = the order the reference writes them.  32 bytes.
 *
 *  start/len    : window on the ORIGINAL read.
 *  kind         : 0 r1 itself or cut from r1, 1 / 2 the left / right part of a middle-adapter split.
 *  break_no     : 0 = not a product of Read::breakByRegions; i >= 1: that function named it by inserting
 *                 "r<i>-" after the first character of the (possibly split-prefixed) name (src/read.cpp:244,256).
 *  region_first/count : slice of the fpl_region list: stretches of the fragment that Read::maskRegionWithN
 *                 overwrote with 'N' (original-read coordinates, ascending, disjoint).
 *  code         : Filter::passFilter of the fragment (after masking); median_q valid when code == FPL_PASS_FILTER.
 * The reference writes --failed_out only for a read with exactly one fragment that fails; it then prints r1,
 * masked only if that fragment IS r1 (kind == 0 and break_no == 0: masking was done in place).
 */
typedef struct fpl_fragment {
    uint32_t read;
    uint32_t seq_no;
    uint32_t start;
    uint32_t len;
    uint32_t region_first;
    uint32_t region_count;
    uint16_t break_no;
    uint8_t code;
    uint8_t kind;
    uint8_t median_q;
    uint8_t reserved[3];
} fpl_fragment;

typedef struct fpl_region {
    uint32_t start;
    uint32_t len;
} fpl_region;

/*
 * Flat int64 counter buffer ("what the RCCL all-reduce sums").  C = max_cycles capacity.
 *
 *   [ pre-filter Stats | post-filter Stats | FilterResult | adapter-key histogram ]
 *
 * One Stats block (FPL_STATS_LEN(C) entries), replacing the members of the reference's
 * class Stats that statRead updates (src/stats.h:70-110):
 *   cyc[c][kind*8 + cls], c < C, cycle-major so that growing C appends:
 *        kind 0 mCycleBaseContents, 1 mCycleBaseQual, 2 mCycleQ20Bases, 3 mCycleQ30Bases,
 *        cls = base ASCII & 7 (A1 C3 T4 U5 N6 G7, src/stats.h:60-69);
 *        mCycleTotalBase / mCycleTotalQual are the sums over cls and are not stored.
 *   base_qual_hist[128]   mBaseQualHistogram
 *   median_hist[128]      mMedianReadQualHistogram
 *   median_bases[128]     mMedianReadQualBases
 *   kmer[1024]            mKmer (the reference allocates 2048, indices are 10 bit)
 *   reads, length_sum     mReads, mLengthSum
 *
 * FilterResult block (FPL_FR_LEN entries), src/filterresult.h:57-64:
 *   filter_read_stats[32], adapter_trimmed_reads, adapter_trimmed_bases,
 *   polyx_reads[4], polyx_bases[4]      (A,T,C,G order of ATCG_BASES, src/common.h:26)
 *
 * Adapter-key histogram: key_hist[a][side][cmplen], a < n_adapters, side 0 = trimmed at
 * read start (key = adapter.substr(alen-cmplen, cmplen)), side 1 = trimmed at read end
 * (key = adapter.substr(0, cmplen)), cmplen <= FPL_MAX_ADAPTER_LEN; cmplen == alen is the
 * full adapter.  The host turns indices into the strings of the reference's
 * map<string,long> mAdapter (src/filterresult.cpp:68-76).
 * Adapter slot order: 0 = start adapter, 1 = end adapter, 2.. = FASTA adapters in the order
 * given (the caller sorts them by FASTA header like src/options.cpp:50-59).
 */
#define FPL_CYC_STRIDE 32
#define FPL_STATS_TAIL (128 * 3 + 1024 + 2)
#define FPL_STATS_LEN(C) ((size_t)(C) * FPL_CYC_STRIDE + FPL_STATS_TAIL)
#define FPL_ST_CYC(c, kind, cls) ((size_t)(c) * FPL_CYC_STRIDE + (size_t)(kind) * 8 + (size_t)(cls))
#define FPL_ST_BASE_QUAL_HIST(C) ((size_t)(C) * FPL_CYC_STRIDE)
#define FPL_ST_MEDIAN_HIST(C) (FPL_ST_BASE_QUAL_HIST(C) + 128)
#define FPL_ST_MEDIAN_BASES(C) (FPL_ST_BASE_QUAL_HIST(C) + 256)
#define FPL_ST_KMER(C) (FPL_ST_BASE_QUAL_HIST(C) + 384)
#define FPL_ST_READS(C) (FPL_ST_BASE_QUAL_HIST(C) + 384 + 1024)
#define FPL_ST_LENGTH_SUM(C) (FPL_ST_READS(C) + 1)
#define FPL_FR_LEN 42
#define FPL_FR_FILTER 0
#define FPL_FR_ADAPTER_READS 32
#define FPL_FR_ADAPTER_BASES 33
#define FPL_FR_POLYX_READS 34
#define FPL_FR_POLYX_BASES 38
#define FPL_KEY_STRIDE (FPL_MAX_ADAPTER_LEN + 1)
#define FPL_KEYHIST_LEN(nad) ((size_t)(nad) * 2 * FPL_KEY_STRIDE)
#define FPL_COUNTERS_LEN(C, nad) (2 * FPL_STATS_LEN(C) + FPL_FR_LEN + FPL_KEYHIST_LEN(nad))
#define FPL_OFF_PRE(C) ((size_t)0)
#define FPL_OFF_POST(C) (FPL_STATS_LEN(C))
#define FPL_OFF_FR(C) (2 * FPL_STATS_LEN(C))
#define FPL_OFF_KEYHIST(C) (2 * FPL_STATS_LEN(C) + FPL_FR_LEN)

typedef struct fpl_ctx fpl_ctx;

/* Reference CLI defaults (src/main.cpp:27-103, src/options.h ctors). */
void fpl_options_default(fpl_options* opt);

/*
 * Create a context on HIP device `device` (>= 0).
 *  start/end  : adapter strings of --start_adapter / --end_adapter after the CLI resolved
 *               them (src/main.cpp:131-140); len 0 = empty string.
 *  fasta      : sequences of --adapter_fasta in the order trimByMultiSequences must visit
 *               them (src/adaptertrimmer.cpp:42-57); n_fasta = 0 means hasFasta = false.
 *  max_cycles : initial capacity C of the per-cycle tables (grown on demand).
 */
int fpl_create(fpl_ctx** out, const fpl_options* opt, const char* start_adapter, int32_t start_len,
               const char* end_adapter, int32_t end_len, const fpl_adapter* fasta, int32_t n_fasta,
               int32_t device, uint32_t max_cycles);
void fpl_destroy(fpl_ctx* ctx);

/*
 * Process one batch whose buffers already live in device memory (HBM).
 *  d_seq, d_qual : n_bytes bytes each; read i occupies [d_off[i], d_off[i+1]).
 *  d_off         : n_reads + 1 uint64 offsets, non-decreasing, d_off[n_reads] <= n_bytes.
 *  max_read_len  : upper bound of the read lengths in the batch (the caller knows it from
 *                  its offsets); used to size the launch and to check capacity.
 *  d_results     : n_reads records, device memory.
 *  stream        : hipStream_t (NULL = default stream).  Asynchronous: returns after the
 *                  launches are enqueued.
 */
int fpl_process_batch_device(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual,
                             const uint64_t* d_off, uint32_t n_reads, uint64_t n_bytes,
                             uint32_t max_read_len, fpl_read_result* d_results, void* stream);

/*
 * Same, from host buffers (pinned recommended): copies in, processes, copies the records
 * back and synchronizes.  This is the call a host worker loop makes in place of
 * processSingleEnd().
 */
int fpl_process_batch(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off,
                      uint32_t n_reads, fpl_read_result* results);

/*
 * The same without the wait: the pipelined form a host thread uses to keep the PCIe link and the
 * kernels busy together (what the reference gets from its producer/consumer queues,
 * src/seprocessor.cpp:331-485).  fpl_process_batch_async() enqueues H2D copies on a copy stream,
 * the kernels on the context's compute stream behind them, the D2H of the records on a third
 * stream, and returns; fpl_wait() blocks until the OLDEST batch in flight is complete and its
 * records are in the `results` array given at submission.  Up to FPL_MAX_IN_FLIGHT batches may be
 * in flight per context (one set of device staging buffers per batch in flight): the copies of batch k+1 overlap
 * the kernels of batch k.  seq / qual / off must stay valid until the batch has been waited for;
 * they should come from fpl_host_alloc() (pinned) -- pageable memory works but the runtime then
 * stages the copy on the calling thread.  With break_enabled / mask_enabled, a submission first
 * drains the batch in flight (its fragment list lives in buffers the next batch reuses), and
 * fpl_get_fragments() refers to the batch most recently waited for.
 * Errors of the asynchronous part are reported by fpl_wait().
 */
#define FPL_MAX_IN_FLIGHT 3
int fpl_process_batch_async(fpl_ctx* ctx, const uint8_t* seq, const uint8_t* qual, const uint64_t* off,
                            uint32_t n_reads, fpl_read_result* results);
int fpl_wait(fpl_ctx* ctx);
int fpl_in_flight(const fpl_ctx* ctx);

/*
 * (ABI v7) The reader's work on the device: FASTQ TEXT in, records out.  Replaces, for the per-read path, what
 * FastqReader::read / ::getLine do per record on the reference's reader thread (src/fastqreader.cpp:219-347): the host
 * hands over a chunk of the file's bytes as they lie there -- it must start at the '@' of a record and end behind the line
 * break of a record's quality line, nothing else is asked of it -- and the device finds the line breaks, checks every record
 * the way FastqReader::read does ('@', '+', as many qualities as bases, :312-341), lays bases and qualities out as the
 * CSR batch the kernels take and runs the batch.  No base is copied on the host: the link carries the same 2.02 bytes per
 * base as with fpl_process_batch_async.
 *
 *   fpl_process_text_async  uploads `text` (page-locked memory recommended) and starts the parse; returns at once.  `text`
 *                           must stay valid until the batch has been waited for.  Shares the FPL_MAX_IN_FLIGHT slots and the
 *                           FIFO order of fpl_process_batch_async.
 *   fpl_peek_text           the parse's verdict for the NEXT PENDING text batch -- the oldest one in flight that has been neither
 *                           started nor cancelled -- as soon as it is in: the upload and the parse kernels, not the per-read
 *                           kernels, so a batch that has only been peeked at is in no counter yet.  Fills *out like fpl_wait_text.
 *   fpl_start_text          enqueues the per-read kernels of the next pending text batch (waits for its parse, not for them).
 *                           Optional: fpl_wait_text starts a batch that was not.  A host that starts batch k + 1 before it waits
 *                           for batch k keeps the device's queue filled while it sits in the wait.
 *   fpl_cancel_text         the next pending text batch will not run; its fpl_wait_text reports FPL_TEXT_CANCELLED.
 *                           Together: a host with several devices publishes every chunk's verdict and lets a chunk run only when
 *                           all chunks in front of it were good -- the reference stops READING at a malformed record
 *                           (src/fastqreader.cpp:326-341), so nothing behind one may be counted (bin/fastplong_amd does this).
 *   fpl_wait_text           blocks until the OLDEST batch in flight (which must be a text batch) is complete.  *out says what
 *                           the chunk held; results[i] is the record of read i and line_starts[4 i + j] the offset, in
 *                           `text`, of line j of record i (0 name, 1 bases, 2 '+', 3 qualities) -- so the caller formats its
 *                           output from the text it still holds.  Both arrays are the library's (page-locked) and stay valid
 *                           until the next submission that takes this batch's slot (the FPL_MAX_IN_FLIGHT-th submission after
 *                           the one that made this batch).
 *
 * status FPL_TEXT_IRREGULAR: the chunk is not "four lines per record, every line ended by \n or \r\n, '@' and '+' in place,
 * equal lengths" (blank lines, a lone \r, a missing final line break, a malformed record: bad_record is the first) -- NOTHING
 * of it was processed or counted; the caller parses the chunk with its own reader (the reference's rules for such text are
 * the sequential reader's: skipped lines, the error texts of :326-341) and submits it through fpl_process_batch_async.
 * FPL_TEXT_TOO_MANY: more than n_bytes / 64 + 16 records (reads shorter than 30 bases on average): same treatment.
 * A text batch is in the counters (fpl_get_counters, fpl_counters_device_ptr) once fpl_wait_text has returned for it: its per-read
 * kernels are enqueued by fpl_start_text or by that call (the uploads of the next chunks, submitted before, run beside them).  n_bytes < 4 GiB (line
 * positions are 32 bits).
 */
#define FPL_TEXT_OK 0
#define FPL_TEXT_IRREGULAR 1
#define FPL_TEXT_TOO_MANY 2
#define FPL_TEXT_CANCELLED 3
typedef struct fpl_text_result {
    uint32_t n_reads;      /* records of the chunk (0 unless status is FPL_TEXT_OK) */
    uint32_t status;       /* FPL_TEXT_* */
    uint64_t n_bases;      /* bases of all reads */
    uint64_t bad_record;   /* FPL_TEXT_IRREGULAR: index of the first record that failed a check, ~0 when the structure did */
    uint32_t max_read_len; /* longest read */
    uint32_t n_lines;      /* line breaks found */
} fpl_text_result;
int fpl_process_text_async(fpl_ctx* ctx, const uint8_t* text, uint64_t n_bytes);
int fpl_peek_text(fpl_ctx* ctx, fpl_text_result* out);
int fpl_start_text(fpl_ctx* ctx);
int fpl_cancel_text(fpl_ctx* ctx);
int fpl_wait_text(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts);

/*
 * (ABI v9) The passing reads of a text batch as gzip, deflated on the device (csrc/gz_emit.h): what a host writes to an --out
 * whose name ends in .gz, without formatting or deflating a byte itself.
 *
 *   fpl_set_text_gzip   a switch of the context, read by fpl_process_text_async: a text batch submitted while it is on is a
 *                       GZIP batch.  Changes nothing about the batch's records, line starts or counters.
 *   fpl_wait_text_gz    fpl_wait_text for the oldest batch in flight, plus its bytes: *gz points to *gz_len bytes that are one
 *                       complete gzip member (RFC 1952; deflate blocks of literals with dynamic Huffman tables, stored blocks
 *                       where a table would not pay) whose inflation is, byte for byte, what the host's formatter appends to
 *                       --out for this batch from `results` and the text: every fragment with code FPL_PASS_FILTER of every read
 *                       that was not dropped, in input order, lines ended by "\n".  Appending the members of successive batches
 *                       to a file gives a valid .gz of the whole output.  *gz_len is 0 (and *gz NULL) when no read passed, when
 *                       the batch's status is not FPL_TEXT_OK, or when the batch was submitted with the switch off.  The layout
 *                       kernel is enqueued behind the batch's per-read kernels on their stream (by fpl_start_text or this call);
 *                       THIS call reads its sizes back, sizes the buffers by them, enqueues the other kernels on the same stream
 *                       and copies the member, on the copy stream, into a page-locked buffer of the batch's slot: two waits for
 *                       the device beside the one for the records.  *gz is the library's and, like results and line_starts, stays
 *                       valid until the next submission that takes this batch's slot.  A gzip batch may also be collected with
 *                       fpl_wait_text: its bytes are then never made.
 *                       Size: never more than 23 + n + 5 * (n / FPL_GZ_BLOCK_BYTES + 1 + 2 * fragments) bytes for n bytes of text.
 *   fpl_get_gzip_batches  how many batches fpl_wait_text_gz (and, ABI v10, fpl_wait_bam_gz) has made members for (the sibling of
 *                       fpl_get_batch_forms).
 */
#define FPL_GZ_BLOCK_BYTES 16384
int fpl_set_text_gzip(fpl_ctx* ctx, int on);
int fpl_wait_text_gz(fpl_ctx* ctx, fpl_text_result* out, const fpl_read_result** results, const uint32_t** line_starts,
                     const uint8_t** gz, uint64_t* gz_len);
int fpl_get_gzip_batches(const fpl_ctx* ctx, uint64_t* out);

/*
 * (ABI v8) BAM records in: the host inflates a BAM's BGZF blocks and walks its records (24 bytes of each: where it starts, its
 * flag, l_seq); the device decodes the packed bases and the qualities (fastplong_amd/csrc/bam_decode.h).  The link carries the
 * packed form up (1.5 bytes per base: half a byte of base, one of quality) and the decoded one back (2 bytes per base, beside the
 * uploads of the next batches on a full-duplex link).  What a record becomes is `samtools fastq`'s twin of it:
 * bases from the 4-bit codes "=ACMGRSVTWYHKDBN" (high nibble first), qualities min(phred, 93) + 33, and for flag 0x10 the bases
 * reverse-complemented (the complement of a code is its four bits reversed) and the qualities reversed.  Which records are
 * passed (secondary / supplementary ones are not), and every check of the file's structure, are the caller's.
 *
 *   bam        the inflated record bytes, n_bytes of them (page-locked memory recommended);
 *   rec_start  n_reads byte offsets into bam: where record i starts (at its block_size field);
 *   off        n_reads + 1 CSR offsets of the output, off[i + 1] - off[i] = l_seq of record i (off[0] may be > 0);
 *   seq_out, qual_out  receive the ASCII bases / qualities of read i at [off[i], off[i + 1]) -- caller-owned arrays of at least
 *              off[n_reads] bytes; for fpl_process_bam_async they must be page-locked (fpl_host_alloc), the device writes them.
 * Every record must lie inside [0, n_bytes) -- fixed fields, name, CIGAR, bases, qualities -- and its l_seq agree with off:
 * the library checks this on the calling thread (FPL_ERR_ARG otherwise; nothing is enqueued).
 *
 *   fpl_process_bam_async  the BAM form of fpl_process_batch_async: takes one of the FPL_MAX_IN_FLIGHT slots, keeps the FIFO order
 *              and is collected by fpl_wait(), after which results[i], seq_out and qual_out hold the batch exactly as if the decoded
 *              arrays had been submitted through fpl_process_batch_async (--break / --mask fragment lists included: fpl_get_fragments
 *              after the wait).  bam, rec_start and off must stay valid, and seq_out / qual_out / results untouched, until the
 *              batch has been waited for.
 *   fpl_decode_bam  decode only, no context, synchronous (like fpl_count_end_kmers): the evaluation prefix of a BAM input --
 *              RNA check, adapter detection, read-count estimate -- runs before any context exists.  Any host memory; nothing is
 *              kept after the call returns.
 */
int fpl_process_bam_async(fpl_ctx* ctx, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off,
                          uint32_t n_reads, uint8_t* seq_out, uint8_t* qual_out, fpl_read_result* results);
int fpl_decode_bam(int32_t device, const uint8_t* bam, uint64_t n_bytes, const uint64_t* rec_start, const uint64_t* off, uint32_t n_reads,
                   uint8_t* seq_out, uint8_t* qual_out);

/*
 * (ABI v10) The passing reads of a BAM batch as gzip, composed and deflated on the device: v8 and v9 joined.  Everything a member
 * needs is in the batch's slot once fpl_process_bam_async has run -- the record bytes (the names), the decoded bases and
 * qualities, the per-read records -- so a host that writes BAM input to a .gz neither formats nor deflates, and need not get the
 * decoded arrays (2 bytes per base) back at all.
 *
 *   fpl_set_bam_gzip   a switch of the context, read by fpl_process_bam_async (the sibling of fpl_set_text_gzip): a BAM batch
 *                      submitted while it is on is a GZIP batch.  Changes nothing about the batch's records, fragments or
 *                      counters.  A gzip batch may pass seq_out == NULL && qual_out == NULL: the decoded arrays are then not
 *                      copied back.  Both NULL or neither (FPL_ERR_ARG otherwise); with the switch off NULL stays FPL_ERR_ARG.
 *                      Contexts with break_enabled / mask_enabled write from fragment lists: the switch is refused
 *                      (FPL_ERR_STATE) for them until fpl_set_fragment_output is on.
 *   fpl_wait_bam_gz    fpl_wait for the oldest batch in flight, plus its bytes: one complete gzip member whose inflation is, byte
 *                      for byte, what the host's formatter appends to --out for the batch's FASTQ twin and `results` -- name
 *                      line '@' + the record's read name (up to its NUL), the '+' line the one byte '+', and as for
 *                      fpl_wait_text_gz every fragment with code FPL_PASS_FILTER of every read that was not dropped, in input
 *                      order, the "split-by-adapter-left-" / "-right-" prefix behind the '@'.  Lifetime, the empty output
 *                      (*gz_len 0 and *gz NULL: no read passed, or the batch is not a gzip batch -- a CSR batch or a BAM batch
 *                      submitted with the switch off is collected exactly as by fpl_wait) and the way the member is made are
 *                      those of fpl_wait_text_gz.  Size: never more than 23 + n + 5 * (n / FPL_GZ_BLOCK_BYTES + 1 + 2 *
 *                      fragments) bytes for n bytes of text.  A gzip batch may also be collected with fpl_wait: its bytes are
 *                      then never made.  A text batch at the head of the queue: FPL_ERR_STATE, as for fpl_wait.
 * fpl_get_gzip_batches counts the members of both calls.
 */
int fpl_set_bam_gzip(fpl_ctx* ctx, int on);
int fpl_wait_bam_gz(fpl_ctx* ctx, const uint8_t** gz, uint64_t* gz_len);

/*
 * The container of a gzip batch's bytes.  FPL_ABI_VERSION stays 10: found by symbol lookup like the inflater calls below; a
 * library without it writes members only, and its caller frames on the host.
 *
 *   fpl_set_gzip_framing  per context; applies to every kind that can return gzip bytes (text, BGZF text, BAM, BGZF BAM) and takes
 *                      effect with the NEXT submission: a batch keeps the framing the context had when it was submitted, so a
 *                      switch with batches in flight is safe.  Other values: FPL_ERR_ARG, and nothing changes.
 *     FPL_GZIP_MEMBER  (the default) one gzip member per batch, as documented above.
 *     FPL_GZIP_BGZF    a whole number of BGZF blocks per batch.  Block k holds exactly bytes [k * 49 152, min((k + 1) * 49 152,
 *                      n)) of the batch's n bytes of text (49 152 = 3 * FPL_GZ_BLOCK_BYTES): an 18-byte header (1f 8b 08 04, no
 *                      time, XFL 0, OS ff, XLEN 6, 'B' 'C' 2 0, BSIZE = the block's bytes - 1), the deflate blocks of that
 *                      stripe -- BFINAL 0, each followed by its aligning empty stored block; dynamic blocks declare two distance
 *                      codes of length 1, a complete set --, one final empty stored block 01 00 00 ff ff, then CRC-32 and ISIZE
 *                      of the BLOCK's bytes.  Every block but the last has ISIZE 49 152; no block is larger than 49 152 + 5 * 53
 *                      + 31 bytes.  Blocks of successive batches appended to a file, then the 28-byte BGZF EOF block (the
 *                      caller's), are a BGZF file: fpl_inflate_bgzf and fpl_process_bgzf_text_async take every block of it.
 *                      Size: never more than n + 5 * (deflate blocks) + 31 * ceil(n / 49 152) bytes.  The inflated bytes, the
 *                      empty output (no read passed: *gz_len 0) and the lifetime are those of the member form.
 */
enum { FPL_GZIP_MEMBER = 0, FPL_GZIP_BGZF = 1 };
int fpl_set_gzip_framing(fpl_ctx* ctx, int framing);

/*
 * The form of a gzip batch's bytes.  FPL_ABI_VERSION stays 10: found by symbol lookup like fpl_set_gzip_framing; a caller of a
 * library without it converts and frames on the host.
 *
 *   fpl_set_gzip_records  per context; applies to every kind that can return gzip bytes and takes effect with the NEXT submission,
 *                      like the framing: a switch with batches in flight is safe.  Other values: FPL_ERR_ARG, and nothing changes.
 *     FPL_GZIP_FASTQ   (the default) the bytes inflate to FASTQ text, as documented above.
 *     FPL_GZIP_BAM     the bytes inflate to unaligned BAM records, one per passing fragment in the text's order: block_size, refID
 *                      -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag 4, l_seq, next_refID -1, next_pos -1, tlen
 *                      0; the name -- the FASTQ name line without its '@' (the split prefix included), cut at the first space or
 *                      tab, truncated to 254 bytes, "*" when nothing is left -- and its NUL; (l_seq + 1) / 2 bytes of bases in
 *                      htslib's seq_nt16_table codes, high nibble first; l_seq qualities, max(byte, 33) - 33.  No tags.
 *                      The framing is BGZF whatever fpl_set_gzip_framing says: a whole number of blocks of 49 152 record bytes
 *                      each, the last one short, nothing (*gz_len 0) when no read passed; no block is larger than 49 152 + 5 * 68
 *                      + 31 bytes.  There is no BAM header and no EOF block in them: a file is the caller's header block(s),
 *                      the batches' bytes in order, and the 28-byte EOF block.
 */
enum { FPL_GZIP_FASTQ = 0, FPL_GZIP_BAM = 1 };
int fpl_set_gzip_records(fpl_ctx* ctx, int records);

/*
 * The auxiliary fields of a BAM input's records in the BAM records of a gzip batch (README "BAM output", --keep_tags).
 * FPL_ABI_VERSION stays 10: both calls are found by symbol lookup; a caller of a library without them writes such records on the host.
 *
 *   fpl_set_bam_tags   per context; on != 0 takes effect with the NEXT submission, like fpl_set_gzip_records.  It changes the
 *                      bytes of a gzip batch only where the batch holds BAM records (fpl_process_bam_async,
 *                      fpl_process_bgzf_bam_async) AND its bytes are BAM records (FPL_GZIP_BAM); every other batch ignores it.
 *                      Then an output record carries, right behind its qualities and counted by its block_size, fields of the input
 *                      record its read came from.  The input record's aux region is what lies between its qualities and its end
 *                      (4 + block_size, never past the bytes submitted).  Fields are taken from its front -- two tag bytes, a
 *                      type, a value: A c C 1 byte, s S 2, i I f 4, Z H up to and including the first NUL, B a subtype of
 *                      cCsSiIf, a u32 count and count values -- up to the first that does not parse: the parsed prefix.  An output
 *                      record that is the only fragment of its read (n_frag 1, kind 0), all of it, of an input record without flag
 *                      0x10, in a context without --break / --mask gets the prefix verbatim; every other one gets the prefix
 *                      without its positional fields (type B, or tag MM Mm ML Ml MN), in their order.  Both fragments of a split
 *                      read carry the read's fields.  Nothing else of the records changes; the deflate blocks are cut by the
 *                      same rule, and a batch is at most twice its input record bytes longer than without the switch.
 *                      The file's header is the caller's: it should repeat the input's @RG lines (the CLI does).
 *   fpl_get_bam_tag_stats   out[4], counted per output record since the context was made: records that kept every field of
 *                      their parsed prefix, records that lost positional fields, tag bytes written, records whose region did not
 *                      parse to its end.  It waits for the kernels of every batch submitted so far.
 */
int fpl_set_bam_tags(fpl_ctx* ctx, int on);
int fpl_get_bam_tag_stats(fpl_ctx* ctx, uint64_t* out);

/*
 * MM / ML / MN re-indexed in such records where they are trimmed or split (README "BAM output", --keep_mods; the rule and its
 * wording: csrc/bam_mod_rules.h).  FPL_ABI_VERSION stays 10: both calls are found by symbol lookup; a caller of a library
 * without them writes such records on the host.
 *
 *   fpl_set_bam_mods   per context; takes effect with the NEXT submission and is ignored unless fpl_set_bam_tags is on.  A changed
 *                      output record -- one that does not get its prefix verbatim -- of a RE-INDEXABLE input record gets, in the
 *                      places of its MM, ML and MN fields, those fields rewritten for its bases [frag_start, + frag_len) of the
 *                      read: per group the deltas that fall on a base of the fragment, the first of them counted from the
 *                      fragment's first base, their ML values, MN = frag_len.  Every other positional field is dropped as before.
 *                      Re-indexable: flag without 0x10, no --break / --mask, exactly one MM (or Mm) of type Z and one ML (Ml) of
 *                      type B:C, at most one integer MN (Mn) that equals l_seq, an MM value of at most 16 well-formed groups whose
 *                      deltas (1 to 9 digits) do not run past the read's count of the group's base, an ML count that matches.  A
 *                      record with such fields that is not re-indexable is written as without the switch.  A record's tag bytes
 *                      never exceed its input region: the bound of fpl_set_bam_tags stands.
 *   fpl_get_bam_mod_stats   out[4], since the context was made: output records re-indexed; changed output records whose
 *                      modification fields were not re-indexable and were dropped; modification positions kept; positions cut
 *                      away.  It waits like fpl_get_bam_tag_stats, whose counts keep their meaning: a re-indexed record that lost
 *                      no other positional field counts as one that kept every field.
 */
int fpl_set_bam_mods(fpl_ctx* ctx, int on);
int fpl_get_bam_mod_stats(fpl_ctx* ctx, uint64_t* out);

/*
 * The move table mv and its ts re-indexed in such records where they are trimmed or split (README "BAM output", --keep_moves; the
 * rule and its wording: csrc/bam_move_rules.h).  FPL_ABI_VERSION stays 10: both calls are found by symbol lookup; a caller of a
 * library without them writes such records on the host.
 *
 *   fpl_set_bam_moves  per context; takes effect with the NEXT submission and is ignored unless fpl_set_bam_tags is on.  It is
 *                      independent of fpl_set_bam_mods: either switch decides its own fields.  A changed output record of a
 *                      MOVE-RE-INDEXABLE input record gets, in the places of its mv and ts fields, the table cut to the moves of
 *                      its bases [frag_start, + frag_len) of the read -- the stride in front, leading zeros kept where frag_start
 *                      is 0 -- and ts advanced by stride x the moves cut from the front, widened to S or I where its own type
 *                      does not hold the value.  Move-re-indexable: flag without 0x10, no --break / --mask, exactly one mv of type
 *                      B:c or B:C with a stride in 1..127 and moves of 0 and 1 of which l_seq are 1, at most one ts of an integer
 *                      type that is not negative.  A record with a table that is not re-indexable, and an output record whose new
 *                      ts passes 2^32 - 1 or whose two fields would grow, is written as without the switch.  A record's tag bytes
 *                      never exceed its input region: the bound of fpl_set_bam_tags stands.
 *   fpl_get_bam_move_stats  out[4], since the context was made: output records re-indexed; changed output records with a table
 *                      that were not re-indexable and lost it; table entries (moves) kept; entries cut away.  It waits like
 *                      fpl_get_bam_tag_stats, whose counts keep their meaning: a changed record counts as one that kept every
 *                      field when every positional field it has was re-indexed by one of the two switches.
 */
int fpl_set_bam_moves(fpl_ctx* ctx, int on);
int fpl_get_bam_move_stats(fpl_ctx* ctx, uint64_t* out);

/*
 * The auxiliary fields of a BAM input's records as COMMENTS behind the names of a gzip batch's FASTQ text (README "Tags as FASTQ
 * comments", --comment_tags; the rule and its wording: csrc/bam_comment_rules.h).  FPL_ABI_VERSION stays 10: both calls are found
 * by symbol lookup; a caller of a library without them formats such batches on the host.
 *
 *   fpl_set_bam_comments   per context; tags holds 2 * n_tags bytes, the selection: n_tags 0 switches the comments off, -1 selects
 *                      every field, 1 to 32 the fields whose two tag bytes equal one of the list's exactly.  More than 32 tags, or
 *                      a byte outside [A-Za-z][A-Za-z0-9], is FPL_ERR_ARG and changes nothing.  It takes effect with the NEXT
 *                      submission, like fpl_set_bam_tags, and changes the bytes of a gzip batch only where the batch holds BAM
 *                      records (fpl_process_bam_async, fpl_process_bgzf_bam_async with fpl_set_bam_gzip on) AND its bytes are FASTQ
 *                      text (FPL_GZIP_FASTQ), in member and in BGZF framing; every other batch ignores it.  It does not depend on
 *                      fpl_set_bam_tags / fpl_set_bam_mods, which keep applying to FPL_GZIP_BAM only.  Then the name line of an
 *                      output read ends with the selected ones among the fields its BAM record would carry with both of those
 *                      switches on -- the parsed prefix for an unchanged record, the non-positional fields for a changed one, MM /
 *                      ML / MN re-indexed for a changed record of a re-indexable input record --, in their order, each behind one
 *                      tab, in the SAM text form: XX:A:c, XX:i:<decimal> for c C s S i I, XX:f:<what printf("%g") gives>, XX:Z: and
 *                      XX:H: with the value, XX:B:<subtype> and ,<value> per element.  A selected A, Z or H field with a byte below
 *                      0x20 or the byte 0x7F in its value is left out.  The deflate blocks are cut by the same rule; a batch is at
 *                      most ten times its input record bytes longer than without the switch (a field's text is at most five times
 *                      its bytes, and both fragments of a split read carry the read's fields).
 *   fpl_get_bam_comment_stats   out[4], since the context was made: output records that got at least one field, fields written,
 *                      comment bytes (tabs included), fields left out for control bytes.  It waits like fpl_get_bam_tag_stats.
 */
int fpl_set_bam_comments(fpl_ctx* ctx, const char* tags, int n_tags);
int fpl_get_bam_comment_stats(fpl_ctx* ctx, uint64_t* out);

/*
 * The BGZF blocks of a BAM inflated on the device (csrc/bgzf_inflate.h).  FPL_ABI_VERSION stays 10: a caller finds these three
 * calls by symbol lookup (dlsym), as it does the calls of v9 and v10, and a library without them is a valid v10 library -- the
 * caller then inflates on the host.
 *
 * The inflater is a handle of its own, not part of a context: the evaluation prefix of a BAM input is read before any fpl_ctx
 * exists (as for fpl_decode_bam).  It owns one stream and its device buffers, which grow with headroom and never shrink.
 *
 *   fpl_inflater_create   NULL when the device cannot be used.
 *   fpl_inflate_bgzf      comp[0 .. comp_bytes) holds the blocks' raw deflate payloads (what lies between a block's gzip header and
 *                         its 8-byte trailer), blocks[i] says where payload i is (comp_off, comp_len <= 16 MiB), where its output
 *                         goes (out_off, isize <= 65536) and what the trailer says (isize, crc32).  Every range is checked on the
 *                         calling thread first: a range outside comp / out is FPL_ERR_ARG and nothing is enqueued.  One call
 *                         uploads comp and the descriptors, launches ONE kernel (a wave per block) and brings back the output
 *                         ranges of the blocks -- bytes of out between them are not touched -- and blocks[i].status.  Synchronous.
 *                         Page-locked comp and out (fpl_host_alloc) are recommended; pageable memory works.  n_blocks == 0: FPL_OK,
 *                         nothing done.  Thread-compatible: one call at a time per handle.
 *   status                FPL_BGZF_OK: out[out_off .. out_off + isize) is the block's data, size and CRC-32 agree with the trailer.
 *                         Anything else: REFUSED -- the bytes of that range are undefined and the caller inflates the block itself;
 *                         the device never has the last word on a bad block.  The kernel refuses whatever it does not vouch for
 *                         (docs/kernels.md), among it streams zlib accepts: a distance code of a single 1-bit code.
 */
typedef struct fpl_bgzf_block { /* 32 bytes */
    uint64_t comp_off;
    uint64_t out_off;
    uint32_t comp_len;
    uint32_t isize;
    uint32_t crc32;
    uint32_t status; /* out */
} fpl_bgzf_block;
enum {
    FPL_BGZF_OK = 0,
    FPL_BGZF_MALFORMED = 1, /* not a deflate stream this kernel decodes */
    FPL_BGZF_SIZE = 2,      /* more or fewer bytes than isize */
    FPL_BGZF_CRC = 3,       /* the bytes' CRC-32 is not the trailer's */
    FPL_BGZF_OVERRUN = 4    /* the stream goes on behind comp_len */
};
typedef struct fpl_inflater fpl_inflater;
fpl_inflater* fpl_inflater_create(int32_t device);
int fpl_inflate_bgzf(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, fpl_bgzf_block* blocks, uint32_t n_blocks, uint8_t* out,
                     uint64_t out_bytes);
void fpl_inflater_destroy(fpl_inflater* inf);

/*
 * A BAM's BGZF blocks in, records out: the inflate, the record walk, the decode and the per-read kernels chained on the device, the
 * inflated bytes never leaving it (csrc/bgzf_inflate.h -> csrc/bam_walk.h -> csrc/bam_decode.h -> the per-read kernels, and with
 * fpl_set_bam_gzip on, the gzip kernels).  FPL_ABI_VERSION stays 10: found by symbol lookup; a library without these calls is a
 * valid v10 library, and the caller then takes fpl_inflate_bgzf / fpl_process_bam_async.
 *
 * A BAM record says where the next one starts, and a batch of blocks rarely ends at a record's end: the bytes behind the last whole
 * record of a submission -- the TAIL -- are kept in the context, on the device, and go in front of the next submission's bytes.
 * The walk of submission k + 1 is ordered behind that of submission k on the context's parse stream; that order carries the tail,
 * and no submission waits for a walk.  The rules of a record are the host walk's (csrc/bam_rules.h, host/bam.cpp); the device
 * words no errors: a submission is taken whole or REFUSED by status, and what is refused the caller takes through the host path.
 *
 *   fpl_process_bgzf_bam_async  comp, comp_bytes, blocks, n_blocks: as for fpl_inflate_bgzf (payloads and descriptors; status is
 *                      not written back), with out_off relative to this submission's inflated bytes.  The blocks must be in order
 *                      and without gaps: out_off[0] == 0, out_off[i + 1] == out_off[i] + isize[i]; the total is at most 0xFFFFFFF0.
 *                      Ranges are checked on the calling thread (FPL_ERR_ARG, nothing enqueued).  skip: inflated bytes in front of
 *                      the first record -- the BAM header, which the caller parses itself; valid only while the context holds no
 *                      tail as far as the host knows: no submission since fpl_create, since fpl_bam_tail_set(ctx, NULL, 0), or since
 *                      an fpl_resume_bgzf_bam that found the tail empty (a refused first stretch goes in again with its skip);
 *                      FPL_ERR_ARG otherwise.  Takes one of the
 *                      FPL_MAX_IN_FLIGHT slots, FIFO.  The upload goes on the copy stream, inflate and walk on the parse stream
 *                      behind it; only the 64-byte header comes back.  comp and blocks must stay valid until the batch has been
 *                      peeked at or waited for.  Contexts with break_enabled / mask_enabled: FPL_ERR_STATE, as for text.
 *   fpl_peek_bgzf_bam  waits for the header of the oldest such batch that is not started, and fills *out.  Nothing of the batch is
 *                      counted yet.
 *   fpl_start_bgzf_bam enqueues the decode and the per-read kernels of that batch.  seq_out, qual_out: page-locked arrays of
 *                      n_bases bytes (the header's) that get the decoded reads as fpl_process_bam_async's do, or both NULL: the
 *                      decoded arrays then stay on the device (the stats-only caller, the gzip batch).  One NULL: FPL_ERR_ARG.
 *                      A refused or empty batch: FPL_OK, nothing to start.
 *   fpl_wait_bgzf_bam  the oldest batch in flight, which must be of this kind (FPL_ERR_STATE otherwise, as fpl_wait, fpl_wait_text
 *                      and fpl_wait_bam_gz are for a batch of this kind).  Starts it with NULL arrays if it was not started.  *out
 *                      is the header; for status FPL_BAMW_OK *results are the n_reads records, *names the name_bytes bytes of all
 *                      names ('@' + the record's read name up to its NUL, nothing between them) and *name_off n_reads + 1 offsets
 *                      into them -- library memory, valid until the next submission that takes this batch's slot, as fpl_wait_text
 *                      documents for its pointers.  gz, gz_len (may be NULL): when fpl_set_bam_gzip was on at submission, the
 *                      member of fpl_wait_bam_gz.  Any of the pointer arguments but ctx and out may be NULL.
 *
 *   status             FPL_BAMW_OK.  FPL_BAMW_BLOCK: a block k_bgzf_inflate did not vouch for, bad_index is the first.
 *                      FPL_BAMW_RECORD: a record failed a check; bad_index is its index in the file (skipped records counted,
 *                      from the first submission of the file on) and bad_pos its byte offset in [the tail | this submission's
 *                      inflated bytes].  FPL_BAMW_TAIL_ROOM: the new tail (tail_bytes) exceeds the context's tail capacity.
 *                      FPL_BAMW_TOO_MANY: more records than the slot's arrays hold (one per 64 bytes and 1024), or names that
 *                      take more than a quarter of [tail room | inflated bytes] and 1 MiB.
 *                      FPL_BAMW_CHAIN: an earlier submission was refused.
 *                      A refused submission counts nothing, leaves the tail exactly as it was, and sets a flag in device memory
 *                      that the walks of the submissions already queued behind it read: they refuse with FPL_BAMW_CHAIN.
 *
 * Recovery (shared with the BGZF text path below, whose submissions keep their tail in the same place; all four calls:
 * FPL_ERR_STATE while a batch of either kind is in flight.  A context's tail belongs to the kind that submitted last, and this
 * kind's submission is FPL_ERR_STATE while the context holds a BGZF text tail as far as the host knows):
 *   fpl_bam_tail_get   the tail's bytes into buf (cap bytes; *len gets the length, FPL_ERR_ARG with *len set when cap is short).
 *   fpl_bam_tail_set   replaces the tail and clears the flag; len 0 is a new file (skip is allowed again, record indices restart).
 *   fpl_resume_bgzf_bam  clears the flag and keeps the tail (an empty one allows skip again): the refused blocks are submitted
 *                      again, e.g. after
 *   fpl_reserve_bam_tail  which makes the tail capacity at least `bytes` (before the first submission: exactly `bytes`; the
 *                      default is FPL_BAM_TAIL_DEFAULT, which holds one record of a 5 Mb read -- a default, not a measured optimum).
 * Any refused stretch goes through the host path without losing a record: get the tail, inflate the refused blocks behind it and
 * walk the bytes on the host, hand the whole records to fpl_process_bam_async, set the tail to the rest, and go on.
 *
 * Environment (read in fpl_create): FPL_BAM_SEG_BYTES=n cuts the walk into segments of n bytes, not of 64 KiB -- for tests, which
 * want many segments from a small file; a value below 64 or above 2^30 is ignored.
 */
#define FPL_BAM_TAIL_DEFAULT (8u << 20)
typedef struct fpl_bam_window { /* 64 bytes */
    uint32_t status;
    uint32_t n_reads;      /* records taken */
    uint64_t n_bases;
    uint32_t max_read_len;
    uint32_t segments;     /* segments the walk cut the buffer into */
    uint64_t name_bytes;
    uint64_t records_seen; /* n_reads and the skipped (secondary / supplementary) ones */
    uint32_t tail_bytes;
    uint32_t rewalked;     /* segments whose guess the chain did not prove, walked again serially */
    uint64_t bad_index;
    uint64_t bad_pos;
} fpl_bam_window;
enum {
    FPL_BAMW_OK = 0,
    FPL_BAMW_BLOCK = 1,
    FPL_BAMW_RECORD = 2,
    FPL_BAMW_TAIL_ROOM = 3,
    FPL_BAMW_TOO_MANY = 4,
    FPL_BAMW_CHAIN = 5
};
int fpl_process_bgzf_bam_async(fpl_ctx* ctx, const uint8_t* comp, uint64_t comp_bytes, const fpl_bgzf_block* blocks, uint32_t n_blocks,
                               uint64_t skip);
int fpl_peek_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out);
int fpl_start_bgzf_bam(fpl_ctx* ctx, uint8_t* seq_out, uint8_t* qual_out);
int fpl_wait_bgzf_bam(fpl_ctx* ctx, fpl_bam_window* out, const fpl_read_result** results, const uint8_t** names, const uint64_t** name_off,
                      const uint8_t** gz, uint64_t* gz_len);
int fpl_bam_tail_get(fpl_ctx* ctx, uint8_t* buf, uint64_t cap, uint64_t* len);
int fpl_bam_tail_set(fpl_ctx* ctx, const uint8_t* bytes, uint64_t len);
int fpl_resume_bgzf_bam(fpl_ctx* ctx);
int fpl_reserve_bam_tail(fpl_ctx* ctx, uint64_t bytes);

/*
 * BGZF-compressed FASTQ in, records out: the blocks of a .fastq.gz that bgzip (or `samtools fastq | bgzip`) wrote are inflated, cut
 * at a record's end, parsed and run on the device, the inflated text never leaving it (csrc/bgzf_inflate.h -> csrc/text_walk.h ->
 * the per-read kernels, and with fpl_set_text_gzip on, the text forms of the gzip kernels).  FPL_ABI_VERSION stays 10: found by
 * symbol lookup; a library without these calls is a valid v10 library, and the caller then inflates on the host and takes
 * fpl_process_text_async.
 *
 * A window of blocks rarely ends at a record's end.  The bytes start at a record (the file's start, or the tail), so with L line
 * breaks in [tail | inflated bytes] the submission holds L / 4 records, and the bytes behind line break 4 (L / 4) - 1 are the new
 * TAIL.  The tail, its capacity, the refusal flag and the four recovery calls are those of the BGZF-BAM path above
 * (fpl_bam_tail_get, fpl_bam_tail_set, fpl_resume_bgzf_bam, fpl_reserve_bam_tail): a context's tail belongs to the kind that
 * submitted last, and submitting the OTHER kind while the context is not fresh -- its tail empty as far as the host knows, the
 * condition that allows fpl_process_bgzf_bam_async's skip -- is FPL_ERR_STATE.  The recovery calls are FPL_ERR_STATE while a
 * batch of either kind is in flight.
 *
 *   fpl_process_bgzf_text_async  the arguments of fpl_process_bgzf_bam_async without skip: payloads and descriptors in order and
 *                      without gaps, ranges checked on the calling thread (FPL_ERR_ARG, nothing enqueued); the tail capacity plus
 *                      the inflated bytes is at most 0xFFFFFFF0 (line positions are 32 bits).  Takes one of the FPL_MAX_IN_FLIGHT
 *                      slots, FIFO.  A submission made while fpl_set_text_gzip is on is a gzip batch.  Contexts with
 *                      break_enabled / mask_enabled: FPL_ERR_STATE, as for text.  comp and blocks must stay valid until the batch
 *                      has been peeked at or waited for.
 *   fpl_peek_bgzf_text waits for the header of the oldest such batch that is not started, and fills *out; nothing is counted yet.
 *   fpl_start_bgzf_text  enqueues the per-read kernels of that batch.  seq_out, qual_out: page-locked arrays of n_bases bytes (the
 *                      header's) that get the bases and qualities as a CSR pair (read i at the running sum of the lengths in
 *                      results), or both NULL: the arrays stay on the device.  One NULL: FPL_ERR_ARG.
 *   fpl_wait_bgzf_text the oldest batch in flight, which must be of this kind (FPL_ERR_STATE otherwise, nothing touched -- and
 *                      every other wait is FPL_ERR_STATE for a batch of this kind).  Starts it with NULL arrays if it was not
 *                      started.  *out is the header; for status FPL_TXTW_OK *results are the n_reads records, *names the name_bytes
 *                      bytes of all names -- every read's whole first line, '@' included, without its line break ("\n" or
 *                      "\r\n"), nothing between them -- and *name_off n_reads + 1 offsets into them; library memory, valid until
 *                      the next submission that takes this batch's slot.  gz, gz_len (may be NULL, together): the member of
 *                      fpl_wait_text_gz when the batch is a gzip batch.
 *
 *   status             FPL_TXTW_OK: taken whole.  FPL_TXTW_BLOCK: a block k_bgzf_inflate did not vouch for, bad_index is the
 *                      first.  FPL_TXTW_IRREGULAR: text in front of the cut that fpl_process_text_async would call irregular -- a
 *                      blank line, a '\r' that is not followed by '\n', a record that fails the '@' / '+' / equal-lengths checks;
 *                      bad_index is the first failing record's index in the file (from the first submission of the file on), ~0
 *                      when only the structure failed, and bad_pos the offset in [the tail | this submission's inflated bytes]
 *                      of that record or of the '\r', whichever comes first.  (A '\r' that is the last byte of a submission is
 *                      judged with the next one, when the byte behind it is there.)
 *                      FPL_TXTW_STRAND: a third line longer than "+" once its "\r" is taken off.  Such a line repeats the name;
 *                      the names this path gives back cannot carry it, and the gzip member writes the line as it stands, so a
 *                      file with such lines takes the host path.  bad_index / bad_pos: that record.
 *                      FPL_TXTW_TAIL_ROOM: the new tail (tail_bytes) exceeds the context's tail capacity.
 *                      FPL_TXTW_TOO_MANY: more records than one per 64 bytes of [tail room | inflated bytes] and 16, or names that
 *                      take more than a quarter of that and 1 MiB.
 *                      FPL_TXTW_CHAIN: an earlier submission was refused.
 *                      A refused submission counts nothing, leaves the tail exactly as it was, and sets the flag in device memory
 *                      that the submissions already queued behind it read: they refuse with FPL_TXTW_CHAIN.
 *   records_seen       the records of the file in the submissions accepted so far, this one included.
 *
 * A refused stretch goes through the host path without losing a record:
 *     fpl_bam_tail_get -> T;  inflate the refused blocks on the host -> B;  parse T + B with the host's reader, which keeps the
 *     bytes behind the last whole record -> R;  the records through fpl_process_batch_async;  fpl_bam_tail_set(R);  go on with
 *     the blocks behind the refused ones.   For FPL_TXTW_TAIL_ROOM: fpl_reserve_bam_tail(tail_bytes), fpl_resume_bgzf_bam, and
 *     the refused blocks (and those refused with CHAIN behind them) again.
 * End of input: a file's last line break makes the last tail empty.  A file without one leaves its last record in the tail:
 *     fpl_bam_tail_get -> the record's bytes, through the host's reader and fpl_process_batch_async -- today's treatment of a
 *     chunk without a final line break.  fpl_bam_tail_set(ctx, NULL, 0) then starts a new file.
 */
typedef struct fpl_text_window { /* 64 bytes */
    uint32_t status;
    uint32_t n_reads;
    uint64_t n_bases;
    uint32_t max_read_len;
    uint32_t n_lines;      /* line breaks in [tail | inflated bytes] */
    uint64_t name_bytes;
    uint64_t records_seen;
    uint32_t tail_bytes;
    uint32_t reserved;
    uint64_t bad_index;
    uint64_t bad_pos;
} fpl_text_window;
enum {
    FPL_TXTW_OK = 0,
    FPL_TXTW_BLOCK = 1,
    FPL_TXTW_IRREGULAR = 2,
    FPL_TXTW_TAIL_ROOM = 3,
    FPL_TXTW_TOO_MANY = 4,
    FPL_TXTW_CHAIN = 5,
    FPL_TXTW_STRAND = 6
};
int fpl_process_bgzf_text_async(fpl_ctx* ctx, const uint8_t* comp, uint64_t comp_bytes, const fpl_bgzf_block* blocks, uint32_t n_blocks);
int fpl_peek_bgzf_text(fpl_ctx* ctx, fpl_text_window* out);
int fpl_start_bgzf_text(fpl_ctx* ctx, uint8_t* seq_out, uint8_t* qual_out);
int fpl_wait_bgzf_text(fpl_ctx* ctx, fpl_text_window* out, const fpl_read_result** results, const uint8_t** names, const uint64_t** name_off,
                       const uint8_t** gz, uint64_t* gz_len);

/*
 * ONE LONG deflate stream -- the payload of an ordinary one-member .gz -- inflated on the device, a window of compressed bytes per
 * call (csrc/gzip_inflate.h).  FPL_ABI_VERSION stays 10: found by symbol lookup like fpl_inflate_bgzf, on the same handle.
 *
 *   fpl_inflate_gzip   comp[0 .. comp_bytes) is a stretch of the member's raw deflate payload (at most 128 MiB behind the start
 *                      bit's byte) and start_bit the bit offset in it of a BLOCK START the caller knows: bit 0 of the payload, or
 *                      where the call before ended.  dict[0 .. dict_len) are the bytes in front of that point, the last 32 KiB of
 *                      them or all there are (dict_len <= 32768; NULL / 0 at a member's start).  The payload is cut into chunks of
 *                      chunk_bytes (0: the default, 32 KiB; 64 .. 16 MiB), block starts inside them are guessed, every chunk is
 *                      decoded on a wave of its own and the guesses are then checked along the chain; only what the chain proves
 *                      is given out.  out[0 .. res->out_bytes) gets the bytes, at most out_cap of them.  One upload, the launches,
 *                      one download; synchronous; bad arguments are FPL_ERR_ARG before anything runs.  One call at a time per handle.
 *   res                status FPL_GZIP_OK: out_bytes bytes are what inflating from start_bit gives, crc32 is their CRC-32, end_bit
 *                      is the bit offset in comp behind the last block decoded -- a block start for the next call, whose comp may
 *                      begin at byte end_bit / 8 -- and final_block says that block was the stream's last.  A call may end before
 *                      the end of comp (a block that goes on behind comp_bytes, a guess that was wrong, out_cap reached): the next
 *                      call goes on from end_bit.  Any other status: REFUSED -- nothing of out is defined and the caller inflates
 *                      from start_bit itself; the device never has the last word on a damaged stream.
 */
typedef struct fpl_gzip_window { /* 32 bytes */
    uint64_t out_bytes;
    uint64_t end_bit;
    uint32_t status;
    uint32_t crc32;
    uint32_t final_block;
    uint32_t chunks; /* chunks of the chain that were taken (for the curious) */
} fpl_gzip_window;
enum {
    FPL_GZIP_OK = 0,
    FPL_GZIP_MALFORMED = 1, /* not a deflate stream this decoder takes, from the very first block on */
    FPL_GZIP_ROOM = 2,      /* the first block alone makes more bytes than out_cap or than the device's room for a chunk */
    FPL_GZIP_OVERRUN = 3    /* the first block goes on behind comp_bytes */
};
int fpl_inflate_gzip(fpl_inflater* inf, const uint8_t* comp, uint64_t comp_bytes, uint64_t start_bit, const uint8_t* dict, uint32_t dict_len,
                     uint8_t* out, uint64_t out_cap, uint32_t chunk_bytes, fpl_gzip_window* res);

/*
 * The passing, trimmed reads of a resident batch as a CSR batch in device memory (csrc/emit.h): what a writer makes of the
 * records of fpl_process_batch_device, made where the bases are, so that a second consumer on the device -- an aligner, a k-mer
 * counter, another fpl_process_batch_device -- never meets the host.  FPL_ABI_VERSION stays 10: found by symbol lookup like the
 * inflater's calls; a library without it is a valid v10 library.
 *
 *   d_seq, d_qual, d_off, n_reads   the batch as it was handed to fpl_process_batch_device; d_results its records.
 *   The output read for input read i, fragment f is the window [d_off[i] + frag_start[f], + frag_len[f]) of d_seq and of d_qual.
 *   A fragment is put out when the read is not dropped, f < n_frag and code[f] == FPL_PASS_FILTER; the output is in input order,
 *   fragment 0 before fragment 1 -- the order, and the bases and quality lines, of what the host's formatter writes to --out.
 *   d_seq_out, d_qual_out   out_cap_bytes bytes each; output read j occupies [d_off_out[j], d_off_out[j + 1]) of both.  No alignment
 *                           is asked of them; they must not overlap the inputs.
 *   d_off_out               room for out_cap_reads + 1 offsets; d_off_out[0] = 0.
 *   d_src, d_kind           per output read the index of its input read and the record's kind (0 unsplit, 1 / 2 the left / right
 *                           part of a middle-adapter split): what a host needs to attach the names.  Either may be NULL.
 *   d_info                  32 bytes in DEVICE memory: the only thing a consumer reads back before it can size its next call.
 * out_cap_bytes = d_off[n_reads] and out_cap_reads = 2 * n_reads ALWAYS suffice: the fragments of a read are disjoint windows of it.
 *
 * The records are the caller's memory and are not trusted: a counted window that reaches outside its read sets status bit 0,
 * totals beyond out_cap_bytes / out_cap_reads set bit 1.  With any bit set n_out = 0, n_bytes = 0, d_off_out[0] = 0 and NOTHING
 * else is written; no read ever leaves [d_off[i], d_off[i + 1]) and no write the capacities.  (d_off itself is the caller's promise,
 * as for fpl_process_batch_device: non-decreasing.)
 *
 * Asynchronous on `stream` and without a wait on the host (the context's workspace -- the layout's per-block sums and eight bytes
 * per output read -- grows like every other: rarely, with headroom, behind a device-wide wait).  Placed on the stream behind the
 * fpl_process_batch_device that writes d_results, it is ordered behind it.  n_reads == 0 gives an all-zero info.
 * FPL_ERR_ARG: ctx or d_info NULL, n_reads > 0 with any other pointer but d_src / d_kind NULL, n_reads > 2^30.  FPL_ERR_STATE:
 * a context with break_enabled / mask_enabled -- its reads live in the fragment list (fpl_get_fragments), not in the records --
 * unless fpl_set_fragment_output is on (below: the call then puts out the fragments).  status bit 2 is that form's.
 */
typedef struct fpl_emit_info { /* 32 bytes, written in DEVICE memory */
    uint64_t n_bytes;          /* bytes of d_seq_out / d_qual_out used = d_off_out[n_out] */
    uint32_t n_out;            /* output reads */
    uint32_t max_len;          /* longest output read */
    uint32_t status;           /* 0 ok; bit 0: a fragment window reaches outside its read; bit 1: out_cap_bytes or out_cap_reads too small */
    uint32_t reserved[3];
} fpl_emit_info;
int fpl_emit_batch_device(fpl_ctx* ctx, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint32_t n_reads,
                          const fpl_read_result* d_results, uint8_t* d_seq_out, uint8_t* d_qual_out, uint64_t out_cap_bytes,
                          uint64_t* d_off_out, uint32_t out_cap_reads, uint32_t* d_src, uint8_t* d_kind, fpl_emit_info* d_info,
                          void* stream);

/* Page-locked host memory for the arrays handed to fpl_process_batch[_async] / fpl_process_text_async: the DMA engines read it
 * directly.  Blocks of 8 MB and more are anonymous memory on transparent huge pages, touched and registered with the runtime
 * (hipHostRegister, portable across devices) -- locking 4 KB pages goes at 4 GB/s, 370 huge pages take 13 ms for 740 MB; smaller
 * blocks, and any failure on that way, come from hipHostMalloc.  NULL when the allocation fails.  Thread-safe. */
void* fpl_host_alloc(size_t bytes);
void fpl_host_free(void* p);

/*
 * Fragment list of the LAST batch (contexts created with break_enabled or mask_enabled; otherwise the counts
 * are zero).  fpl_get_fragments synchronizes, copies the records to the host and sorts them by (read, seq_no).
 */
int fpl_fragment_counts(fpl_ctx* ctx, uint32_t* n_fragments, uint32_t* n_regions);
int fpl_get_fragments(fpl_ctx* ctx, fpl_fragment* fragments, uint32_t n_fragments, fpl_region* regions,
                      uint32_t n_regions);

/*
 * Device output for contexts with break_enabled / mask_enabled, from the fragment list.  FPL_ABI_VERSION stays 10: found by symbol
 * lookup like fpl_set_gzip_framing; a caller of a library without it formats such runs on the host, as before.
 *
 * Without the switch every device output form refuses such a context (fpl_set_bam_gzip, fpl_emit_batch_device, text batches), and
 * nothing here changes that.  With it the fragment list of the LAST batch is put in the reference's order on the device
 * (csrc/frag_index.h: place = first[read] + seq_no, no sort) and read there:
 *
 *   fpl_set_fragment_output  per context, while nothing is in flight (FPL_ERR_STATE otherwise).  On a context without
 *                      break_enabled / mask_enabled it succeeds and changes nothing.  While it is on
 *                        - fpl_set_bam_gzip succeeds, and fpl_wait_bam_gz returns the member of the batch's FRAGMENTS;
 *                        - fpl_process_text_async is admitted under the rule CSR and BAM batches have -- nothing else in flight
 *                          --, with fpl_set_text_gzip its member is the fragments' too.  The resident kinds
 *                          (fpl_process_bgzf_bam_async, fpl_process_bgzf_text_async) stay FPL_ERR_STATE;
 *                        - fpl_emit_batch_device puts out the fragments (below);
 *                        - fpl_set_gzip_records(FPL_GZIP_BAM), fpl_set_bam_tags(1) and fpl_set_bam_comments with a selection
 *                          are FPL_ERR_STATE, and the switch itself is FPL_ERR_STATE while one of them is on: those forms
 *                          stay with the host in fragment mode.
 *   The member (or the BGZF blocks, fpl_set_gzip_framing) inflates to exactly what the host's formatter writes for the batch and
 *   its fragment list (host/format.cpp, format_range with a FragmentList): per fragment with code FPL_PASS_FILTER of a read that
 *   is not dropped, in (read, seq_no) order, the name's first byte, "r<break_no>-" when break_no != 0, the split prefix by kind,
 *   the rest of the name; the bases with the fragment's regions as 'N'; the '+' line and the qualities unmasked.  Sizes as for
 *   the other gzip batches, with `fragments` the list's.  A list that overflowed (fpl_fragment_counts: FPL_ERR_CAPACITY) makes
 *   the wait FPL_ERR_CAPACITY and nothing is written.
 *
 *   fpl_emit_batch_device with the switch on: the output reads are the passing fragments of the context's LAST batch -- the lists
 *   fpl_get_fragments reads, valid until the context's next fpl_process_batch_device --, so the call belongs behind that batch
 *   on its stream, with the batch's d_seq / d_qual / d_off / n_reads.  Of d_results only `dropped` is read.  d_src[j] is the read,
 *   d_kind[j] the fragment's kind; the bases carry their 'N' (k_emit_mask runs behind the gather), the qualities do not.
 *   out_cap_reads = the fragment count's bound (2 * n_reads + bases / (break window + 1) + 16) and out_cap_bytes = d_off[n_reads]
 *   always suffice.  fpl_emit_info.status bit 2: the lists overflowed or do not index; n_out = 0 and nothing else is written.
 *   fpl_set_emit_break_no  a DEVICE array of out_cap_reads uint16 the next fpl_emit_batch_device calls fill with break_no of
 *                      every output read (with d_src and d_kind: what names it); NULL (the default): none.  Read only with the
 *                      switch on.
 */
int fpl_set_fragment_output(fpl_ctx* ctx, int on);
int fpl_set_emit_break_no(fpl_ctx* ctx, uint16_t* d_break_no);

/* Counter buffer: capacity, number of adapter slots, length, device pointer, host copy. */
uint32_t fpl_max_cycles(const fpl_ctx* ctx);
int32_t fpl_n_adapters(const fpl_ctx* ctx);
size_t fpl_counters_len(const fpl_ctx* ctx);
/* Grow the per-cycle capacity (all ranks must agree on C before an all-reduce). */
int fpl_reserve_cycles(fpl_ctx* ctx, uint32_t max_cycles);
/* int64 device buffer of fpl_counters_len() entries; valid until the next grow/destroy. A
   multi-GPU host all-reduces (sum) this buffer in place over RCCL. */
void* fpl_counters_device_ptr(fpl_ctx* ctx);
int fpl_get_counters(fpl_ctx* ctx, int64_t* host_buf, size_t n);
/*
 * The merge that follows the join in the reference (Stats::merge src/stats.cpp:1013-1082,
 * FilterResult::merge src/filterresult.cpp:28-61), for the contexts of ONE process (one per device):
 * agrees on the per-cycle capacity (max over the contexts, fpl_reserve_cycles), then sums the counter
 * buffers in place with one grouped RCCL all-reduce (int64, sum) over xGMI, so that afterwards every
 * context holds the totals.  n == 1 only reserves.  librccl is loaded on first use (dlopen), so hosts
 * that never call this do not need it.  Hosts that run one PROCESS per device all-reduce
 * fpl_counters_device_ptr() themselves (bench.py does, through torch.distributed) after agreeing on C.
 */
int fpl_allreduce_counters(fpl_ctx** ctxs, int32_t n);
/* (ABI v5) Path of the RCCL library fpl_allreduce_counters runs on: "" until a merge has needed it.  A librccl the process has
 * mapped already is taken first (PyTorch-ROCm's own), then the loader's search path, ROCm's directory and the directory of the
 * HIP runtime in use.  With FPL_RCCL_FORCE=1 in the environment a merge of ONE context goes through RCCL as well (a one-rank
 * communicator; the buffer comes out unchanged) -- the way to exercise the collective on a box with a single GPU. */
const char* fpl_rccl_library(void);
/* (ABI v5) Optional: make the RCCL communicators of these contexts' devices AHEAD of the merge and keep them -- ncclCommInitAll over
 * a node's eight devices takes far longer than the all-reduce of a few megabytes that follows, and a host can pay for it on a thread
 * of its own while its batches run (bin/fastplong_amd does).  fpl_allreduce_counters uses kept communicators when they were made
 * for exactly its devices (same order) and makes its own otherwise.  fpl_comm_init(NULL, 0) gives them back.  Thread-safe; may run
 * beside fpl_process_batch* on the same contexts. */
int fpl_comm_init(fpl_ctx** ctxs, int32_t n);

/* The counting loops of the adapter auto-detection, Evaluator::evalAdapterAndReadNum (src/evaluator.cpp:300-345), on the
 * device: for the reads of the evaluation prefix (host CSR arrays; the reference looks at <= 64 Ki reads / 512 Mbases) count
 * the 10-mers starting at the first 128 positions (side 0) or at the last 129 positions in front of the `shift_tail` skipped
 * bases (side 1).  counts / position_acc: host arrays of 4^10 entries, overwritten; *total = keys counted.  What the reference
 * does with the counters (getTopKey :268-326, extendKeyToAdapter :328-404) stays with the caller.  No context is needed: the
 * detection runs before the adapters -- and with them the contexts -- exist (src/main.cpp:270-277). */
int fpl_count_end_kmers(int32_t device, const uint8_t* seq, const uint64_t* off, uint32_t n_reads, int32_t side, int32_t shift_tail,
                        uint32_t* counts, uint64_t* position_acc, uint64_t* total);
/* ... and the whole decision on the device (fastplong_amd/csrc/adapter_pick.h): the counters stay in HBM, one more launch
 * picks the seed -- the admissible key with the largest count, Evaluator::getTopKey (src/evaluator.cpp:268-326) -- and grows it
 * into an adapter (Evaluator::extendKeyToAdapter, :328-404).  What comes back is what Evaluator::evalAdapterAndReadNum
 * (:191-222) needs for its verdict: the seed and its count, the number of keys seen, the keys counted, the grown sequence.
 * key = -1 (len 0) when no key qualifies.  is_rna: T is spelled U. */
typedef struct fpl_adapter_pick {
    int32_t key;
    uint32_t count;
    uint32_t total_key;
    int32_t len;
    uint64_t total;
    char seq[72]; /* NUL-terminated, <= 64 bases */
} fpl_adapter_pick;
int fpl_pick_adapter(int32_t device, const uint8_t* seq, const uint64_t* off, uint32_t n_reads, int32_t side, int32_t shift_tail,
                     int32_t is_rna, fpl_adapter_pick* out);
int fpl_reset_counters(fpl_ctx* ctx);
int fpl_synchronize(fpl_ctx* ctx);

/*
 * Which kernel forms the batches of a context took since fpl_create() / fpl_reset_counters() (ABI v6).  The library picks
 * per batch, by the batch's size: the end trims run in k_trim_ends_batched (64 reads per wave) from FPL_FORM_TRIM_BATCHED_MIN
 * reads on and one wave per read below, the statistics pass is k_stats_sorted (one table update per base) from
 * FPL_FORM_STATS_SORTED_MIN reads on and the two-update k_stats below (csrc/pipeline.h) -- a host that flushes small batches
 * never runs the forms a large resident batch is timed on, and this call says so.  The reference has no counterpart (its
 * unit of work is a pack of 16 reads, src/common.h:33).
 *   out[0] batches   out[1] reads   out[2] batches through k_trim_ends_batched   out[3] batches through k_stats_sorted
 *   out[4] reads of the largest batch   out[5] batches whose end trims started ahead of the main stream (fpl_assume_inputs_ready /
 *   the asynchronous path's own copy events), beside the scan of the batch before
 */
/*
 * A promise about fpl_process_batch_device (ABI v6): yes != 0 says that d_seq / d_qual / d_off of every later call are COMPLETE
 * on the device when the call is made -- resident data, or copies the caller has already waited for -- not merely ordered on
 * the call's stream.  The library then starts the end trims of a batch beside the kernels of the batch before it (they are
 * bound by memory latency, the scan and the statistics pass by instruction issue).  Without the promise only the library's own
 * asynchronous path (fpl_process_batch_async: it knows when its copies are in) does that.  Results are the same either way.
 * The promise holds until it is withdrawn (yes == 0): a caller that later hands in inputs which are only ORDERED on the call's
 * stream -- written by a kernel or a copy still in flight there -- must withdraw it first, or the trims may read them early.
 */
int fpl_assume_inputs_ready(fpl_ctx* ctx, int yes);

#define FPL_FORM_TRIM_BATCHED_MIN 65536
#define FPL_FORM_STATS_SORTED_MIN 150000
int fpl_get_batch_forms(const fpl_ctx* ctx, uint64_t out[6]);

/*
 * Per-kernel timing, measured with HIP events recorded on the stream the kernels are launched
 * on.  fpl_enable_timing(ctx, 1) starts a measurement window; every later
 * fpl_process_batch_device() records one event set (a ring of 128).  fpl_get_kernel_times()
 * waits for the recorded events and returns, per kernel, the time SUMMED over the batches of
 * the window (n_batches of them); names[i] are static strings.  The stages are those of csrc/pipeline.h (STAGE_NAMES); a stage
 * whose kernels run on one of the context's side streams -- the end trims of a batch whose inputs were known to be in (see
 * fpl_assume_inputs_ready), the post-only statistics pass of a large batch -- shows what is left of them IN LINE, not their
 * duration: withdraw the promise / set FPL_NO_OVERLAP=1 for in-line timings, or use rocprofv3's kernel table.
 */
#define FPL_MAX_KERNEL_TIMES 16
int fpl_enable_timing(fpl_ctx* ctx, int enable);
int fpl_get_kernel_times(fpl_ctx* ctx, float* ms, const char** names, int* n, int* n_batches);

const char* fpl_strerror(int code);
const char* fpl_last_error(const fpl_ctx* ctx);
int fpl_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FASTPLONG_AMD_H */
