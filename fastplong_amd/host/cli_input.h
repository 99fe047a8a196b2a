/*
 * cli_input.h -- the two looks the CLI takes at its input before the first batch: the evaluation of its first reads (RNA,
 * adapters, --split's file size) and the plan of how it is read (chunks of a mapping, one sequential reader, BAM).
 * Part of cli.cpp's translation unit.
 */
#ifndef FPLH_CLI_INPUT_H
#define FPLH_CLI_INPUT_H

#include "cli_device.h"
#include "bam_out.h"
#include "evaluator.h"
#include "fastq.h"
#include "gzip.h"
#include "pool.h"

struct InputFacts {
    bool bam = false;         /* BAM input (host/bam.h): recognised by its content; its bases are decoded on the device */
    bool isRNA = false;
    string bamReadGroups;     /* --keep_tags: the @RG lines of the input's header, as the outputs' headers repeat them */
    void* inflater = nullptr; /* --device_inflate: the first device's inflater (fpl_inflater_create) for BGZF blocks or a one-member .gz, or none */
};

/* The evaluation of the input's first reads: Evaluator::evaluateSeqLenAndCheckRNA (src/evaluator.cpp:16-61: U vs T in the
   first 100 reads), the adapter auto-detection (src/main.cpp:270-277) and --split's file size (src/main.cpp:282-293).
   An "auto" adapter that was detected and --split's size are written into `opt`. */
static InputFacts evaluate_input(Options& opt, const DeviceApi& api) {
    InputFacts in;
    in.bam = !opt.from_stdin && fplh::is_bam_file(opt.in);
    if (opt.keepTags && !in.bam) error_exit("--keep_tags needs BAM input (--in " + opt.in + " is not a BAM file)");
    if (opt.commentTags && !in.bam) error_exit("--comment_tags needs BAM input (--in " + opt.in + " is not a BAM file)");
    if (opt.reindexComments && in.bam) error_exit("--reindex_comments needs FASTQ input (--in " + opt.in + " is a BAM file: --comment_tags writes its fields as comments, re-indexed)");
    if (in.bam) {
        const DeviceApi::BamDecodeFn bamDecode = api.decode_bam;
        if (!api.process_bam_async || !bamDecode)
            error_exit("BAM input needs fpl_process_bam_async and fpl_decode_bam (C-ABI version 8), which the loaded libfastplong_amd.so lacks");
        fplh::set_bam_decoder([bamDecode](const uint8_t* bam, uint64_t nb, const uint64_t* rec, const uint64_t* of, uint32_t n, uint8_t* sq,
                                          uint8_t* ql) { return bamDecode(0, bam, nb, rec, of, n, sq, ql) == FPL_OK; });
        /* --device_inflate: the BGZF blocks are inflated on the first device (fpl_inflate_bgzf), by the reader of the
           evaluation prefix and by the main one.  A library without the three calls: the host inflates, silently, as for
           the calls of v10. */
        if (opt.deviceInflate) {
            if (api.inflater_create && api.inflate_bgzf && api.inflater_destroy) in.inflater = api.inflater_create(0);
            if (in.inflater) fplh::set_bam_inflater(api.inflate_bgzf, in.inflater);
        }
    }
    /* --device_inflate on a gzip FILE: the single-member lane of the in-memory expansion hands its member to the first device
       window by window (fpl_inflate_gzip; host/gzip.h set_gzip_inflater).  The multi-member lane, --gz_stream and pipes never
       come near it.  A library without the call: the host inflates, silently. */
    if (opt.deviceInflate && !in.bam && !opt.from_stdin && !opt.gzStream && api.inflater_create && api.inflate_gzip && api.inflater_destroy) {
        unsigned char magic[2] = {0, 0};
        if (FILE* f = fopen(opt.in.c_str(), "rb")) {
            if (fread(magic, 1, 2, f) != 2) magic[0] = 0;
            fclose(f);
        }
        if (magic[0] == 0x1f && magic[1] == 0x8b) in.inflater = api.inflater_create(0);
        if (in.inflater) fplh::set_gzip_inflater(api.inflate_gzip, in.inflater);
    }
    if (!opt.from_stdin) {
        fplh::Batch b;
        if (in.bam) {
            fplh::read_bam_prefix(opt.in, b, 100, 1L << 62);
            if (opt.keepTags) in.bamReadGroups = fplh::bam_read_group_lines(fplh::bam_prefix_header_text());
        } else {
            fplh::FastqReader ev(opt.in);
            if (!ev.ok()) error_exit("Failed to open file: " + opt.in);
            ev.fill(b, ~0ull, 100);
        }
        long numT = 0, numU = 0;
        for (uint8_t c : b.seq) {
            numT += c == 'T';
            numU += c == 'U';
        }
        if (numT > 0 && numU > 0) error_exit("This data contains both U and T");
        if (numU > 0) {
            in.isRNA = true;
            cerr << "RNA direct sequencing data" << endl;
        }
    }
    /* adapter auto-detection, src/main.cpp:270-277 (an undetected "auto" stays literal, as in the reference) */
    long readNum = 0;
    if (opt.o.adapter_enabled && (opt.startAd == "auto" || opt.endAd == "auto")) {
        if (opt.from_stdin) cerr << "Adapter auto-detection is disabled for STDIN mode" << endl;
        else {
            /* counting, seed and growth of the detection run on the first device (fpl_pick_adapter; device 0: the first of
               --gpus); the host keeps the verdict.  (FPLH_HOST_KMERS: everything on the host -- test / measurement hook) */
            if (!getenv("FPLH_HOST_KMERS"))
                fplh::set_adapter_picker([](const uint8_t* sq, const uint64_t* of, uint32_t n, int side, int shift, bool rna,
                                            fplh::AdapterVerdict& v) {
                    fpl_adapter_pick p;
                    if (fpl_pick_adapter(0, sq, of, n, side, shift, rna ? 1 : 0, &p) != FPL_OK) return false;
                    v.key = p.key;
                    v.count = p.count;
                    v.total_key = p.total_key;
                    v.total = p.total;
                    v.adapter.assign(p.seq, (size_t)(p.len > 0 ? p.len : 0));
                    return true;
                });
            fplh::detect_adapters(opt.in, opt.o.trim_tail, in.isRNA, opt.startAd, opt.endAd, &readNum);
            cerr << endl;
        }
    }
    if (opt.splitByNumber) { /* src/main.cpp:282-293: the evaluator's guess of the read count decides the file size */
        if (readNum == 0) readNum = fplh::evaluate_read_num(opt.in);
        opt.splitSize = readNum / opt.splitNumber;
        if (opt.splitSize <= 0) { /* one record per file at least */
            opt.splitSize = 1;
            cerr << "WARNING: the input file has less reads than the number of files to split" << endl;
        }
    }
    return in;
}

/* How the input is read.  A regular uncompressed file is cut into chunks of --chunk_mb that --reader_threads
   workers parse at the same time (FastqReader::parse_chunk: each worker reads its chunk from the page cache,
   locates the records and copies their lines into a page-locked batch); the pipeline's reader stage puts the chunks
   back in order and checks every chunk's guessed start against its predecessor.  Everything else -- gzip,
   pipes, --reads_to_process -- goes through the one sequential reader. */
struct InputPlan {
    int hw = 1; /* (what the scheduler lets this process use: affinity and cgroup quota) */
    uint64_t chunkBytes = 0;
    int chunkFd = -1;
    const char* chunkMem = nullptr; /* the input's text in memory (a mapping of the file / inflated gzip members) instead of a descriptor */
    bool chunkMemMapped = false;    /* ... a file mapping: its pages go back to the kernel as the reader passes them */
    uint64_t chunkFileSize = 0;
    bool chunked = false;
    bool textMode = false; /* --device_parse (the default wherever it applies): the device finds the records of every chunk */
    int readerThreads = 0;
    int nWork = 0;                        /* the size of the pipeline's Work pool */
    fplh::FastqReader* reader = nullptr;  /* neither chunks nor BAM: the sequential reader */
    fplh::BamReader* bamReader = nullptr; /* BAM input: batches of --chunk_mb of inflated records */
};

/* the uncompressed regular file behind fd, mapped: the parsers take the file's bytes in place from a mapping (18 GB of page
   cache: pipeline 0.76 -> 0.58 s against pread into per-thread windows, and no first-touch penalty on a file this process has
   not read before); the pages are handed back as the reader stage passes them.  (FPLH_NO_MMAP_INPUT: measurement hook.)  A file
   cut short under the mapping raises SIGBUS where pread would have returned an error: same message, same exit code */
static void map_input(InputPlan& p, int fd, size_t size) {
    void* m = mmap(nullptr, size, PROT_READ, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) return;
    madvise(m, size, MADV_SEQUENTIAL);
    p.chunkMem = (const char*)m;
    p.chunkMemMapped = true;
    struct sigaction sa;
    memset(&sa, 0, sizeof(sa));
    sa.sa_handler = [](int) {
        static const char msg[] = "ERROR: reading the input failed (file truncated while it was being read?)\n";
        ssize_t r = write(2, msg, sizeof(msg) - 1);
        (void)r;
        _exit(1);
    };
    sigaction(SIGBUS, &sa, nullptr);
}

/* a gzip file made of several members (bgzip, a `cat` of per-chunk files, what fastp / fastplong / this host
   write): the members are inflated side by side into anonymous memory, which the chunk parsers then take like
   a mapped file.  One deflate stream, or more text than a third of the machine's memory: the sequential
   reader and its stream.  (FPLH_NO_GZ_EXPAND: measurement / test hook) */
/* The whole text sits in memory until the parsers have passed it: it may take what the process can still get --
   MemAvailable and the cgroup's limit, whichever is smaller -- less the page-locked arena and the batches in
   flight (2 GiB), and of that no more than half; anything larger is streamed.  --gz_stream (or FPLH_NO_GZ_EXPAND)
   forces the stream. */
static void expand_gzip_input(InputPlan& p, const Options& opt) {
    const double t0 = now_s();
    const uint64_t budget = fplh::memory_budget(), hold = 2ull << 30;
    const uint64_t cap = budget > hold ? (budget - hold) / 2 : 0;
    uint64_t sz = 0, reserved = 0;
    p.chunkMem = cap ? fplh::gunzip_members_to_memory(opt.in, max(4, min(64, p.hw)), cap, &sz, &reserved) : nullptr;
    if (p.chunkMem && sz <= p.chunkBytes) { /* one chunk of text: not worth the parsers */
        munmap((void*)p.chunkMem, (size_t)reserved);
        p.chunkMem = nullptr;
    }
    uint64_t dev_windows = 0, dev_refused = 0;
    fplh::gzip_inflater_counts(&dev_windows, &dev_refused);
    if (dev_windows && opt.verbose)
        cerr << "input: gzip member inflated on the device: " << dev_windows << " windows (" << dev_refused << " refused, inflated by the host)" << endl;
    if (!p.chunkMem && opt.verbose)
        cerr << "input: gzip text not expanded in memory (" << now_s() - t0 << " s spent finding out): the sequential reader streams it" << endl;
    if (p.chunkMem) { /* (the mapping lives until the process ends) */
        p.chunkFileSize = sz;
        if (opt.verbose)
            cerr << "input: gzip members inflated into memory: " << sz << " bytes of text in " << now_s() - t0 << " s" << endl;
    }
}

static InputPlan plan_input(const Options& opt, const InputFacts& in, const DeviceApi& api) {
    InputPlan p;
    p.hw = max(1, fplh::effective_cpus());
    p.chunkBytes = (uint64_t)max(1L, opt.chunkMb) << 20;
    if (const char* e = getenv("FPLH_CHUNK_BYTES")) /* test hook: tiny chunks put every cut inside some record */
        if (atol(e) > 0) p.chunkBytes = (uint64_t)atol(e);
    if (!in.bam && !opt.from_stdin && opt.readsToProcess == 0 && !getenv("FPLH_NO_CHUNKS")) {
        const int fd = open(opt.in.c_str(), O_RDONLY);
        struct stat st;
        unsigned char magic[2] = {0, 0};
        if (fd >= 0 && fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && pread(fd, magic, 2, 0) == 2 &&
            !(magic[0] == 0x1f && magic[1] == 0x8b)) {
            p.chunkFd = fd;
            p.chunkFileSize = (uint64_t)st.st_size;
            if (!getenv("FPLH_NO_MMAP_INPUT") && p.chunkFileSize > p.chunkBytes) /* (a file of one chunk goes through the sequential reader) */
                map_input(p, fd, (size_t)st.st_size);
        } else if (fd >= 0) {
            const bool gz_file = S_ISREG(st.st_mode) && magic[0] == 0x1f && magic[1] == 0x8b;
            close(fd);
            if (gz_file && !opt.gzStream && !getenv("FPLH_NO_GZ_EXPAND") && (uint64_t)st.st_size > p.chunkBytes / 8) /* (small inputs: the stream) */
                expand_gzip_input(p, opt);
        }
    }
    /* (half of the CPUs parse, the rest formats, copies and writes; sixteen parsers feed one device's PCIe link with room to
       spare -- 4.7 GB/s of text each -- so several devices get sixteen each, as far as the CPUs go) */
    p.readerThreads = opt.readerThreads > 0 ? opt.readerThreads : max(2, min(16 * opt.nGpus, p.hw / 2));
    p.chunked = (p.chunkFd >= 0 || p.chunkMem) && p.chunkFileSize > p.chunkBytes;
    /* the chunk parsers cut the batches: one per --chunk_mb of text; --batch_mbases / --batch_reads only size the batches
       of the sequential reader (pipes, streamed gzip, --reads_to_process) */
    if (p.chunked && opt.batchSizeGiven)
        cerr << "WARNING: --batch_mbases / --batch_reads do not apply to this input: its batches are the chunks of --chunk_mb ("
             << (p.chunkBytes >> 20) << " MB of text each); lower --chunk_mb for smaller batches" << endl;
    /* Work objects bound what is in flight: one per parser, FPL_MAX_IN_FLIGHT per device in the copy / kernel stage,
       one per device being formatted, two waiting for the writer */
    const bool gzOut = !opt.splitEnabled && (ends_with_gz(opt.out) || ends_with_gz(opt.failedOut) || ends_with_bam(opt.out) || ends_with_bam(opt.failedOut)); /* (then up to four batches are formatted at a time) */
    /* (+ FPLH_EXTRA_WORK, default 6: with exactly as many as the stages can hold, a parser waits for a Work object while the writer
       or a formatter still holds one, and the device thread finds its queue empty -- the link then idles between two uploads) */
    const int extraWork = getenv("FPLH_EXTRA_WORK") ? atoi(getenv("FPLH_EXTRA_WORK")) : 6;
    p.nWork = (p.chunked ? p.readerThreads : 1) + (FPL_MAX_IN_FLIGHT + 1) * opt.nGpus + 2 + (gzOut ? 3 : 0) + (p.chunked ? max(0, extraWork) : 0);
    /* --device_parse: the chunk parsers only LOAD the file's bytes (page-locked), the device finds the records
       (fpl_process_text_async); --break / --mask keep the host's reader (their fragment lists come back batch by batch through
       the CSR entry points) unless --device_gzip has the device write their output, and so do inputs that are not cut into chunks (pipes, a streamed gzip, a small file) */
    /* (the default wherever it applies; --host_parse keeps the host's parsers, --device_parse only says so out loud) */
    if (opt.deviceParse && opt.hostParse) error_exit("--device_parse and --host_parse exclude each other");
    /* (--break / --mask with --device_gzip, where the device may write the output: fpl_set_fragment_output lets text batches in) */
    p.textMode = !opt.hostParse && !getenv("FPLH_HOST_PARSE") && p.chunked && (!opt.fragmentMode || fragment_device_out(opt, api)) &&
                 p.chunkBytes < (3ull << 30);
    if (opt.deviceParse && !p.textMode && opt.verbose)
        cerr << "input: --device_parse does not apply (it needs an uncompressed file or multi-member gzip cut into chunks, --chunk_mb below 3072, --break / --mask only with --device_gzip and a .gz output): the host parses" << endl;
    if (p.chunked && p.textMode) /* one block holds a chunk's text and the stretch behind it that the last record may run into */
        fplh::ByteBuf::set_arena((size_t)(p.chunkBytes + (5u << 20)), (size_t)p.nWork);
    else if (p.chunked) /* a chunk holds about half its bytes in bases: one block each for the bases and the qualities of a batch */
        fplh::ByteBuf::set_arena((size_t)(p.chunkBytes / 2 + p.chunkBytes / 16 + (2u << 20)), 2 * (size_t)p.nWork);
    if (in.bam) {
        p.bamReader = new fplh::BamReader(opt.in);
        if (!p.bamReader->ok()) error_exit("Failed to open file: " + opt.in);
        if (in.inflater) p.bamReader->set_inflater(api.inflate_bgzf, in.inflater);
        p.bamReader->set_check_tags(opt.keepTags || opt.commentTags);
    } else if (!p.chunked) {
        p.reader = new fplh::FastqReader(opt.in);
        if (!p.reader->ok()) error_exit("Failed to open file: " + opt.in);
        /* threads of the reader's refill / locate / copy phases (FPLH_PARSE_THREADS overrides) */
        const char* e = getenv("FPLH_PARSE_THREADS");
        p.reader->set_copy_threads(e && atoi(e) > 0 ? atoi(e) : max(1, min(8, p.hw / 2)));
    }
    return p;
}

#endif
