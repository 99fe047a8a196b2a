/*
 * cli_pipeline.h -- the host pipeline of `fastplong_amd`: batches in input order through four stages,
 *   reader (one thread: parse or load) -> device (one thread per device: copies and kernels) -> format (helper threads:
 *   the output text) -> writer (the calling thread: writes in input order, plans --split*).
 * Pipeline owns what the stages share; every stage is one of its member functions, and DeviceStage is the state machine
 * of one device thread.  Part of cli.cpp's translation unit.
 */
#ifndef FPLH_CLI_PIPELINE_H
#define FPLH_CLI_PIPELINE_H

#include "cli_input.h"
#include "cli_output.h"
#include "fastq.h"
#include "report.h"
#include "split.h"

/* One batch on its way through the host pipeline:
 *   reader thread (parse into CSR) -> one thread per device (fpl_process_batch, then the output text on a few
 *   helper threads) -> the main thread (writes the pieces in input order).
 * Where the reference's workers hand strings to WriterThread (src/seprocessor.cpp:283-313), the stages here
 * hand whole batches; a small pool of Work objects bounds what is in flight. */
struct Work {
    uint64_t seq_no = 0;
    fplh::Batch batch;
    vector<fpl_read_result> res;
    fplh::FragmentList frags; /* --break / --mask */
    vector<string> outs, faileds;
    vector<fplh::BamTagSrc> outTags, failedTags; /* --keep_tags: where the records of outs / faileds take their auxiliary fields from */
    vector<fplh::FqCommentSrc> outNotes, failedNotes; /* --reindex_comments: which input read and range every record of outs / faileds is */
    string gz_member;  /* --out *.gz deflated on the device (fpl_wait_text_gz): this batch's gzip member, written as it is */
    bool dev_gz = false;
    bool dev_gz_empty = false; /* a gzip BAM batch in which nothing passed: --out gets nothing, and the decoded arrays may never have come back */
    vector<struct iovec> gather; /* --out as a gather list over the batch's own arrays (plain output, see build_gather) */
    string gather_text;          /* the few bytes of it that exist nowhere yet: names with a split prefix */
    int rc = 0;
    string err;
    std::atomic<int> holders{0}; /* --split*: the per-worker writer threads that still read this batch (+ the in-order thread) */
    bool verdict_done = false;   /* --device_parse: this batch's verdict is published (a chunk that came back from the host's reader is submitted a second time) */
};
/* The passing reads of a batch as they go to --out (Read::appendToString, src/read.cpp:119-143), NOT copied together: every
 * line is a slice of what the batch already holds -- names and '+' lines in Batch::text, bases and qualities in the
 * page-locked arrays -- so the writer hands the kernel a gather list (writev) instead of a second copy of the data.
 * Formatting 18 GB of output text was 4.5 of the pipeline's 9 CPU-seconds, and the CPU quota is what bounds it.
 * (Plain --out only: gzip members, --failed_out, --split* and --break / --mask output go through format_batch_parallel.) */
static void build_gather(const fplh::Batch& b, const fpl_read_result* res, vector<struct iovec>& iov, string& text,
                         uint32_t first = 0, uint32_t last = ~0u) {
    static const char* prefix[3] = {"", "split-by-adapter-left-", "split-by-adapter-right-"}; /* src/read.cpp:199,208 */
    static const char nl_byte = '\n';
    const uint32_t n = min(last, b.n());
    iov.clear();
    text.clear();
    size_t need = 0; /* bytes of prefixed names: reserved up front, the list points into the string */
    for (uint32_t i = first; i < n; i++) {
        const fpl_read_result& r = res[i];
        if (r.dropped) continue;
        for (int f = 0; f < r.n_frag; f++)
            if (r.code[f] == FPL_PASS_FILTER && r.kind[f] >= 1 && r.kind[f] <= 2 && b.name_len[i] > 0)
                need += b.name_len[i] + strlen(prefix[r.kind[f]]);
    }
    text.reserve(need + 1);
    auto put = [&](const void* p, size_t len) {
        struct iovec v;
        v.iov_base = const_cast<void*>(p);
        v.iov_len = len;
        iov.push_back(v);
    };
    for (uint32_t i = first; i < n; i++) {
        const fpl_read_result& r = res[i];
        if (r.dropped) continue;
        const char* name = b.name_ptr(i);
        const uint32_t nl = b.name_len[i], sl = b.strand_len[i];
        const char* strand = b.strand_ptr(i);
        const uint8_t* sq = b.seq_ptr(i);
        const uint8_t* ql = b.qual_ptr(i);
        for (int f = 0; f < r.n_frag; f++) {
            if (r.code[f] != FPL_PASS_FILTER) continue;
            const char* pf = prefix[r.kind[f] <= 2 ? r.kind[f] : 0];
            if (*pf && nl > 0) { /* name->insert(1, prefix) */
                const size_t at = text.size();
                text.append(name, 1);
                text.append(pf);
                text.append(name + 1, nl - 1);
                put(text.data() + at, text.size() - at);
            } else {
                put(name, nl);
            }
            put(&nl_byte, 1);
            put(sq + r.frag_start[f], r.frag_len[f]);
            put(&nl_byte, 1);
            put(strand, sl);
            put(&nl_byte, 1);
            put(ql + r.frag_start[f], r.frag_len[f]);
            put(&nl_byte, 1);
        }
    }
}
/* all of a gather list to fd (writev takes 1024 entries and about 2 GiB at a time, and may stop short) */
static bool write_gather(int fd, vector<struct iovec>& iov) {
    size_t k = 0;
    while (k < iov.size()) {
        const int cnt = (int)min<size_t>(1024, iov.size() - k);
        ssize_t w = writev(fd, iov.data() + k, cnt);
        if (w < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        while (w > 0 && k < iov.size()) { /* skip what went out, trim the entry it stopped in */
            if ((size_t)w >= iov[k].iov_len) {
                w -= (ssize_t)iov[k].iov_len;
                k++;
            } else {
                iov[k].iov_base = (char*)iov[k].iov_base + w;
                iov[k].iov_len -= (size_t)w;
                w = 0;
            }
        }
        while (k < iov.size() && iov[k].iov_len == 0) k++;
    }
    return true;
}

template <class T>
class Channel {
   public:
    void push(T v) {
        { lock_guard<mutex> g(m_); q_.push_back(v); }
        cv_.notify_one();
    }
    T pop() { /* blocks */
        unique_lock<mutex> g(m_);
        cv_.wait(g, [&] { return !q_.empty(); });
        T v = q_.front();
        q_.pop_front();
        return v;
    }
    bool try_pop(T& v) {
        lock_guard<mutex> g(m_);
        if (q_.empty()) return false;
        v = q_.front();
        q_.pop_front();
        return true;
    }
   private:
    mutex m_;
    condition_variable cv_;
    deque<T> q_;
};

/* --device_parse: the reference stops READING at a malformed record (FastqReader::read returns NULL, src/fastqreader.cpp:326-341),
   so nothing behind one may be counted -- but a chunk's verdict comes from its device, and the chunks of several devices are
   under way side by side.  Every chunk's verdict is published here (fpl_peek_text: the parse only, nothing counted yet), and a
   chunk's per-read kernels are let go (fpl_wait_text; a CSR batch: its submission) only when every chunk in front of it was
   good; a chunk behind a malformed record is dropped (fpl_cancel_text).  Waits only ever look at smaller sequence numbers. */
struct Verdicts {
    mutex m;
    condition_variable cv;
    vector<uint8_t> v; /* 0 unknown, 1 good, 2 holds a malformed record */
    uint64_t frontier = 0, bad = ~0ull;
    string bad_text;
    void publish(uint64_t j, bool good, const string& text = string()) {
        {
            lock_guard<mutex> g(m);
            if (v.size() <= j) v.resize(j + 1, 0);
            v[j] = good ? 1 : 2;
            if (!good && j < bad) {
                bad = j;
                bad_text = text;
            }
            while (frontier < v.size() && v[frontier] == 1) frontier++;
        }
        cv.notify_all();
    }
    bool wait_before(uint64_t j) { /* true: a chunk in front of j holds a malformed record -- j is not part of the input */
        unique_lock<mutex> g(m);
        cv.wait(g, [&] { return frontier >= j || bad < j; });
        return bad < j;
    }
};

/* --verbose, per device thread: seconds in copies + kernels (waits), seconds inside the submissions, seconds with nothing in
   flight and nothing parsed (starved), how often the queue was empty when there was room for another batch, and how deep the
   submissions found the pipeline */
struct DeviceTimes {
    double tGpu = 0, tSubmit = 0, tStarved = 0;
    uint64_t nMiss = 0, nSubmit = 0, depthSum = 0;
};

struct Pipeline {
    Pipeline(const Options& opt, const DeviceApi& api, const InputFacts& facts, InputPlan& in, Outputs& out, const vector<fpl_ctx*>& ctxs);
    /* all four stages, from the first batch to the last byte of --out; the calling thread is the writer */
    void run();

    /* ---- fixed before the first thread starts: every stage reads it */
    const Options& opt;
    const DeviceApi& api;
    const InputFacts& facts;
    InputPlan& in;
    Outputs& out;
    const vector<fpl_ctx*>& ctxs;
    const int nGpus;
    bool devGz = false;         /* --out *.gz: text batches come back with their gzip member (fpl_wait_text_gz) */
    bool devBamGz = false;      /* ... BAM-backed batches do (fpl_wait_bam_gz) */
    bool devBgzf = false;       /* --bgzf: ... and those bytes are BGZF blocks (fpl_set_gzip_framing) */
    bool devBamOut = false;     /* --out *.bam: ... and they are BAM records in BGZF blocks (fpl_set_gzip_records) */
    bool bamKeepArrays = true;  /* a BAM batch's decoded bases are copied back to the host */
    int nFmt = 1, fmtThreads = 1;
    bool splitThreads = false;  /* --split*: the workers' writers have threads of their own */
    double tStart = 0;

    /* ---- shared between the stages: synchronised in themselves */
    vector<Work> pool;
    Channel<Work*> freeq;         /* writer (split workers) / reader -> reader: Work objects nobody holds */
    vector<Channel<Work*>> devq;  /* reader -> device thread d */
    Channel<Work*> fmtq;          /* device threads -> formatters */
    Channel<Work*> doneq;         /* formatters -> writer */
    Verdicts verdicts;
    std::atomic<bool> stopInput{false};  /* a device thread found a malformed record: the reader stops cutting chunks */
    std::atomic<uint64_t> nTextBatches{0}, nTextFallbacks{0}; /* --device_parse: chunks the device parsed / chunks handed back to the host's reader */
    std::atomic<uint64_t> nDevGz{0};
    std::atomic<uint64_t> nDevBgzf{0}; /* --bgzf: BGZF blocks the device framed */
    std::atomic<int> devEnded{0};

    /* ---- written by the reader thread alone (read after it is joined) */
    long readsLeft = -1;
    uint64_t nBatches = 0;
    double tParse = 0, tRedo = 0;
    uint64_t nRedo = 0;
    string inputError; /* a malformed record: reported the way the sequential reader does, the input ends there */
    string ioError;    /* the input could not be read / decompressed to its end: the run fails (src/fastqreader.cpp:92-137) */

    /* ---- element d: written by device thread d alone; element f: by formatter f alone */
    vector<DeviceTimes> devTimes;
    vector<double> tFormat;

    /* ---- written by the writer (the thread inside run()) alone */
    double tWrite = 0;
    fplh::HtmlInputs page; /* per-read lengths and median qualities: what Stats keeps beyond the counters */
    uint64_t readBase = 0; /* the input index of the next batch's first read */
    long packReads = 0, packPassed = 0; /* the pack of 16 input reads under way (it may straddle two batches) */

   private:
    void enable_device_gzip();
    void reader_stage();
    void read_sequential();
    void read_chunks();
    void device_stage(int d);
    void format_stage(int f);
    void writer_stage();
    void release(Work* w) {
        if (--w->holders == 0) freeq.push(w);
    }
    void note_reads(const Work& w);
    void split_reads(Work* wp);
    void finish_split();
};

Pipeline::Pipeline(const Options& opt_, const DeviceApi& api_, const InputFacts& facts_, InputPlan& in_, Outputs& out_,
                   const vector<fpl_ctx*>& ctxs_)
    : opt(opt_), api(api_), facts(facts_), in(in_), out(out_), ctxs(ctxs_), nGpus(opt_.nGpus), pool((size_t)in_.nWork), devq((size_t)opt_.nGpus) {
    readsLeft = opt.readsToProcess > 0 ? opt.readsToProcess : -1;
    enable_device_gzip();
    /* formatter stage threads: one per device -- or four when the output is deflated, each with a quarter of the helpers:
       a batch of one chunk (32 MB of text) cut into 64 members keeps 64 helpers busy for a few milliseconds between two
       thread hand-offs (measured: 25 ms per batch, 1.3 GB/s), four batches side by side in 16 members each do not wait
       for one another */
    /* (slices a batch's output is formatted in: one worker each; gzip outputs are deflated per slice, which is compute-
       bound, so they get more, smaller slices) */
    const bool anyGz = out.any_gz();
    nFmt = anyGz ? max(nGpus, 4) : nGpus;
    fmtThreads = max(1, min(anyGz ? max(8, 64 / nFmt * nGpus) : 16, in.hw / max(1, nGpus) - 1));
    for (auto& w : pool) freeq.push(&w);
    devTimes.resize((size_t)nGpus);
    tFormat.assign((size_t)nFmt, 0);
    page.threads = opt.workers;
    page.title = opt.reportTitle;
    splitThreads = out.split && !getenv("FPLH_SPLIT_ONE_THREAD"); /* (test hook: the replay on the writer's thread) */
    tStart = now_s();
}

/* --out *.gz: the device composes and deflates the passing reads of every chunk IT parsed (fpl_set_text_gzip /
   fpl_wait_text_gz, C-ABI version 9) and the writer appends the member; a chunk that falls back to the host's reader, and a
   batch the library makes no member for, is formatted and deflated here as before -- members are self-contained, so the
   two kinds mix in one file.  -z 5..9 ask for a smaller file than a Huffman-only coder gives and keep the host's deflate;
   so do --failed_out's own file, --split*, --break / --mask without --device_gzip, --host_parse, --host_gzip.
   A library without the entry points (DeviceApi): the host's deflate, without a word. */
void Pipeline::enable_device_gzip() {
    bool eligible = out.fout && out.fout.gz && !out.split && !opt.hostGzip && opt.compression <= 4;
    /* --reindex_comments: the name lines of FASTQ text are the host's to rewrite -- there is no device form of the flag --, so the
       host formats and deflates every batch of such a run, with or without --device_gzip.  (A .bam output cuts its names at the
       first tab and stays as it is.) */
    if (opt.reindexComments && !(out.fout && out.fout.bam)) eligible = false;
    /* --break / --mask: only with --device_gzip, FASTQ text only, and only where every context takes fpl_set_fragment_output (the
       device then composes from the fragment lists; the host still fetches them for the reports and --failed_out) */
    if (opt.fragmentMode) {
        const bool on = eligible && fragment_device_out(opt, api) && !out.fout.bam && enable_on_all(api.set_fragment_output, true, ctxs);
        if (!on && in.textMode) error_exit("--break / --mask: the device cannot write this output (fpl_set_fragment_output refused)");
        eligible = on;
    }
    /* --bgzf: under the same conditions the device frames its batches as BGZF blocks; a library without fpl_set_gzip_framing
       makes members only, so the host deflates and frames everything, without a word */
    /* --out *.bam: the device form under the conditions of a .gz output WITH --device_gzip, for text batches and BAM-backed ones
       alike (README "BAM output": not the default until whole-run numbers exist); a library without fpl_set_gzip_records leaves
       everything to the host, without a word.  Records are BGZF by themselves: --bgzf changes nothing for them. */
    const bool bamOut = out.fout && out.fout.bam;
    /* --keep_tags: the device form needs fpl_set_bam_tags besides; against a library without it the host writes every record */
    if (bamOut && opt.keepTags) eligible = eligible && api.set_bam_tags != nullptr;
    /* --keep_mods: ... and fpl_set_bam_mods, in the same way */
    if (bamOut && opt.keepMods) eligible = eligible && api.set_bam_mods != nullptr;
    /* --keep_moves: ... and fpl_set_bam_moves */
    if (bamOut && opt.keepMoves) eligible = eligible && api.set_bam_moves != nullptr;
    if (bamOut) eligible = eligible && opt.deviceGzip && (in.textMode || facts.bam) && (devBamOut = frame_on_all(api.set_gzip_records, ctxs));
    if (bamOut && opt.keepTags && devBamOut &&
        !(enable_on_all(api.set_bam_tags, true, ctxs) && (!opt.keepMods || enable_on_all(api.set_bam_mods, true, ctxs)) &&
          (!opt.keepMoves || enable_on_all(api.set_bam_moves, true, ctxs)))) { /* (a context refused: the host's form) */
        for (fpl_ctx* c : ctxs) (void)api.set_gzip_records(c, FPL_GZIP_FASTQ);
        eligible = devBamOut = false;
    }
    if (eligible && !bamOut && opt.bgzf && (in.textMode || (facts.bam && opt.deviceGzip))) eligible = devBgzf = frame_on_all(api.set_gzip_framing, ctxs);
    if (eligible && in.textMode) devGz = enable_on_all(api.set_text_gzip, api.wait_text_gz != nullptr, ctxs);
    /* the same for BAM input (fpl_set_bam_gzip / fpl_wait_bam_gz, C-ABI version 10): the device composes the member from the
       records' names and the bases it decoded, under the same conditions with "parsed on the device" replaced by "BAM-backed
       batch" -- and with --device_gzip asked for: whether this form beats the host's deflate beside the BGZF inflate on the
       same CPUs has not been measured, so a BAM run keeps the host's path unless told otherwise.  Without --failed_out the
       decoded arrays are not even copied back (seq_out / qual_out NULL): the host formats nothing of such a batch. */
    /* --comment_tags: the device's FASTQ form of a BAM-backed batch needs fpl_set_bam_comments besides; against a library without
       it, or where a context refuses the list, the host formats every batch, without a word */
    if (eligible && facts.bam && opt.deviceGzip && opt.commentTags && !bamOut) {
        bool on = api.set_bam_comments != nullptr;
        for (size_t d = 0; on && d < ctxs.size(); d++)
            on = api.set_bam_comments(ctxs[d], (const char*)opt.commentSel.tag, opt.commentSel.n) == FPL_OK;
        if (!on)
            for (size_t d = 0; api.set_bam_comments && d < ctxs.size(); d++) (void)api.set_bam_comments(ctxs[d], nullptr, 0);
        eligible = on;
    }
    if (eligible && facts.bam && opt.deviceGzip) devBamGz = enable_on_all(api.set_bam_gzip, api.wait_bam_gz != nullptr, ctxs);
    bamKeepArrays = !devBamGz || out.ffail; /* (--failed_out is formatted on the host: it needs the decoded bases) */
    devBgzf = devBgzf && (devGz || devBamGz);
    devBamOut = devBamOut && (devGz || devBamGz);
    if (bamOut && opt.verbose)
        cerr << "output: BAM records" << (devBamOut ? ", packed and deflated on the device (a batch that falls back: by the host)" : ", packed and deflated by the host") << endl;
    if ((devGz || devBamGz) && !opt.bgzf && !bamOut && opt.verbose) cerr << "output: gzip members deflated on the device" << endl;
    if (opt.bgzf && !bamOut && opt.verbose)
        cerr << "output: BGZF blocks" << (devBgzf ? ", deflated and framed on the device (a batch that falls back: by the host)" : ", deflated and framed by the host") << endl;
}

/* ---- stage 1: batches in input order -> devq (round-robin over the devices) */
void Pipeline::reader_stage() {
    if (in.chunked && !in.bamReader) read_chunks();
    else read_sequential();
    for (int d = 0; d < nGpus; d++) devq[d].push(nullptr);
}

/* the one sequential reader: BAM (batches of --chunk_mb of inflated records), or FASTQ that is not cut into chunks
   (batches of --batch_mbases / --batch_reads) */
void Pipeline::read_sequential() {
    fplh::BamReader* const bam = in.bamReader;
    for (;;) {
        uint32_t maxReads = bam ? 0x3FFFFFFFu : opt.batchReads;
        if (readsLeft >= 0) maxReads = (uint32_t)min<long>(readsLeft, maxReads);
        if (maxReads == 0) break;
        Work* w = freeq.pop();
        w->batch.clear();
        const double t0 = now_s();
        const uint32_t got = bam ? bam->fill(w->batch, in.chunkBytes, maxReads) : in.reader->fill(w->batch, opt.batchBases, maxReads);
        tParse += now_s() - t0;
        if (got == 0) {
            freeq.push(w);
            break;
        }
        if (readsLeft >= 0) readsLeft -= w->batch.n();
        w->seq_no = nBatches++;
        devq[w->seq_no % nGpus].push(w); /* batches are dealt round-robin in input order */
    }
    if (bam) {
        if (!bam->warning().empty()) cerr << bam->warning() << endl;
        if (!bam->error().empty()) ioError = bam->error();
    } else if (in.reader->input_error()) {
        ioError = in.reader->input_error_text();
    }
}

void Pipeline::read_chunks() {
    /* the parsers take their batches from the Work pool; next() puts the chunks back in input order */
    auto acquire = [&]() {
        fplh::ChunkedReader::Item it;
        Work* w = freeq.pop();
        w->verdict_done = false;
        it.batch = &w->batch;
        it.token = w;
        return it;
    };
    auto give_back = [&](fplh::ChunkedReader::Item it) { freeq.push((Work*)it.token); };
    fplh::ChunkedReader cr(in.chunkFd, in.chunkFileSize, in.chunkBytes, in.readerThreads, acquire, give_back, in.chunkMem, in.textMode);
    fplh::ChunkedReader::Item it;
    uint64_t unmapped = 0;
    while (cr.next(it)) {
        Work* w = (Work*)it.token;
        if (stopInput.load()) { /* (--device_parse: a device found a malformed record in an earlier chunk) */
            freeq.push(w);
            break;
        }
        w->seq_no = nBatches++;
        devq[w->seq_no % nGpus].push(w);
        if (in.chunkMem) { /* pages no parser looks at again (unmapping 18 GB at exit costs 0.2 s of process time) */
            const uint64_t dead = cr.dead_below() & ~(uint64_t)((2u << 20) - 1);
            if (dead > unmapped) {
                if (in.chunkMemMapped) munmap((void*)(in.chunkMem + unmapped), (size_t)(dead - unmapped));
                else madvise((void*)(in.chunkMem + unmapped), (size_t)(dead - unmapped), MADV_DONTNEED);
                unmapped = dead;
            }
        }
    }
    inputError = cr.malformed_text();
    ioError = cr.io_error_text();
    nRedo = cr.chunks_parsed_again();
    tRedo = cr.redo_seconds();
    tParse = cr.busiest_parser_seconds();
}

/* ---- stage 2, one thread per device: copies and kernels, FPL_MAX_IN_FLIGHT batches deep.
   A text batch (the device parses) goes through three calls: its submission (upload + parse), its APPROVAL (the parse's
   verdict, published for the other devices' threads; then fpl_start_text: the per-read kernels) and its wait.  The loop
   approves batch k + 1 before it waits for batch k, so the device's queue holds the next batch's kernels while this thread
   sits in the wait, and the thread's own time in the runtime (some thirty calls per batch) overlaps the device's.
   Everything in here belongs to the one device thread; what it shares with the others goes through Pipeline's channels,
   Verdicts and atomics. */
class DeviceStage {
   public:
    DeviceStage(Pipeline& p, int d)
        : p(p), ctx(p.ctxs[(size_t)d]), devq(p.devq[(size_t)d]), t(p.devTimes[(size_t)d]), fragmentMode(p.opt.fragmentMode),
          textMode(p.in.textMode), depth(fragmentMode ? 1 : FPL_MAX_IN_FLIGHT) {}
    void run();

   private:
    enum State { TEXT_PENDING, TEXT_STARTED, TEXT_DROPPED, TEXT_HANDED_BACK, CSR };
    struct Flight {
        Work* w;
        int state;
    };
    Pipeline& p;
    fpl_ctx* const ctx;
    Channel<Work*>& devq;
    DeviceTimes& t;
    const bool fragmentMode, textMode;
    const size_t depth;
    deque<Flight> inflight; /* in the order of submission: the library's slots are a FIFO */
    deque<Work*> redo;      /* chunks the host's reader took: in again as CSR batches */
    bool open = true;       /* the reader's end marker has not come yet */

    void fail(Work* w, int rc) {
        w->rc = rc;
        if (w->err.empty()) w->err = string(fpl_strerror(rc)) + " " + fpl_last_error(ctx);
    }
    static void make_empty(Work* w) { /* an empty batch, as the reader makes them */
        w->batch.clear();
        w->batch.off.push_back(0);
        w->batch.name_off.push_back(0);
        w->res.clear();
    }
    /* --out is this batch's gzip member as the device made it (copied out of the context's buffer, which the next wait reuses) */
    void take_member(Work* w, const uint8_t* gzp, uint64_t gzn) {
        w->gz_member.assign((const char*)gzp, (size_t)gzn);
        w->dev_gz = true;
        if (p.devBgzf || p.devBamOut) { /* (BSIZE at byte 16 of every block: the device's blocks all have the 18-byte header) */
            uint64_t blocks = 0;
            for (uint64_t at = 0; at + 18 <= gzn; at += 1u + gzp[at + 16] + 256u * gzp[at + 17]) blocks++;
            p.nDevBgzf += blocks;
        }
        p.nDevGz++;
    }
    size_t n_pending() const {
        size_t n = 0;
        for (auto& x : inflight) n += x.state == TEXT_PENDING;
        return n;
    }
    void finish_all() {
        while (!inflight.empty()) finish_oldest();
    }
    bool approve_next();
    void finish_oldest();
    void finish_csr(Work* w);
    void fetch_fragments(Work* w);
    void finish_text(Work* w, int state);
    Work* take();
    void submit(Work* w);
};

/* the oldest text batch that is still pending: verdict first, then its kernels -- or not.  false: none is pending */
bool DeviceStage::approve_next() {
    Flight* f = nullptr;
    for (auto& x : inflight)
        if (x.state == TEXT_PENDING) {
            f = &x;
            break;
        }
    if (!f) return false;
    const double t0 = now_s();
    Work* w = f->w;
    fplh::Batch& b = w->batch;
    fpl_text_result tr;
    bool good = true, to_csr = false;
    string bad_text;
    int rc = fpl_peek_text(ctx, &tr);
    if (rc == FPL_OK && tr.status != FPL_TEXT_OK) {
        /* irregular text (blank lines, a lone \r, no line break at the end, a record the reference would stop at):
           nothing of it was counted -- the host's reader takes the chunk, by the reference's rules */
        rc = fpl_cancel_text(ctx);
        fplh::FastqReader::ChunkInfo ci;
        vector<char> window;
        const uint64_t len = b.raw_len;
        const char* base = (const char*)b.raw.data() + b.raw_begin;
        b.text_backed = false;
        fplh::FastqReader::parse_chunk(-1, len, 0, len, true, window, b, ci, 1, base);
        p.nTextFallbacks++;
        to_csr = true;
        if (ci.status == 3) { /* the input ends at this record, as with the host's reader; what the chunk holds in front of it counts */
            good = false;
            bad_text = ci.err;
            p.stopInput = true;
        }
    }
    p.verdicts.publish(w->seq_no, good, bad_text);
    const bool drop = p.verdicts.wait_before(w->seq_no);
    if (rc != FPL_OK) { /* (the run fails with this batch's error) */
        if (!to_csr) (void)fpl_cancel_text(ctx);
        fail(w, rc);
        f->state = TEXT_DROPPED;
    } else if (drop) { /* behind a malformed record: not part of the input */
        if (!to_csr) rc = fpl_cancel_text(ctx);
        make_empty(w);
        if (rc != FPL_OK) fail(w, rc);
        f->state = TEXT_DROPPED;
    } else if (to_csr) {
        if (b.n() > 0) { /* in again, as a CSR batch; the cancelled slot stays in the FIFO until its turn */
            w->res.resize(b.n());
            w->verdict_done = true;
            redo.push_back(w);
            f->w = nullptr;
            f->state = TEXT_HANDED_BACK;
        } else {
            make_empty(w);
            f->state = TEXT_DROPPED;
        }
    } else {
        rc = fpl_start_text(ctx);
        if (rc != FPL_OK) fail(w, rc);
        f->state = TEXT_STARTED;
    }
    t.tGpu += now_s() - t0;
    return true;
}

/* the results of the oldest batch in flight; then it is the formatters' */
void DeviceStage::finish_oldest() {
    if (inflight.front().state == TEXT_PENDING) approve_next(); /* (the oldest pending batch is this one) */
    const Flight f = inflight.front();
    inflight.pop_front();
    const double t0 = now_s();
    if (f.state == CSR) finish_csr(f.w);
    else finish_text(f.w, f.state);
    t.tGpu += now_s() - t0;
    if (f.w) p.fmtq.push(f.w);
}

void DeviceStage::finish_csr(Work* w) {
    if (w->rc == FPL_OK) {
        const bool member = p.devBamGz && w->batch.bam_backed;
        const uint8_t* gzp = nullptr;
        uint64_t gzn = 0;
        const int rc = member ? p.api.wait_bam_gz(ctx, &gzp, &gzn) : fpl_wait(ctx);
        if (rc != FPL_OK) fail(w, rc);
        else if (gzn) take_member(w, gzp, gzn);
        else if (member) w->dev_gz_empty = true; /* no member: nothing of this batch passed */
    }
    if (w->rc == FPL_OK && fragmentMode) fetch_fragments(w);
}

/* --break / --mask, any number of output reads per read: the list of the batch just waited for */
void DeviceStage::fetch_fragments(Work* w) {
    uint32_t nf = 0, nr = 0;
    int rc = fpl_fragment_counts(ctx, &nf, &nr);
    if (rc == FPL_OK) {
        w->frags.frags.resize(nf);
        w->frags.regs.resize(nr);
        rc = fpl_get_fragments(ctx, w->frags.frags.data(), nf, w->frags.regs.data(), nr);
        w->frags.index(w->batch.n());
    }
    if (rc != FPL_OK) fail(w, rc);
}

/* (a slot that was cancelled -- dropped, or handed back with w == nullptr -- is waited for all the same: the library's
   slots are a FIFO) */
void DeviceStage::finish_text(Work* w, int state) {
    fpl_text_result tr;
    const fpl_read_result* rr = nullptr;
    const uint32_t* ls = nullptr;
    const uint8_t* gzp = nullptr;
    uint64_t gzn = 0;
    const int rc = p.devGz ? p.api.wait_text_gz(ctx, &tr, &rr, &ls, &gzp, &gzn) : fpl_wait_text(ctx, &tr, &rr, &ls);
    if (state == TEXT_STARTED && w->rc == FPL_OK) {
        if (rc != FPL_OK) fail(w, rc);
        else if (tr.status != FPL_TEXT_OK) fail(w, FPL_ERR_STATE); /* (the verdict was "good") */
        else {
            w->res.assign(rr, rr + tr.n_reads);
            w->batch.adopt_lines(ls, tr.n_reads);
            p.nTextBatches++;
            if (gzn) take_member(w, gzp, gzn); /* (no member: nothing passed, or the library makes none -- the formatter's turn) */
            if (fragmentMode) fetch_fragments(w); /* (the reports and --failed_out work from the list) */
        }
    } else if (w && rc != FPL_OK && w->rc == FPL_OK) {
        fail(w, rc);
    }
}

/* the next batch to submit: one that came back from the host's reader first, else the reader's next -- waiting for it only
   when nothing is in flight.  nullptr: none right now (or the reader's end marker: none ever again) */
Work* DeviceStage::take() {
    Work* w = nullptr;
    if (!redo.empty()) {
        w = redo.front();
        redo.pop_front();
        return w;
    }
    if (!open) return nullptr;
    if (inflight.empty()) {
        const double ts = now_s();
        w = devq.pop();
        t.tStarved += now_s() - ts;
    } else if (!devq.try_pop(w)) { /* nothing parsed yet: go on with what is in flight meanwhile */
        t.nMiss++;
        return nullptr;
    }
    if (!w) open = false;
    return w;
}

/* upload + parse (text), upload + decode + kernels (BAM), upload + kernels (CSR): the batch joins the batches in flight, or,
   where nothing was enqueued for it, goes on to the formatters in its place in the order */
void DeviceStage::submit(Work* w) {
    w->res.resize(w->batch.n());
    w->err.clear();
    w->rc = FPL_OK;
    w->dev_gz = false;
    w->dev_gz_empty = false;
    if (textMode && !w->batch.text_backed && !w->verdict_done) {
        /* a CSR batch in a run whose chunks the device parses (a chunk the sequencer parsed itself): its kernels
           are enqueued by the submission, so it waits for the verdicts in front of it first -- with nothing of
           this thread in flight, whose verdicts nobody else could publish */
        finish_all();
        w->verdict_done = true;
        p.verdicts.publish(w->seq_no, true);
        if (p.verdicts.wait_before(w->seq_no)) {
            make_empty(w);
            p.fmtq.push(w);
            return;
        }
    }
    t.depthSum += inflight.size() + 1;
    const double t0 = now_s();
    const fplh::Batch& b = w->batch;
    const bool text = b.text_backed;
    if (text)
        w->rc = fpl_process_text_async(ctx, b.raw.data() + b.raw_begin, b.raw_len);
    else if (b.bam_backed) /* (the device decodes the bases into the batch's own page-locked arrays) */
        w->rc = p.api.process_bam_async(ctx, b.bam.data(), b.bam.size(), b.rec_start.data(), b.off.data(), b.n(),
                                        p.bamKeepArrays ? w->batch.seq.data() : nullptr, p.bamKeepArrays ? w->batch.qual.data() : nullptr,
                                        w->res.data());
    else
        w->rc = fpl_process_batch_async(ctx, b.seq.data(), b.qual.data(), b.off.data(), b.n(), w->res.data());
    t.tGpu += now_s() - t0;
    t.tSubmit += now_s() - t0;
    t.nSubmit++;
    if (w->rc != FPL_OK) { /* nothing was enqueued: hand the error on in order */
        fail(w, w->rc);
        if (textMode && text) p.verdicts.publish(w->seq_no, true); /* (nobody may wait for this chunk's verdict for ever) */
        finish_all();
        p.fmtq.push(w);
        return;
    }
    inflight.push_back(Flight{w, text ? (int)TEXT_PENDING : (int)CSR});
}

void DeviceStage::run() {
    while (open || !inflight.empty() || !redo.empty()) {
        /* 1. fill the pipeline: every free slot gets a batch if one is parsed (uploads queue up behind one another) */
        bool starved = false;
        while (inflight.size() < depth) {
            Work* w = take();
            if (!w) {
                starved = true;
                break;
            }
            submit(w);
        }
        if (inflight.empty()) continue;
        /* 2. the oldest pending batch's verdict and kernels -- while another upload is queued behind it (or nothing more is
           to come): the wait inside is for ITS upload, and the link must not run dry meanwhile */
        /* (all but the newest pending batch: the batch this thread is about to wait for was then started an iteration ago,
           and the next one's kernels sit in the device's queue behind its) */
        while (n_pending() >= 2) approve_next();
        if (n_pending() == 1 && starved) approve_next();
        /* 3. the oldest batch's results, when the pipeline is full or has nothing else to do */
        if (inflight.size() >= depth || starved) finish_oldest();
    }
    p.fmtq.push(nullptr);
}

void Pipeline::device_stage(int d) { DeviceStage(*this, d).run(); }

/* ---- stage 3: the output text of a batch, on helper threads (the writer only writes) */
void Pipeline::format_stage(int f) {
    const bool toFailed = (bool)out.ffail;
    for (;;) {
        Work* w = fmtq.pop();
        if (!w) {
            /* one end marker per device thread; the formatter that sees the last one wakes the others */
            if (devEnded.load() >= nGpus) break;
            if (++devEnded == nGpus) {
                for (int i = 0; i + 1 < nFmt; i++) fmtq.push(nullptr);
                break;
            }
            continue;
        }
        const double t1 = now_s();
        if (w->rc == FPL_OK && !out.split && out.gatherOut) {
            build_gather(w->batch, w->res.data(), w->gather, w->gather_text);
        } else if (w->rc == FPL_OK && w->dev_gz && !toFailed) { /* --out is this batch's member as the device made it */
            w->outs.resize(1);
            w->outs[0].swap(w->gz_member);
        } else if (w->rc == FPL_OK && w->dev_gz_empty && !toFailed) {
            /* nothing to write, and nothing to format from: without --failed_out the batch's bases stayed on the device */
            w->outs.clear();
        } else if (w->rc == FPL_OK && !out.split) { /* (--split* output is cut per pack of 16 reads by the writer) */
            fplh::format_batch_parallel(w->batch, w->res.data(), fmtThreads, w->outs, toFailed ? &w->faileds : nullptr,
                                        opt.fragmentMode ? &w->frags : nullptr);
            /* --keep_tags: which input record every record of the pieces came from, by the formatter's own order */
            const fplh::FragmentList* fl = opt.fragmentMode ? &w->frags : nullptr;
            const bool tagOut = out.keepTags && out.fout && out.fout.bam && !w->dev_gz, tagFailed = out.keepTags && toFailed && out.ffail.bam;
            if (tagOut) w->outTags.clear(), fplh::bam_tag_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, false, w->outTags, out.keepMods, out.keepMoves);
            if (tagFailed) w->failedTags.clear(), fplh::bam_tag_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, true, w->failedTags, out.keepMods, out.keepMoves);
            /* --comment_tags: the same lists, with re-indexing on, for the outputs that are FASTQ text; in front of the deflate */
            const bool noteOut = out.comments && w->batch.bam_backed && out.fout && !out.fout.bam && !w->dev_gz;
            const bool noteFailed = out.comments && w->batch.bam_backed && toFailed && !out.ffail.bam;
            if (noteOut) w->outTags.clear(), fplh::bam_tag_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, false, w->outTags, true), out.comment_pieces(w->outs, w->outTags);
            if (noteFailed) w->failedTags.clear(), fplh::bam_tag_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, true, w->failedTags, true), out.comment_pieces(w->faileds, w->failedTags);
            /* --reindex_comments: a text input's comments follow the trims and splits, for the same outputs, in the same place */
            const bool fixOut = out.reindexComments && !w->batch.bam_backed && out.fout && !out.fout.bam && !w->dev_gz;
            const bool fixFailed = out.reindexComments && !w->batch.bam_backed && toFailed && !out.ffail.bam;
            if (fixOut) w->outNotes.clear(), fplh::fq_comment_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, false, w->outNotes), out.reindex_pieces(w->outs, w->outNotes);
            if (fixFailed) w->failedNotes.clear(), fplh::fq_comment_sources(w->batch, w->res.data(), 0, w->batch.n(), fl, true, w->failedNotes), out.reindex_pieces(w->faileds, w->failedNotes);
            if (w->dev_gz) { /* (formatted for --failed_out alone) */
                w->outs.resize(1);
                w->outs[0].swap(w->gz_member);
            } else if (out.fout && out.fout.gz) out.gzip_pieces(w->outs, out.fout, tagOut ? &w->outTags : nullptr);
            if (toFailed && out.ffail.gz) out.gzip_pieces(w->faileds, out.ffail, tagFailed ? &w->failedTags : nullptr);
        }
        tFormat[(size_t)f] += now_s() - t1;
        doneq.push(w);
    }
    doneq.push(nullptr);
}

/* ---- stage 4, the calling thread: the batches' output in input order, the per-read lists of the HTML report, and with
   --split* the plan of which read goes to which worker's file */
void Pipeline::writer_stage() {
    map<uint64_t, Work*> ready;
    uint64_t next = 0;
    int live = nFmt;
    while (live > 0) {
        Work* w = doneq.pop();
        if (!w) {
            live--;
            continue;
        }
        ready[w->seq_no] = w;
        while (!ready.empty() && ready.begin()->first == next) {
            Work* r = ready.begin()->second;
            ready.erase(ready.begin());
            if (r->rc != FPL_OK) error_exit("fpl_process_batch: " + r->err);
            const double t0 = now_s();
            if (out.fout && out.gatherOut) {
                if (!r->gather.empty()) {
                    if (!write_gather(fileno(out.fout.f), r->gather)) error_exit("write failed");
                    out.fout.wrote = true;
                }
            } else if (out.fout) out.fout.write_pieces(r->outs);
            if (out.ffail) out.ffail.write_pieces(r->faileds);
            r->holders = 1; /* this thread's own hold, until note_reads is done with the batch */
            if (out.split) split_reads(r);
            note_reads(*r);
            tWrite += now_s() - t0;
            next++;
            release(r);
        }
    }
}

void Pipeline::note_reads(const Work& w) {
    /* (the per-read loop stays on locals: this object is shared with other threads, and nothing in here may make the compiler
       load a member again for every read) */
    const uint32_t n = w.batch.n();
    const int workers = opt.workers;
    const bool fragmentMode = opt.fragmentMode;
    const uint64_t base = readBase;
    fplh::HtmlInputs& pg = page;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t wk = fplh::ReadLists::worker_of(base + i, workers);
        const fpl_read_result& r = w.res[i];
        pg.pre.add(wk, (int32_t)(w.batch.off[i + 1] - w.batch.off[i]), r.median_q_pre);
        if (!fragmentMode)
            for (int f = 0; f < r.n_frag; f++)
                if (r.code[f] == FPL_PASS_FILTER) pg.post.add(wk, (int32_t)r.frag_len[f], r.median_q_post[f]);
    }
    if (fragmentMode)
        for (const fpl_fragment& fr : w.frags.frags)
            if (fr.code == FPL_PASS_FILTER)
                pg.post.add(fplh::ReadLists::worker_of(base + fr.read, workers), (int32_t)fr.len, fr.median_q);
    readBase = base + n;
}

/* --split*: the writer only PLANS -- which reads of the batch go to which worker's writer, and after which of them the
   worker's ThreadConfig::markProcessed is due (with what count); the workers' own threads (SplitOutput::start_threads)
   put the text together and write it, every worker into its own file.  A pack of 16 reads belongs to worker
   (index / 16) % workers (src/seprocessor.cpp:343-378); one that straddles two batches is marked with the second. */
struct PackRange {
    uint32_t first, last;
    long mark; /* -1: the pack goes on in the next batch */
};
void Pipeline::split_reads(Work* wp) { /* before note_reads: readBase is the index of the batch's first read */
    const Work& w = *wp;
    const uint32_t n = w.batch.n();
    const fplh::FragmentList* fl = opt.fragmentMode ? &w.frags : nullptr;
    const int workers = opt.workers;
    const uint64_t base = readBase;
    long reads = packReads, passedReads = packPassed;
    vector<vector<PackRange>> plan((size_t)workers);
    for (uint32_t i = 0; i < n;) {
        const uint64_t g = base + i;
        const uint32_t j = (uint32_t)min<uint64_t>(n, i + (16 - g % 16));
        const int wk = (int)((g / 16) % (uint64_t)workers);
        for (uint32_t k = i; k < j; k++) { /* `passed`, src/seprocessor.cpp:264-276: any output read of the read passes */
            bool passed = false;
            if (fl) {
                for (uint32_t x = fl->first[k]; x < fl->first[k + 1]; x++) passed |= fl->frags[x].code == FPL_PASS_FILTER;
            } else {
                for (int f = 0; f < w.res[k].n_frag; f++) passed |= w.res[k].code[f] == FPL_PASS_FILTER;
            }
            passedReads += passed;
        }
        reads += j - i;
        long mark = -1;
        if ((base + j) % 16 == 0) { /* the pack is complete: ThreadConfig::markProcessed */
            mark = opt.splitByLines ? passedReads : reads;
            reads = passedReads = 0;
        }
        plan[(size_t)wk].push_back({i, j, mark});
        i = j;
    }
    packReads = reads, packPassed = passedReads;
    fplh::SplitOutput* const split = out.split;
    for (int wk = 0; wk < workers; wk++) {
        if (plan[(size_t)wk].empty()) continue;
        auto job = [this, split, wp, wk, fl, ranges = std::move(plan[(size_t)wk])]() {
            const bool notes = out.comments && wp->batch.bam_backed; /* --comment_tags: the comments go into formatted text */
            const bool fix = out.reindexComments && !wp->batch.bam_backed; /* --reindex_comments: the same */
            const bool gather = !fl && !split->gzipped() && !notes && !fix;
            vector<struct iovec> iov;
            vector<fplh::BamTagSrc> src;
            vector<fplh::FqCommentSrc> fixSrc;
            string text;
            for (const PackRange& r : ranges) {
                if (gather) { /* the worker's getWriter1()->writeString(outstr), as a gather list over the batch's arrays */
                    build_gather(wp->batch, wp->res.data(), iov, text, r.first, r.last);
                    split->write_gather(wk, iov.data(), iov.size());
                } else {
                    text.clear();
                    fplh::format_range(wp->batch, wp->res.data(), r.first, r.last, text, nullptr, fl);
                    if (notes) {
                        uint64_t st[4] = {0, 0, 0, 0};
                        src.clear();
                        fplh::bam_tag_sources(wp->batch, wp->res.data(), r.first, r.last, fl, false, src, true);
                        fplh::add_tag_comments(text, src.data(), src.size(), *out.comments, st);
                        for (int k = 0; k < 4; k++) g_bamCommentStats[k] += st[k];
                    }
                    if (fix) {
                        uint64_t st[5] = {0, 0, 0, 0, 0};
                        fixSrc.clear();
                        fplh::fq_comment_sources(wp->batch, wp->res.data(), r.first, r.last, fl, false, fixSrc);
                        fplh::reindex_comments(text, fixSrc.data(), fixSrc.size(), st);
                        for (int k = 0; k < 5; k++) g_fqCommentStats[k] += st[k];
                    }
                    split->write(wk, text);
                }
                if (r.mark >= 0) split->mark(wk, r.mark);
            }
            if (splitThreads) release(wp);
        };
        if (splitThreads) {
            wp->holders++;
            split->post(wk, std::move(job));
        } else {
            job();
        }
    }
}

/* the last, short pack; then the workers' files are closed */
void Pipeline::finish_split() {
    fplh::SplitOutput* const split = out.split;
    if (packReads > 0) {
        const int wk = (int)(((readBase - 1) / 16) % (uint64_t)opt.workers);
        const long cnt = opt.splitByLines ? packPassed : packReads;
        if (splitThreads) split->post(wk, [split, wk, cnt]() { split->mark(wk, cnt); });
        else split->mark(wk, cnt);
    }
    const double t0 = now_s();
    split->close(); /* (threaded: waits for the workers' writers) */
    tWrite += now_s() - t0;
    delete split;
    out.split = nullptr;
}

void Pipeline::run() {
    thread readerThread([this]() { reader_stage(); });
    vector<thread> devThreads, fmtStage;
    for (int d = 0; d < nGpus; d++) devThreads.emplace_back([this, d]() { device_stage(d); });
    for (int f = 0; f < nFmt; f++) fmtStage.emplace_back([this, f]() { format_stage(f); });
    if (splitThreads) out.split->start_threads();
    writer_stage();
    if (out.split) finish_split();
    readerThread.join();
    for (auto& t : devThreads) t.join();
    for (auto& t : fmtStage) t.join();
    if (inputError.empty() && verdicts.bad != ~0ull) inputError = verdicts.bad_text; /* (--device_parse: the record a device's chunk came back with) */
    if (!inputError.empty()) cerr << inputError; /* (the sequential reader printed it when it met the record) */
    if (!ioError.empty()) error_exit(ioError);
}

#endif
