/*
 * cli_finish.h -- what follows the last batch: the --verbose account of the pipeline, the merge of the devices' counters
 * and the reports.  Part of cli.cpp's translation unit.
 */
#ifndef FPLH_CLI_FINISH_H
#define FPLH_CLI_FINISH_H

#include "batch.h"
#include "cli_pipeline.h"

/* --verbose: where the wall time of the host pipeline went (busy seconds per stage), and which paths the batches took */
static void print_pipeline_summary(const Pipeline& p) {
    const InputPlan& in = p.in;
    double g = 0, f = 0;
    for (const DeviceTimes& t : p.devTimes) g = max(g, t.tGpu);
    for (double t : p.tFormat) f = max(f, t);
    cerr << "host pipeline: " << p.nBatches << " batches, wall " << now_s() - p.tStart << " s; busy: parse " << p.tParse
         << " s" << (in.chunked ? " (busiest of " + to_string(in.readerThreads) + " chunk parsers; " + to_string(p.nRedo) + " chunks parsed again, " + to_string(p.tRedo) + " s)" : string())
         << ", copies + kernels (waits) " << g << " s, format (" << p.fmtThreads << " threads) " << f << " s, write " << p.tWrite
         << " s" << endl;
    for (int d = 0; d < p.nGpus; d++) {
        const DeviceTimes& t = p.devTimes[(size_t)d];
        cerr << "device thread " << d << ": " << t.nSubmit << " submissions " << t.tSubmit << " s (mean depth behind them "
             << (t.nSubmit ? (double)t.depthSum / (double)t.nSubmit : 0.0) << "), queue empty with room for a batch " << t.nMiss
             << " times, nothing in flight and nothing parsed " << t.tStarved << " s" << endl;
    }
    if (p.facts.inflater && in.bamReader) {
        uint64_t onDev = 0, refused = 0;
        fplh::bam_prefix_block_counts(onDev, refused);
        cerr << "input: BGZF blocks inflated on the device: " << onDev + in.bamReader->blocks_on_device() << " ("
             << refused + in.bamReader->blocks_refused() << " refused, inflated by the host)" << endl;
    }
    if (p.devBamGz || (in.textMode && p.devGz))
        cerr << "device gzip: " << p.nDevGz.load() << " members deflated on the device (in the waits above)" << endl;
    if (p.out.fout && p.out.fout.bam) cerr << "BAM records: BGZF blocks framed on the device: " << p.nDevBgzf.load() << " (every other block by the host)" << endl;
    else if (p.opt.bgzf) cerr << "BGZF blocks framed on the device: " << p.nDevBgzf.load() << " (every other block by the host)" << endl;
    if (p.opt.keepTags) { /* both forms: the host's converter and, where the library has the call, every context's kernels */
        uint64_t t[4];
        for (int k = 0; k < 4; k++) t[k] = g_bamTagStats[k].load();
        for (fpl_ctx* ctx : p.ctxs) {
            uint64_t c[4] = {0, 0, 0, 0};
            if (p.api.get_bam_tag_stats && p.api.get_bam_tag_stats(ctx, c) == FPL_OK)
                for (int k = 0; k < 4; k++) t[k] += c[k];
        }
        cerr << "BAM tags: " << t[0] << " records kept every field, " << t[1] << " lost positional fields (MM, ML, MN, B arrays), " << t[2]
             << " bytes" << endl;
    }
    if (p.opt.keepMods) { /* the same two forms */
        uint64_t t[4];
        for (int k = 0; k < 4; k++) t[k] = g_bamModStats[k].load();
        for (fpl_ctx* ctx : p.ctxs) {
            uint64_t c[4] = {0, 0, 0, 0};
            if (p.api.get_bam_mod_stats && p.api.get_bam_mod_stats(ctx, c) == FPL_OK)
                for (int k = 0; k < 4; k++) t[k] += c[k];
        }
        cerr << "BAM modifications: " << t[0] << " records re-indexed, " << t[1] << " not re-indexable and dropped, " << t[2]
             << " positions kept, " << t[3] << " cut away" << endl;
    }
    if (p.opt.keepMoves) { /* the same two forms */
        uint64_t t[4];
        for (int k = 0; k < 4; k++) t[k] = g_bamMoveStats[k].load();
        for (fpl_ctx* ctx : p.ctxs) {
            uint64_t c[4] = {0, 0, 0, 0};
            if (p.api.get_bam_move_stats && p.api.get_bam_move_stats(ctx, c) == FPL_OK)
                for (int k = 0; k < 4; k++) t[k] += c[k];
        }
        cerr << "BAM move tables: " << t[0] << " records re-indexed, " << t[1] << " not re-indexable and dropped, " << t[2]
             << " entries kept, " << t[3] << " cut away" << endl;
    }
    if (p.opt.commentTags) { /* the same two forms */
        uint64_t t[4];
        for (int k = 0; k < 4; k++) t[k] = g_bamCommentStats[k].load();
        for (fpl_ctx* ctx : p.ctxs) {
            uint64_t c[4] = {0, 0, 0, 0};
            if (p.api.get_bam_comment_stats && p.api.get_bam_comment_stats(ctx, c) == FPL_OK)
                for (int k = 0; k < 4; k++) t[k] += c[k];
        }
        cerr << "FASTQ comments: " << t[0] << " records, " << t[1] << " fields, " << t[2] << " bytes, " << t[3] << " fields left out (control bytes)" << endl;
    }
    if (p.opt.reindexComments) {
        uint64_t t[5];
        for (int k = 0; k < 5; k++) t[k] = g_fqCommentStats[k].load();
        cerr << "FASTQ comments re-indexed: " << t[0] << " reads, " << t[1] << " not re-indexable and dropped, " << t[2] << " positions kept, " << t[3]
             << " cut away, " << t[4] << " reads left as they are (not tags)" << endl;
    }
    if (in.textMode)
        cerr << "device parse: " << p.nTextBatches.load() << " chunks parsed on the device, " << p.nTextFallbacks.load()
             << " handed back to the host's reader (irregular text)" << endl;
    /* which kernel forms the batches took: the library picks by batch size (csrc/pipeline.h) */
    uint64_t k[6] = {0, 0, 0, 0, 0, 0};
    for (fpl_ctx* ctx : p.ctxs) {
        uint64_t c[6] = {0, 0, 0, 0, 0, 0};
        if (fpl_get_batch_forms(ctx, c) == FPL_OK) {
            for (int i = 0; i < 4; i++) k[i] += c[i];
            k[4] = max(k[4], c[4]);
        }
    }
    if (k[0])
        cerr << "kernel forms: " << k[0] << " batches, mean " << k[1] / k[0] << " reads (largest " << k[4] << "); end trims: " << k[2]
             << " through k_trim_ends_batched (64 reads per wave, from " << FPL_FORM_TRIM_BATCHED_MIN << " reads on), " << k[0] - k[2]
             << " one wave per read; statistics: " << k[3] << " through k_stats_sorted (from " << FPL_FORM_STATS_SORTED_MIN
             << " reads on), " << k[0] - k[3] << " through the two-update k_stats" << endl;
}

/* merge: agree on the per-cycle capacity, then ONE all-reduce (sum, int64) over RCCL -- behind the C-ABI; the first
   context's copy of the sums feeds the reports */
static vector<int64_t> merge_counters(const Options& opt, vector<fpl_ctx*>& ctxs, thread& commMaker, uint32_t* maxCycles) {
    const double tJ0 = now_s();
    const bool commMade = commMaker.joinable();
    if (commMade) commMaker.join();
    /* (what the end of the run waited for the communicators: the first use of RCCL in a process takes seconds, a short run
       is over before it is) */
    if (opt.verbose && commMade) cerr << "counter merge: waited " << now_s() - tJ0 << " s for fpl_comm_init after the last batch" << endl;
    const double tM0 = now_s();
    const int rc = fpl_allreduce_counters(ctxs.data(), (int32_t)ctxs.size());
    if (opt.verbose && fpl_rccl_library()[0]) cerr << "counter merge: " << now_s() - tM0 << " s" << endl;
    if (rc != FPL_OK) error_exit(string("fpl_allreduce_counters: ") + fpl_strerror(rc) + " " + fpl_last_error(ctxs[0]));
    if (opt.verbose && fpl_rccl_library()[0])
        cerr << "counter merge: one all-reduce over " << ctxs.size() << " device(s), RCCL from " << fpl_rccl_library() << endl;
    if (commMade) (void)fpl_comm_init(nullptr, 0); /* the kept communicators go back before any context does */
    *maxCycles = fpl_max_cycles(ctxs[0]);
    vector<int64_t> counters(fpl_counters_len(ctxs[0]));
    if (fpl_get_counters(ctxs[0], counters.data(), counters.size()) != FPL_OK) error_exit("fpl_get_counters failed");
    /* (the contexts, the page-locked arena and the HIP runtime are not torn down piece by piece: the process is about
       to end -- see the _exit at the bottom of main -- and unpinning a gigabyte of staging costs tenths of a second) */
    return counters;
}

/* the summary on stderr, the JSON and HTML reports, and the closing lines */
static void write_reports(const Options& opt, const InputFacts& facts, const vector<int64_t>& counters, uint32_t maxCycles,
                          const fplh::HtmlInputs& page, double tStart) {
    fplh::ReportInputs ri;
    ri.counters = counters.data();
    ri.C = maxCycles;
    ri.adapters.push_back(opt.startAd);
    ri.adapters.push_back(opt.endAd);
    for (auto& s : opt.fasta) ri.adapters.push_back(s);
    ri.adapter_enabled = opt.o.adapter_enabled;
    ri.polyx = opt.o.polyx;
    ri.complexity = opt.o.complexity_filter;
    ri.length_filter = opt.o.length_filter;
    ri.max_length = opt.o.max_length;
    ri.is_rna = facts.isRNA;
    ri.command = opt.command;
    cerr << fplh::summary_text(ri);
    const double tRep0 = now_s();
    /* nothing reads a batch any more: the page-locked arena is unpinned (0.09 s for 1.4 GB) while the reports are written,
       instead of by the kernel when the process exits */
    thread arenaRelease([]() { fplh::ByteBuf::release_arena(); });
    { /* the two report writers only read the counters: side by side */
        bool jsonOk = true;
        double tJson = 0;
        thread jt([&]() {
            jsonOk = fplh::write_json(opt.jsonFile, ri);
            tJson = now_s() - tRep0;
        });
        const bool htmlOk = fplh::write_html(opt.htmlFile, ri, page);
        const double tHtml = now_s() - tRep0;
        jt.join();
        if (!jsonOk) error_exit("Failed to write: " + opt.jsonFile);
        if (!htmlOk) error_exit("Failed to write: " + opt.htmlFile);
        if (opt.verbose)
            cerr << "reports: json " << tJson << " s beside html " << tHtml << " s; since start " << now_s() - tStart << " s" << endl;
    }
    arenaRelease.join();
    const time_t t2 = time(NULL);
    cerr << endl << "JSON report: " << opt.jsonFile << endl;
    cerr << "HTML report: " << opt.htmlFile << endl;
    cerr << endl << opt.command << endl;
    cerr << "fastplong v0.4.1 (fastplong_amd), time used: " << (t2) - opt.t1 << " seconds" << endl;
}

#endif
