/*
 * cli_device.h -- what the CLI needs from libfastplong_amd.so beyond the calls it links against: the optional entry points
 * of the later C-ABI versions, looked up by name, and the device contexts.  Part of cli.cpp's translation unit.
 */
#ifndef FPLH_CLI_DEVICE_H
#define FPLH_CLI_DEVICE_H

#include "bam.h"
#include "cli_options.h"
#include "gzip.h"

/* The optional entry points.  They are looked up at run time: the binary must start against a library without them (the
   test stand-ins, an older build).  Which of them a run NEEDS is the caller's business: BAM input without the two v8 calls
   is an error (evaluate_input), a missing gzip or inflater call leaves that work on the host without a word. */
struct DeviceApi {
    typedef int (*BamAsyncFn)(fpl_ctx*, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, uint32_t, uint8_t*, uint8_t*,
                              fpl_read_result*);
    typedef int (*BamDecodeFn)(int32_t, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, uint32_t, uint8_t*, uint8_t*);
    typedef void* (*InflaterCreateFn)(int32_t);
    typedef void (*InflaterDestroyFn)(void*);
    typedef int (*SetGzipFn)(fpl_ctx*, int);
    typedef int (*WaitTextGzFn)(fpl_ctx*, fpl_text_result*, const fpl_read_result**, const uint32_t**, const uint8_t**, uint64_t*);
    typedef int (*WaitBamGzFn)(fpl_ctx*, const uint8_t**, uint64_t*);
    /* BAM input, C-ABI version 8 */
    BamAsyncFn process_bam_async = nullptr;
    BamDecodeFn decode_bam = nullptr;
    /* --device_inflate (the ABI version is still 10, the three calls are found by name) */
    InflaterCreateFn inflater_create = nullptr;
    fplh::BgzfInflateFn inflate_bgzf = nullptr;
    InflaterDestroyFn inflater_destroy = nullptr;
    fplh::GzipInflateFn inflate_gzip = nullptr; /* (the same handle: a one-member .gz, host/gzip.h) */
    /* --out *.gz deflated on the device: text batches (version 9), BAM-backed batches (version 10) */
    SetGzipFn set_text_gzip = nullptr;
    WaitTextGzFn wait_text_gz = nullptr;
    SetGzipFn set_bam_gzip = nullptr;
    WaitBamGzFn wait_bam_gz = nullptr;
    /* --bgzf: the device frames its gzip batches as BGZF blocks (found by name; without it the host frames everything) */
    SetGzipFn set_gzip_framing = nullptr;
    /* --out *.bam: the device's gzip batches are BAM records in BGZF blocks (found by name; without it the host converts and frames) */
    SetGzipFn set_gzip_records = nullptr;
    /* --keep_tags: ... and those records carry the input records' auxiliary fields (found by name; without it the host writes
       every record of such a run) */
    typedef int (*BamTagStatsFn)(fpl_ctx*, uint64_t*);
    SetGzipFn set_bam_tags = nullptr;
    BamTagStatsFn get_bam_tag_stats = nullptr;
    /* --keep_mods: ... and re-index MM / ML / MN in them (found by name; without them the host writes every record of such a run) */
    SetGzipFn set_bam_mods = nullptr;
    BamTagStatsFn get_bam_mod_stats = nullptr;
    /* --keep_moves: ... and the move table and ts (found by name, and without them the host writes, in the same way) */
    SetGzipFn set_bam_moves = nullptr;
    BamTagStatsFn get_bam_move_stats = nullptr;
    /* --comment_tags: the device's FASTQ gzip form of a BAM-backed batch writes the fields behind the names (found by name; without
       it the host formats every batch of such a run) */
    typedef int (*SetBamCommentsFn)(fpl_ctx*, const char*, int);
    SetBamCommentsFn set_bam_comments = nullptr;
    BamTagStatsFn get_bam_comment_stats = nullptr;
    /* --break / --mask with --device_gzip: the device writes its gzip batches from the fragment lists (found by name; without it
       such a run stays with the host's formatter) */
    SetGzipFn set_fragment_output = nullptr;
};

static DeviceApi load_device_api() {
    DeviceApi a;
    a.process_bam_async = (DeviceApi::BamAsyncFn)dlsym(RTLD_DEFAULT, "fpl_process_bam_async");
    a.decode_bam = (DeviceApi::BamDecodeFn)dlsym(RTLD_DEFAULT, "fpl_decode_bam");
    a.inflater_create = (DeviceApi::InflaterCreateFn)dlsym(RTLD_DEFAULT, "fpl_inflater_create");
    a.inflate_bgzf = (fplh::BgzfInflateFn)dlsym(RTLD_DEFAULT, "fpl_inflate_bgzf");
    a.inflater_destroy = (DeviceApi::InflaterDestroyFn)dlsym(RTLD_DEFAULT, "fpl_inflater_destroy");
    a.inflate_gzip = (fplh::GzipInflateFn)dlsym(RTLD_DEFAULT, "fpl_inflate_gzip");
    a.set_text_gzip = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_text_gzip");
    a.wait_text_gz = (DeviceApi::WaitTextGzFn)dlsym(RTLD_DEFAULT, "fpl_wait_text_gz");
    a.set_bam_gzip = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_bam_gzip");
    a.wait_bam_gz = (DeviceApi::WaitBamGzFn)dlsym(RTLD_DEFAULT, "fpl_wait_bam_gz");
    a.set_gzip_framing = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_gzip_framing");
    a.set_gzip_records = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_gzip_records");
    a.set_bam_tags = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_bam_tags");
    a.get_bam_tag_stats = (DeviceApi::BamTagStatsFn)dlsym(RTLD_DEFAULT, "fpl_get_bam_tag_stats");
    a.set_bam_mods = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_bam_mods");
    a.get_bam_mod_stats = (DeviceApi::BamTagStatsFn)dlsym(RTLD_DEFAULT, "fpl_get_bam_mod_stats");
    a.set_bam_moves = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_bam_moves");
    a.get_bam_move_stats = (DeviceApi::BamTagStatsFn)dlsym(RTLD_DEFAULT, "fpl_get_bam_move_stats");
    a.set_bam_comments = (DeviceApi::SetBamCommentsFn)dlsym(RTLD_DEFAULT, "fpl_set_bam_comments");
    a.get_bam_comment_stats = (DeviceApi::BamTagStatsFn)dlsym(RTLD_DEFAULT, "fpl_get_bam_comment_stats");
    a.set_fragment_output = (DeviceApi::SetGzipFn)dlsym(RTLD_DEFAULT, "fpl_set_fragment_output");
    return a;
}

/* --break / --mask: may the device write this run's --out?  Only when --device_gzip asks for it, under the other conditions of
   the device's gzip form (a .gz, no --split*, -z <= 4, no --host_gzip, not BAM records, no --comment_tags, no --reindex_comments) and with a library
   that has the call.  Without the flag nothing about such a run changes. */
static bool fragment_device_out(const Options& opt, const DeviceApi& api) {
    return opt.fragmentMode && opt.deviceGzip && api.set_fragment_output && ends_with_gz(opt.out) && !opt.toStdout && !opt.splitEnabled &&
           opt.compression <= 4 && !opt.hostGzip && !opt.commentTags && !opt.reindexComments;
}

/* BGZF framing (set_gzip_framing) or BAM records (set_gzip_records: FPL_GZIP_BAM is 1 like FPL_GZIP_BGZF) on every context or
   on none */
static bool frame_on_all(DeviceApi::SetGzipFn set, const vector<fpl_ctx*>& ctxs) {
    static_assert((int)FPL_GZIP_BAM == (int)FPL_GZIP_BGZF && (int)FPL_GZIP_FASTQ == (int)FPL_GZIP_MEMBER, "one helper for both calls");
    bool on = set != nullptr;
    for (size_t d = 0; on && d < ctxs.size(); d++)
        if (set(ctxs[d], FPL_GZIP_BGZF) != FPL_OK) on = false;
    if (!on)
        for (size_t d = 0; set && d < ctxs.size(); d++) (void)set(ctxs[d], FPL_GZIP_MEMBER);
    return on;
}

/* a gzip form on every context or on none: one context that refuses switches all of them back off (`have_wait`: the wait
   call that fetches the members exists too) */
static bool enable_on_all(DeviceApi::SetGzipFn set, bool have_wait, const vector<fpl_ctx*>& ctxs) {
    bool on = set && have_wait;
    for (size_t d = 0; on && d < ctxs.size(); d++)
        if (set(ctxs[d], 1) != FPL_OK) on = false;
    if (!on)
        for (size_t d = 0; set && d < ctxs.size(); d++) (void)set(ctxs[d], 0);
    return on;
}

/* one context per device (and, in the pipeline, one host thread) */
static vector<fpl_ctx*> create_contexts(const Options& opt) {
    const int nGpus = opt.nGpus;
    vector<fpl_adapter> fa(opt.fasta.size());
    for (size_t i = 0; i < opt.fasta.size(); i++) fa[i] = fpl_adapter{opt.fasta[i].data(), (int32_t)opt.fasta[i].size()};
    vector<fpl_ctx*> ctxs((size_t)nGpus, nullptr);
    /* (a context costs a tenth of a second -- streams, events, tables, the device's first allocations: the devices' contexts
       are made side by side, a node's eight in the time of one) */
    vector<int> rcs((size_t)nGpus, FPL_OK);
    auto make = [&](int d) {
        rcs[(size_t)d] = fpl_create(&ctxs[(size_t)d], &opt.o, opt.startAd.data(), (int32_t)opt.startAd.size(), opt.endAd.data(),
                                    (int32_t)opt.endAd.size(), fa.data(), (int32_t)fa.size(), d, 65536);
    };
    vector<thread> makers;
    for (int d = 1; d < nGpus; d++) makers.emplace_back(make, d);
    make(0);
    for (auto& t : makers) t.join();
    for (int d = 0; d < nGpus; d++) {
        if (rcs[(size_t)d] == FPL_ERR_NO_DEVICE)
            error_exit("fastplong_amd needs " + to_string(nGpus) + " HIP device(s); there is no CPU path");
        if (rcs[(size_t)d] != FPL_OK) error_exit(string("fpl_create: ") + fpl_strerror(rcs[(size_t)d]));
    }
    return ctxs;
}

#endif
