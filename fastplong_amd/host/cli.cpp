/*
 * cli.cpp -- `fastplong_amd`: fastplong's command line (flag names, short forms, defaults and
 * validation messages of reference src/main.cpp:27-103 and src/options.cpp:68-207) in front of
 * the MI355X hot path.  The host keeps what the reference's host keeps -- FASTQ reader/writer,
 * batching, report writers -- and calls fpl_process_batch() where the reference's workers call
 * SingleEndProcessor::processSingleEnd() (src/seprocessor.cpp:440).
 *
 * Batches are cut in input order and dealt round-robin to --gpus devices (one fpl_ctx and one
 * host thread per device); outputs are written back in input order; at the end the per-device
 * counter buffers are summed with one RCCL all-reduce (the replacement of Stats::merge /
 * FilterResult::merge, src/seprocessor.cpp:108-121) and rank 0's copy feeds the reports.
 *
 * --split / --split_by_lines replay what the reference's workers do with their private writers
 * (src/threadconfig.cpp:72-120) in the one writer thread: see SplitOutput.
 *
 * This file is main() alone; the units it runs through, one header each (all part of this translation unit):
 *   cli_options.h   the flag table, Options, parse_options: the command line, validated
 *   cli_device.h    DeviceApi (the optional C-ABI entry points, looked up by name), the device contexts
 *   cli_input.h     evaluate_input (RNA, adapters, --split's size), InputPlan / plan_input (chunks, readers, Work pool size)
 *   cli_output.h    OutFile, Outputs: --out, --failed_out, --split*
 *   cli_pipeline.h  Work, Channel, Verdicts, Pipeline and its four stages, DeviceStage
 *   cli_finish.h    the --verbose account, the counter merge, the reports
 */
#include "cli_finish.h"

/* measurement hook: FPLH_T0 = the launcher's time.time() */
static double since_launch() {
    const char* e = getenv("FPLH_T0");
    return e ? chrono::duration<double>(chrono::system_clock::now().time_since_epoch()).count() - atof(e) : -1.0;
}

int main(int argc, char* argv[]) {
    /* (before any other thread exists: a context drives five streams, the runtime's default is four hardware queues per device and
       two streams on one queue run in submission order -- fpl_create asks for the same, but setenv belongs where one thread runs) */
    setenv("GPU_MAX_HW_QUEUES", "8", 0);
    if (argc == 1) {
        cerr << "fastplong_amd: fastplong's per-read hot path on MI355X" << endl << "version 0.4.1-compatible" << endl;
        return 0;
    }
    if (argc == 2 && (strcmp(argv[1], "-v") == 0 || strcmp(argv[1], "--version") == 0)) {
        cout << "fastplong 0.4.1" << endl;
        return 0;
    }
    Options opt = parse_options(argc, argv);
    const double tMain = now_s();
    const double launchToMain = since_launch();
    const DeviceApi api = load_device_api();
    const InputFacts facts = evaluate_input(opt, api);

    const double tEval = now_s();
    vector<fpl_ctx*> ctxs = create_contexts(opt);
    /* the communicators of the closing merge, made while the batches run (a thread of its own: ncclCommInitAll over several devices
       takes longer than many a run's whole pipeline; a failure here is not one yet -- the merge then makes its own and reports) */
    thread commMaker;
    /* FPL_NO_COMM_PREINIT=1: no thread here, the merge makes the communicators itself (the round-3 order) */
    if ((opt.nGpus > 1 || getenv("FPL_RCCL_FORCE")) && !getenv("FPL_NO_COMM_PREINIT"))
        commMaker = thread([ctxs]() mutable { (void)fpl_comm_init(ctxs.data(), (int32_t)ctxs.size()); });
    const double tCreate = now_s();
    if (opt.verbose)
        cerr << "start-up: input evaluation " << tEval - tMain << " s, device contexts " << tCreate - tEval << " s" << endl;
    /* the CSR arrays of every batch are page-locked (fpl_host_alloc), so the DMA engines read them in place */
    if (!getenv("FPLH_NO_PIN")) /* (measurement hook: pageable batches, the runtime stages the copies) */
        fplh::ByteBuf::set_allocator(fpl_host_alloc, fpl_host_free);

    InputPlan plan = plan_input(opt, facts, api);
    Outputs outs = open_outputs(opt, facts.bamReadGroups);
    Pipeline pipeline(opt, api, facts, plan, outs, ctxs);
    pipeline.run();
    if (opt.verbose) print_pipeline_summary(pipeline);
    outs.close();

    uint32_t maxCycles = 0;
    const vector<int64_t> counters = merge_counters(opt, ctxs, commMaker, &maxCycles);
    write_reports(opt, facts, counters, maxCycles, pipeline.page, pipeline.tStart);
    if (opt.verbose && launchToMain >= 0)
        cerr << "since launch: main() entered at " << launchToMain << " s, returning at " << since_launch() << " s" << endl;
    if (getenv("FPLH_TEARDOWN_TIMING")) { /* measurement hook: what the explicit teardown would cost */
        const double a = now_s();
        for (fpl_ctx* ctx : ctxs) fpl_destroy(ctx);
        if (facts.inflater) api.inflater_destroy(facts.inflater);
        cerr << "teardown: contexts " << now_s() - a << " s" << endl;
    }
    /* every output has been written, flushed and closed above; skip the static destructors (worker pool, HIP runtime) */
    fflush(NULL);
    if (getenv("FPLH_NORMAL_EXIT")) exit(0); /* (measurement hook: a profiler's atexit handlers must run -- rocprofv3 writes its tables there) */
    _exit(0);
}
