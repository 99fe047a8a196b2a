/*
 * cli_options.h -- the command line of `fastplong_amd` as one plain struct: fastplong's flag table (reference
 * src/main.cpp:27-103) plus this host's own flags, parsed and validated with the reference's messages in the reference's
 * order (Options::validate, src/options.cpp:68-207).  Part of cli.cpp's translation unit; behind parse_options() nothing
 * looks a flag up by name.
 */
#ifndef FPLH_CLI_OPTIONS_H
#define FPLH_CLI_OPTIONS_H

/* (every system header of the translation unit: the other cli_*.h include this file) */
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/uio.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "fastplong_amd.h"
#include "bam_comments.h"
#include "fasta.h"

using namespace std;

static void error_exit(const string& msg) { /* src/util.h:270-273 */
    cerr << "ERROR: " << msg << endl;
    /* the reference's exit(-1) status without its static destructors: a thread of this process may still be inside
       fpl_comm_init (ncclCommInitAll) or a device call when an error ends the run, and tearing the library's statics down under it
       can crash or hang at exit */
    fflush(NULL);
    _exit(255);
}

/* seconds on the steady clock: every timer of the host (--verbose: busy seconds per stage) */
static double now_s() { return chrono::duration<double>(chrono::steady_clock::now().time_since_epoch()).count(); }

static bool ends_with_gz(const string& p) { return p.size() > 3 && p.compare(p.size() - 3, 3, ".gz") == 0; }
static bool ends_with_bam(const string& p) { return p.size() > 4 && p.compare(p.size() - 4, 4, ".bam") == 0; } /* unaligned BAM output */

struct Flag {
    const char* name;
    char shortc;
    bool has_value;
    const char* def;
};
/* the flag table of src/main.cpp:27-103, plus --gpus / --batch_mbases of this host */
static const Flag FLAGS[] = {
    {"in", 'i', true, ""}, {"out", 'o', true, ""}, {"failed_out", 0, true, ""}, {"compression", 'z', true, "4"},
    {"stdin", 0, false, ""}, {"stdout", 0, false, ""}, {"reads_to_process", 0, true, "0"}, {"dont_overwrite", 0, false, ""},
    {"verbose", 'V', false, ""}, {"disable_adapter_trimming", 'A', false, ""}, {"start_adapter", 's', true, "auto"},
    {"end_adapter", 'e', true, "auto"}, {"adapter_fasta", 'a', true, ""}, {"distance_threshold", 'd', true, "0.25"},
    {"trimming_extension", 0, true, "10"}, {"trim_front", 'f', true, "0"}, {"trim_tail", 't', true, "0"},
    {"trim_poly_x", 'x', false, ""}, {"poly_x_min_len", 0, true, "10"}, {"cut_front", '5', false, ""},
    {"cut_tail", '3', false, ""}, {"cut_window_size", 'W', true, "4"}, {"cut_mean_quality", 'M', true, "20"},
    {"cut_front_window_size", 0, true, "4"}, {"cut_front_mean_quality", 0, true, "20"},
    {"cut_tail_window_size", 0, true, "4"}, {"cut_tail_mean_quality", 0, true, "20"}, {"mask", 'N', false, ""},
    {"mask_window_size", 0, true, "50"}, {"mask_mean_quality", 0, true, "10"}, {"break", 'b', false, ""},
    {"break_window_size", 0, true, "100"}, {"break_mean_quality", 0, true, "10"},
    {"disable_quality_filtering", 'Q', false, ""}, {"qualified_quality_phred", 'q', true, "15"},
    {"unqualified_percent_limit", 'u', true, "40"}, {"n_base_limit", 0, true, "1000000"},
    {"n_percent_limit", 'n', true, "10"}, {"mean_qual", 'm', true, "0"}, {"disable_length_filtering", 'L', false, ""},
    {"length_required", 'l', true, "20"}, {"length_limit", 0, true, "0"}, {"low_complexity_filter", 'y', false, ""},
    {"complexity_threshold", 'Y', true, "30"}, {"json", 'j', true, "fastplong.json"}, {"html", 'h', true, "fastplong.html"},
    {"report_title", 'R', true, "fastplong report"}, {"thread", 'w', true, "3"}, {"split", 0, true, "0"},
    {"split_by_lines", 0, true, "0"}, {"split_prefix_digits", 0, true, "4"},
    {"gpus", 0, true, "1"}, {"batch_mbases", 0, true, "256"}, {"batch_reads", 0, true, "0"},
    {"reader_threads", 0, true, "0"}, {"chunk_mb", 0, true, "32"}, {"gz_stream", 0, false, ""}, {"device_parse", 0, false, ""}, {"host_parse", 0, false, ""}, {"host_gzip", 0, false, ""}, {"device_gzip", 0, false, ""}, {"device_inflate", 0, false, ""}, {"bgzf", 0, false, ""}, {"keep_tags", 0, false, ""}, {"keep_mods", 0, false, ""}, {"keep_moves", 0, false, ""}, {"comment_tags", 0, true, ""}, {"reindex_comments", 0, false, ""},
};

struct Args {
    map<string, string> val;
    map<string, bool> seen;
    bool exist(const string& k) const { return seen.count(k) > 0; }
    string str(const string& k) const { return val.at(k); }
    int i(const string& k) const { return atoi(val.at(k).c_str()); }
    long l(const string& k) const { return atol(val.at(k).c_str()); }
    double d(const string& k) const { return atof(val.at(k).c_str()); }
};

static Args parse(int argc, char** argv) {
    Args a;
    for (const Flag& f : FLAGS) a.val[f.name] = f.def;
    for (int i = 1; i < argc; i++) {
        string t = argv[i];
        const Flag* fl = nullptr;
        string inline_val;
        bool has_inline = false;
        if (t.rfind("--", 0) == 0) {
            string name = t.substr(2);
            size_t eq = name.find('=');
            if (eq != string::npos) {
                inline_val = name.substr(eq + 1);
                name = name.substr(0, eq);
                has_inline = true;
            }
            for (const Flag& f : FLAGS)
                if (name == f.name) fl = &f;
            if (!fl) error_exit("undefined option: --" + name);
        } else if (t.size() == 2 && t[0] == '-') {
            for (const Flag& f : FLAGS)
                if (f.shortc && t[1] == f.shortc) fl = &f;
            if (!fl) error_exit("undefined short option: " + t);
        } else {
            error_exit("unexpected argument: " + t);
        }
        a.seen[fl->name] = true;
        if (fl->has_value) {
            if (has_inline) a.val[fl->name] = inline_val;
            else {
                if (i + 1 >= argc) error_exit(string("option needs value: --") + fl->name);
                a.val[fl->name] = argv[++i];
            }
        }
    }
    return a;
}

/* Sequence::reverseComplement, src/sequence.cpp:29-77: A<->T, C<->G (either case), else N */
static string reverse_complement(const string& s) {
    string r(s.rbegin(), s.rend());
    for (char& c : r) {
        switch (c) {
            case 'A': case 'a': c = 'T'; break;
            case 'T': case 't': c = 'A'; break;
            case 'C': case 'c': c = 'G'; break;
            case 'G': case 'g': c = 'C'; break;
            default: c = 'N';
        }
    }
    return r;
}

/* What the command line asked for.  Filled by parse_options(); the input evaluation (cli_input.h) then settles the
   adapters an "auto" stands for and --split's file size, and nothing writes it after that. */
struct Options {
    fpl_options o;
    string in, out, failedOut, jsonFile, htmlFile, reportTitle;
    bool from_stdin = false; /* --stdin, or --in /dev/stdin: no second pass over the input (evaluation, chunks, --split N) */
    bool toStdout = false, verbose = false;
    int readsToProcess = 0;
    string startAd, endAd;
    vector<string> fasta; /* --adapter_fasta */
    bool fragmentMode = false; /* --break / --mask: any number of output reads per read */
    /* --split / --split_by_lines, src/main.cpp:225-250 */
    bool splitEnabled = false, splitByNumber = false, splitByLines = false;
    int splitDigits = 0, splitNumber = 0;
    long splitSize = 0;
    int workers = 0; /* Options::validate, src/options.cpp:120-125: the HTML report's point order and --split see it */
    int nGpus = 1;
    uint64_t batchBases = 0;
    uint32_t batchReads = 0;
    bool batchSizeGiven = false; /* --batch_mbases or --batch_reads on the command line */
    long chunkMb = 0;
    int readerThreads = 0, compression = 0;
    bool gzStream = false, deviceParse = false, hostParse = false, hostGzip = false, deviceGzip = false, deviceInflate = false;
    bool bgzf = false; /* --bgzf: every .gz this run writes is BGZF blocks plus the EOF block */
    bool keepMods = false; /* --keep_mods: with --keep_tags, a trimmed or split record's MM / ML / MN are re-indexed, not dropped (csrc/bam_mod_rules.h) */
    bool keepMoves = false; /* --keep_moves: with --keep_tags, a trimmed or split record's move table mv and its ts are re-indexed, not dropped (csrc/bam_move_rules.h) */
    bool keepTags = false; /* --keep_tags: BAM input's auxiliary fields and @RG lines go into the .bam outputs (README "BAM output") */
    /* --comment_tags LIST: BAM input's auxiliary fields go behind the name lines of every FASTQ output (README "Tags as FASTQ comments") */
    bool commentTags = false;
    fplh::BamCommentSelection commentSel = {};
    /* --reindex_comments: the SAM fields a FASTQ input carries as comments follow every trim and split into the FASTQ outputs (README
       "Comments of a FASTQ input"; csrc/fq_comment_rules.h) */
    bool reindexComments = false;
    string command; /* src/main.cpp:252-256 */
    time_t t1 = 0;
};

/* Options::validate, src/options.cpp:68-207 (the checks that concern this path) */
static void validate(const Args& cmd, Options& p, int wShared, int qShared) {
    const fpl_options& o = p.o;
    if (p.in.empty()) error_exit("read input should be specified by --in, or enable --stdin if you want to read STDIN");
    if (p.toStdout && !p.out.empty()) {
        cerr << "In STDOUT mode, ignore the output filename " << p.out << endl;
        p.out = "";
    }
    { /* --dont_overwrite, src/options.cpp:90-112 */
        const bool keep = cmd.exist("dont_overwrite");
        auto exists = [](const string& f) { return !f.empty() && access(f.c_str(), F_OK) == 0; };
        const string why = " already exists and you have set to not rewrite output files by --dont_overwrite";
        if (keep && exists(p.out)) error_exit(p.out + why);
        if (keep && exists(p.failedOut)) error_exit(p.failedOut + why);
        if (!p.failedOut.empty() && p.failedOut == p.out) error_exit("--failed_out and --out shouldn't have same file name");
        if (keep && exists(p.jsonFile)) error_exit(p.jsonFile + why);
        if (keep && exists(p.htmlFile)) error_exit(p.htmlFile + why);
    }
    if (p.toStdout && p.splitEnabled) error_exit("splitting mode cannot work with stdout mode");
    if (p.splitEnabled) { /* src/options.cpp:151-168 */
        if (p.splitDigits < 0 || p.splitDigits > 10)
            error_exit("you have enabled splitting output to multiple files, the digits number of file name prefix (--split_prefix_digits) should be 0 ~ 10.");
        if (p.splitByNumber) {
            if (p.splitNumber < 2 || p.splitNumber >= 1000)
                error_exit("you have enabled splitting output by file number, the number of files (--split) should be 2 ~ 999.");
            if (p.workers > p.splitNumber) p.workers = p.splitNumber; /* thread number cannot be more than the number of file to split */
        }
        if (p.splitByLines && p.splitSize < 1000 / 4)
            error_exit("you have enabled splitting output by file lines, the file lines (--split_by_lines) should be >= 1000.");
    }
    if (p.readsToProcess < 0) error_exit("the number of reads to process (--reads_to_process) cannot be negative");
    if (o.trim_front < 0) error_exit("trim_front1 (--trim_front1) should be >0, suggest 0 ~ 100");
    if (o.trim_tail < 0) error_exit("trim_tail1 (--trim_tail1) should be >0, suggest 0 ~ 100");
    if (o.qualified_qual - 33 < 0 || o.qualified_qual - 33 > 93)
        error_exit("qualitified phred (--qualified_quality_phred) should be 0 ~ 93, suggest 3 ~ 20");
    if (o.avg_qual_req < 0 || o.avg_qual_req > 93)
        error_exit("average quality score requirement (--mean_qual) should be 0 ~ 93, suggest 5 ~ 30");
    if (o.unqualified_percent_limit < 0 || o.unqualified_percent_limit > 100)
        error_exit("unqualified percent limit (--unqualified_percent_limit) should be 0 ~ 100, suggest 20 ~ 60");
    if (o.n_base_percent_limit < 0 || o.n_base_percent_limit > 100)
        error_exit("N base percent limit (--n_percent_limit) should be 0 ~ 100, suggest 5 ~ 20");
    if (o.n_base_limit < 0 || o.n_base_limit > 1000000) error_exit("N base number limit (--n_base_limit) should be 0 ~ 1000000");
    if (o.required_length < 0) error_exit("length requirement (--length_required) should be >0, suggest >50");
    if (o.cut_front || o.cut_tail) {
        if (wShared < 1 || wShared > 1000) error_exit("the sliding window size for cutting by quality (--cut_window_size) should be between 1~1000.");
        if (qShared < 1 || qShared > 30) error_exit("the mean quality requirement for cutting by quality (--cut_mean_quality) should be 1 ~ 30, suggest 15 ~ 20.");
        if (o.cut_front_window < 1 || o.cut_front_window > 1000) error_exit("the sliding window size for cutting by quality (--cut_front_window_size) should be between 1~1000.");
        if (o.cut_front_quality < 1 || o.cut_front_quality > 30) error_exit("the mean quality requirement for cutting by quality (--cut_front_mean_quality) should be 1 ~ 30, suggest 15 ~ 20.");
        if (o.cut_tail_window < 1 || o.cut_tail_window > 1000) error_exit("the sliding window size for cutting by quality (--cut_tail_window_size) should be between 1~1000.");
        if (o.cut_tail_quality < 1 || o.cut_tail_quality > 30) error_exit("the mean quality requirement for cutting by quality (--cut_tail_mean_quality) should be 1 ~ 30, suggest 13 ~ 20.");
    }
    if (p.startAd != "auto" && !p.startAd.empty()) {
        if (p.startAd.length() <= 3) error_exit("the sequence of <adapter_sequence> should be longer than 3");
        for (char c : p.startAd)
            if (c != 'A' && c != 'T' && c != 'C' && c != 'G')
                error_exit("the adapter <adapter_sequence> can only have bases in {A, T, C, G}, but the given sequence is: " + p.startAd);
    }
    if (o.ed_max < 0 || o.ed_max > 1.0) error_exit("the adapter <distance_threshold> should be 0.0 ~ 1.0, suggest 0.1 ~ 0.3");
    if (o.trimming_extension < 0 || o.trimming_extension > 100) error_exit("the adapter <trimming_extension> should be 0 ~ 100, suggest 5 ~ 30");
}

/* the run writes FASTQ text somewhere: --stdout, an --out (or its --split* files) or a --failed_out that is not a .bam */
static bool has_fastq_output(const Options& p) {
    return p.toStdout || (!p.out.empty() && !ends_with_bam(p.out)) || (!p.splitEnabled && !p.failedOut.empty() && !ends_with_bam(p.failedOut));
}

static Options parse_options(int argc, char** argv) {
    const Args cmd = parse(argc, argv);
    Options p;
    fpl_options& o = p.o;

    p.in = cmd.str("in"), p.out = cmd.str("out"), p.failedOut = cmd.str("failed_out");
    p.toStdout = cmd.exist("stdout");
    p.readsToProcess = cmd.i("reads_to_process");
    if (cmd.exist("stdin")) p.in = "/dev/stdin";
    p.from_stdin = p.in == "/dev/stdin";

    fpl_options_default(&o);
    o.adapter_enabled = !cmd.exist("disable_adapter_trimming");
    p.startAd = cmd.str("start_adapter"), p.endAd = cmd.str("end_adapter");
    o.ed_max = cmd.d("distance_threshold");
    o.trimming_extension = cmd.i("trimming_extension");
    if (p.startAd != "auto" && p.endAd == "auto") p.endAd = reverse_complement(p.startAd); /* src/main.cpp:138-140 */
    if (!cmd.str("adapter_fasta").empty()) {
        string err;
        if (!fplh::load_fasta_adapters(cmd.str("adapter_fasta"), p.fasta, &cerr, err)) error_exit(err);
    }
    o.trim_front = cmd.i("trim_front");
    o.trim_tail = cmd.i("trim_tail");
    o.polyx = cmd.exist("trim_poly_x");
    o.polyx_min_len = cmd.i("poly_x_min_len");
    o.cut_front = cmd.exist("cut_front");
    o.cut_tail = cmd.exist("cut_tail");
    const int wShared = cmd.i("cut_window_size"), qShared = cmd.i("cut_mean_quality");
    o.cut_front_window = cmd.exist("cut_front_window_size") ? cmd.i("cut_front_window_size") : wShared;
    o.cut_front_quality = cmd.exist("cut_front_mean_quality") ? cmd.i("cut_front_mean_quality") : qShared;
    o.cut_tail_window = cmd.exist("cut_tail_window_size") ? cmd.i("cut_tail_window_size") : wShared;
    o.cut_tail_quality = cmd.exist("cut_tail_mean_quality") ? cmd.i("cut_tail_mean_quality") : qShared;
    if (!o.cut_front && !o.cut_tail &&
        (cmd.exist("cut_window_size") || cmd.exist("cut_mean_quality") || cmd.exist("cut_front_window_size") ||
         cmd.exist("cut_front_mean_quality") || cmd.exist("cut_tail_window_size") || cmd.exist("cut_tail_mean_quality")))
        cerr << "WARNING: you specified the options for cutting by quality, but forgot to enable any of "
                "cut_front/cut_tail/cut_right. This will have no effect." << endl;
    o.qual_filter = !cmd.exist("disable_quality_filtering");
    o.qualified_qual = 33 + cmd.i("qualified_quality_phred"); /* num2qual */
    o.unqualified_percent_limit = cmd.i("unqualified_percent_limit");
    o.avg_qual_req = cmd.i("mean_qual");
    o.n_base_percent_limit = cmd.i("n_percent_limit");
    o.n_base_limit = cmd.i("n_base_limit");
    o.length_filter = !cmd.exist("disable_length_filtering");
    o.required_length = cmd.i("length_required");
    o.max_length = cmd.i("length_limit");
    o.complexity_filter = cmd.exist("low_complexity_filter");
    o.complexity_percent = min(100, max(0, cmd.i("complexity_threshold")));
    o.mask_enabled = cmd.exist("mask"); /* src/main.cpp:207-215 */
    o.mask_window = cmd.i("mask_window_size");
    o.mask_quality = cmd.i("mask_mean_quality");
    o.break_enabled = cmd.exist("break");
    o.break_window = cmd.i("break_window_size");
    o.break_quality = cmd.i("break_mean_quality");
    if ((o.mask_enabled && o.mask_window <= 0) || (o.break_enabled && o.break_window <= 0))
        error_exit("the window size of --mask / --break must be positive");
    p.fragmentMode = o.mask_enabled || o.break_enabled;
    /* src/main.cpp:225-250 */
    p.splitEnabled = cmd.exist("split") || cmd.exist("split_by_lines");
    p.splitDigits = cmd.i("split_prefix_digits");
    if (cmd.exist("split") && cmd.exist("split_by_lines"))
        error_exit("You cannot set both splitting by file number (--split) and splitting by file lines (--split_by_lines), please choose either.");
    if (cmd.exist("split")) {
        p.splitNumber = cmd.i("split");
        p.splitByNumber = true;
    }
    if (cmd.exist("split_by_lines")) {
        const long lines = cmd.l("split_by_lines");
        if (lines % 4 != 0) error_exit("Line number (--split_by_lines) should be a multiple of 4");
        p.splitSize = lines / 4; /* 4 lines per record */
        p.splitByLines = true;
    }
    if (p.from_stdin && p.splitByNumber) error_exit("Splitting by file number is not supported in STDIN mode");
    p.jsonFile = cmd.str("json"), p.htmlFile = cmd.str("html"), p.reportTitle = cmd.str("report_title");
    p.workers = cmd.i("thread");
    if (p.workers < 1) p.workers = 1;
    else if (p.workers > 16) {
        cerr << "WARNING: fastp uses up to 16 threads although you specified " << p.workers << endl;
        p.workers = 16;
    }
    p.nGpus = max(1, cmd.i("gpus"));
    p.batchBases = (uint64_t)max(1L, cmd.l("batch_mbases")) * 1000000ull;
    p.batchReads = cmd.l("batch_reads") > 0 ? (uint32_t)cmd.l("batch_reads") : 0x3FFFFFFFu;
    p.batchSizeGiven = cmd.exist("batch_mbases") || cmd.exist("batch_reads");
    p.chunkMb = cmd.l("chunk_mb");
    p.readerThreads = cmd.i("reader_threads");
    p.compression = cmd.i("compression");
    p.verbose = cmd.exist("verbose");
    p.gzStream = cmd.exist("gz_stream"), p.deviceParse = cmd.exist("device_parse"), p.hostParse = cmd.exist("host_parse");
    p.hostGzip = cmd.exist("host_gzip"), p.deviceGzip = cmd.exist("device_gzip"), p.deviceInflate = cmd.exist("device_inflate");
    p.bgzf = cmd.exist("bgzf");
    const bool bamOut = (ends_with_bam(p.out) && !p.toStdout) || (!p.splitEnabled && ends_with_bam(p.failedOut)); /* (BGZF by itself: --bgzf changes nothing for it) */
    if (p.bgzf && !bamOut && !((ends_with_gz(p.out) && !p.toStdout) || (!p.splitEnabled && ends_with_gz(p.failedOut))))
        error_exit("--bgzf needs an output whose name ends in .gz (--out, --failed_out or the --split files)");
    p.keepTags = cmd.exist("keep_tags");
    if (p.keepTags && !bamOut) error_exit("--keep_tags needs an output whose name ends in .bam (--out or --failed_out)");
    p.keepMods = cmd.exist("keep_mods");
    if (p.keepMods && !p.keepTags) error_exit("--keep_mods needs --keep_tags");
    p.keepMoves = cmd.exist("keep_moves");
    if (p.keepMoves && !p.keepTags) error_exit("--keep_moves needs --keep_tags");
    p.commentTags = cmd.exist("comment_tags");
    if (p.commentTags) {
        if (!fplh::parse_comment_tags(cmd.str("comment_tags"), p.commentSel))
            error_exit("--comment_tags takes * or a list of 1 to 32 two-character tags such as MM,ML (got: " + cmd.str("comment_tags") + ")");
        if (!has_fastq_output(p)) error_exit("--comment_tags needs a FASTQ output (--out, --failed_out, --stdout or the --split files; a .bam output follows --keep_tags)");
    }
    p.reindexComments = cmd.exist("reindex_comments");
    if (p.reindexComments) {
        if (p.commentTags) error_exit("--reindex_comments and --comment_tags exclude each other (the one is for FASTQ input, the other for BAM input)");
        if (!has_fastq_output(p)) error_exit("--reindex_comments needs a FASTQ output (--out, --failed_out, --stdout or the --split files; a .bam output cuts its names at the first tab)");
    }
    if (p.splitEnabled && ends_with_bam(p.out)) error_exit("--split / --split_by_lines do not write BAM files (--out " + p.out + ")");

    stringstream ss; /* src/main.cpp:252-256 */
    for (int i = 0; i < argc; i++) ss << argv[i] << " ";
    p.command = ss.str();
    p.t1 = time(NULL);

    validate(cmd, p, wShared, qShared);
    return p;
}

#endif
