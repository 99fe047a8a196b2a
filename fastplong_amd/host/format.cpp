#include "fastq.h"

#include <string.h>

#include <algorithm>

#include "pool.h"

using namespace std;

namespace fplh {

/* FAILED_TYPES, src/common.h:55-64 */
static const char* failed_type(int code) {
    switch (code) {
        case 0: return "passed";
        case 4: return "failed_polyx_filter";
        case 8: return "failed_bad_overlap";
        case 12: return "failed_too_many_n_bases";
        case 16: return "failed_too_short";
        case 17: return "failed_too_long";
        case 20: return "failed_quality_filter";
        case 24: return "failed_low_complexity";
        default: return "";
    }
}

void format_batch(const Batch& b, const fpl_read_result* res, string& out, string* failed) {
    format_range(b, res, 0, b.n(), out, failed);
}

void FragmentList::index(uint32_t n_reads) {
    first.assign((size_t)n_reads + 1, 0);
    for (const fpl_fragment& f : frags)
        if (f.read < n_reads) first[f.read + 1]++;
    for (uint32_t i = 0; i < n_reads; i++) first[i + 1] += first[i];
}

void format_batch_parallel(const Batch& b, const fpl_read_result* res, int threads, vector<string>& outs,
                           vector<string>* faileds, const FragmentList* fl) {
    const uint32_t n = b.n();
    if (threads < 1) threads = 1;
    /* the pieces keep their capacity from batch to batch (the Work objects are recycled): fresh multi-megabyte strings
       would be mapped, faulted in page by page and unmapped again for every batch */
    outs.resize(threads);
    for (auto& o : outs) o.clear();
    if (faileds) {
        faileds->resize(threads);
        for (auto& o : *faileds) o.clear();
    }
    /* slices of about equal numbers of bases */
    vector<uint32_t> cut(threads + 1, n);
    cut[0] = 0;
    const uint64_t total = n ? b.off[n] : 0;
    for (int t = 1; t < threads; t++) {
        const uint64_t want = total / threads * t;
        cut[t] = (uint32_t)(std::lower_bound(b.off.begin(), b.off.begin() + n, want) - b.off.begin());
    }
    parallel_run(threads, [&](int t) {
        const size_t want = (size_t)((b.off[cut[t + 1]] - b.off[cut[t]]) * 2 + (uint64_t)(cut[t + 1] - cut[t]) * 128 + 64);
        if (outs[t].capacity() < want) outs[t].reserve(want + want / 4);
        format_range(b, res, cut[t], cut[t + 1], outs[t], faileds ? &(*faileds)[t] : nullptr, fl);
    });
}

/* bases [start, start + len) of a read with the regions Read::maskRegionWithN overwrote (src/read.cpp:217-225) */
static void append_masked(string& out, const uint8_t* s, uint32_t start, uint32_t len, const fpl_region* regs, uint32_t n_regs) {
    const size_t at = out.size();
    out.append((const char*)s + start, len);
    for (uint32_t k = 0; k < n_regs; k++) {
        if (regs[k].start < start || regs[k].start - start >= len) continue;
        const uint32_t a = regs[k].start - start, l = std::min(regs[k].len, len - a);
        memset(&out[at + a], 'N', l);
    }
}

/* or1->appendToStringWithTag, src/read.cpp:145-173: bases and qualities [start, start + len) of the read under its name and the
   tag of `code`, the n_regs regions shown as N */
static void append_tagged(string& out, const char* name, uint32_t nl, const char* strand, uint32_t sl, const uint8_t* s, const uint8_t* q,
                          uint32_t start, uint32_t len, int code, const fpl_region* regs, uint32_t n_regs) {
    out.append(name, nl);
    out.push_back(' ');
    out.append(failed_type(code));
    out.push_back('\n');
    append_masked(out, s, start, len, regs, n_regs);
    out.push_back('\n');
    out.append(strand, sl);
    out.push_back('\n');
    out.append((const char*)q + start, len);
    out.push_back('\n');
}

void format_range(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, string& out,
                  string* failed, const FragmentList* fl) {
    static const char* prefix[3] = {"", "split-by-adapter-left-", "split-by-adapter-right-"}; /* src/read.cpp:199,208 */
    for (uint32_t i = first; i < last; i++) {
        const fpl_read_result& r = res[i];
        if (r.dropped) continue;
        const char* name = b.name_ptr(i);
        const uint32_t nl = b.name_len[i], sl = b.strand_len[i];
        const char* strand = b.strand_ptr(i);
        const uint8_t* s = b.seq_ptr(i);
        const uint8_t* q = b.qual_ptr(i);
        if (fl) { /* --break / --mask: any number of output reads, src/seprocessor.cpp:234-281 */
            const uint32_t f0 = fl->first[i], f1 = fl->first[i + 1];
            for (uint32_t k = f0; k < f1; k++) {
                const fpl_fragment& f = fl->frags[k];
                const fpl_region* rg = fl->regs.data() + f.region_first;
                if (f.code == FPL_PASS_FILTER) {
                    /* the name went through breakByGap's insert(1, "split-..") and then breakByRegions'
                       insert(1, "r<i>-") (src/read.cpp:199,208,244,256) */
                    if (nl > 0) out.append(name, 1);
                    if (f.break_no) {
                        out.push_back('r');
                        out.append(std::to_string(f.break_no));
                        out.push_back('-');
                    }
                    out.append(prefix[f.kind <= 2 ? f.kind : 0]);
                    if (nl > 1) out.append(name + 1, nl - 1);
                    out.push_back('\n');
                    append_masked(out, s, f.start, f.len, rg, f.region_count);
                    out.push_back('\n');
                    out.append(strand, sl);
                    out.push_back('\n');
                    out.append((const char*)q + f.start, f.len);
                    out.push_back('\n');
                } else if (failed && f1 - f0 == 1) {
                    /* or1 with its tag; it shows the N only when the one output read IS r1 (masked in place) */
                    const bool in_place = f.kind == 0 && f.break_no == 0;
                    append_tagged(*failed, name, nl, strand, sl, s, q, r.r1_start, r.r1_len, f.code, rg, in_place ? f.region_count : 0);
                }
            }
            continue;
        }
        for (int f = 0; f < r.n_frag; f++) {
            if (r.code[f] == FPL_PASS_FILTER) { /* Read::appendToString, src/read.cpp:119-143 */
                const char* pf = prefix[r.kind[f] <= 2 ? r.kind[f] : 0];
                if (*pf && nl > 0) { /* name->insert(1, prefix) */
                    out.append(name, 1);
                    out.append(pf);
                    out.append(name + 1, nl - 1);
                } else {
                    out.append(name, nl);
                }
                out.push_back('\n');
                out.append((const char*)s + r.frag_start[f], r.frag_len[f]);
                out.push_back('\n');
                out.append(strand, sl);
                out.push_back('\n');
                out.append((const char*)q + r.frag_start[f], r.frag_len[f]);
                out.push_back('\n');
            } else if (failed && r.n_frag == 1) { /* the trimmed r1 */
                append_tagged(*failed, name, nl, strand, sl, s, q, r.r1_start, r.r1_len, r.code[f], nullptr, 0);
            }
        }
    }
}

}  // namespace fplh
