/* fq_comments.cpp -- see fq_comments.h */
#include "fq_comments.h"

#include <string.h>

#include <algorithm>
#include <atomic>

#include "../csrc/fq_comment_rules.h"
#include "bam_out.h"
#include "pool.h"

namespace fplh {

namespace rule = fpl::fqcomment;

namespace {
/* the rule's sink over a string */
struct StringSink {
    std::string& s;
    void put(const char* p, uint32_t n) { s.append(p, n); }
    void copy(const uint8_t* p, uint64_t n) { s.append((const char*)p, (size_t)n); }
};
}  // namespace

void fq_comment_sources(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, const FragmentList* fl, bool failed,
                        std::vector<FqCommentSrc>& src) {
    for (uint32_t i = first; i < last && i < b.n(); i++) {
        const fpl_read_result& r = res[i];
        if (r.dropped) continue;
        const uint32_t l_seq = (uint32_t)(b.off[i + 1] - b.off[i]);
        const FqCommentSrc whole = {b.name_ptr(i), b.name_len[i], b.seq_ptr(i), l_seq, 0, 0, true, failed, fl != nullptr};
        auto add = [&](uint32_t start, uint32_t len, bool changed) {
            FqCommentSrc s = whole;
            s.start = std::min(start, l_seq), s.len = std::min(len, l_seq - s.start), s.changed = changed;
            src.push_back(s);
        };
        if (fl) { /* --break / --mask: every record is changed */
            const uint32_t f0 = fl->first[i], f1 = fl->first[i + 1];
            for (uint32_t k = f0; k < f1; k++) {
                const fpl_fragment& f = fl->frags[k];
                const bool pass = f.code == FPL_PASS_FILTER;
                if (!failed && pass) add(f.start, f.len, true);
                else if (failed && !pass && f1 - f0 == 1) add(r.r1_start, r.r1_len, true);
            }
            continue;
        }
        for (int k = 0; k < r.n_frag; k++) {
            const bool pass = r.code[k] == FPL_PASS_FILTER;
            if (!failed && pass) add(r.frag_start[k], r.frag_len[k], !rule::unchanged(r.n_frag, r.kind[k], r.frag_start[k], r.frag_len[k], l_seq, false));
            else if (failed && !pass && r.n_frag == 1) /* the trimmed read */
                add(r.r1_start, r.r1_len, !rule::unchanged(1, 0, r.r1_start, r.r1_len, l_seq, false));
        }
    }
}

void reindex_comments(std::string& text, const FqCommentSrc* src, size_t n_src, uint64_t stats[5]) {
    if (n_src == 0 || text.empty()) return;
    std::string out;
    out.reserve(text.size());
    const char* p = text.data();
    const char* const end = p + text.size();
    auto line_end = [&](const char* at) {
        const char* e = (const char*)memchr(at, '\n', (size_t)(end - at));
        return e ? e : end;
    };
    rule::Counts c = {0, 0, 0, 0, 0};
    for (size_t k = 0; p < end; k++) {
        const char* name_e = line_end(p);
        if (k < n_src) {
            const FqCommentSrc& s = src[k];
            StringSink sink{out};
            rule::line_text((const uint8_t*)p, (uint64_t)(name_e - p), (const uint8_t*)s.name, s.name_len, s.seq, s.l_seq, s.start, s.len, s.changed,
                            s.failed, s.fragment_mode, sink, c);
        } else
            out.append(p, (size_t)(name_e - p));
        /* the line's end and the record's three other lines, as they are */
        const char* q = name_e; /* (at a line end, or at the text's) */
        for (int l = 0; l < 3 && q < end; l++) q = line_end(q + 1);
        if (q < end) q++;
        out.append(name_e, (size_t)(q - name_e));
        p = q;
    }
    stats[0] += c.reindexed, stats[1] += c.lost, stats[2] += c.kept, stats[3] += c.cut, stats[4] += c.left;
    text.swap(out);
}

void pieces_reindex_comments(std::vector<std::string>& pieces, const std::vector<FqCommentSrc>& src, uint64_t stats[5]) {
    std::vector<size_t> first(pieces.size() + 1, 0); /* where piece i's records start in src */
    parallel_run((int)pieces.size(), [&](int i) { first[(size_t)i + 1] = fastq_record_count(pieces[(size_t)i]); });
    for (size_t i = 0; i < pieces.size(); i++) first[i + 1] += first[i];
    std::atomic<uint64_t> sum[5];
    for (auto& s : sum) s = 0;
    parallel_run((int)pieces.size(), [&](int i) {
        uint64_t st[5] = {0, 0, 0, 0, 0};
        const size_t a = std::min(first[(size_t)i], src.size()), b = std::min(first[(size_t)i + 1], src.size());
        reindex_comments(pieces[(size_t)i], src.data() + a, b - a, st);
        for (int k = 0; k < 5; k++) sum[k] += st[k];
    });
    for (int k = 0; k < 5; k++) stats[k] += sum[k];
}

}  // namespace fplh
