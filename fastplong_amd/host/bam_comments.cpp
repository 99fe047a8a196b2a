/* bam_comments.cpp -- see bam_comments.h */
#include "bam_comments.h"

#include <string.h>

#include <algorithm>
#include <atomic>

#include "pool.h"

namespace fplh {

namespace rule = fpl::bamcomment;

namespace {
/* the Z / H scan of the shared walk, by memchr */
struct MemScan {
    uint64_t operator()(const uint8_t* v, uint64_t left) const {
        const void* z = left ? memchr(v, 0, (size_t)left) : nullptr;
        return z ? (uint64_t)((const uint8_t*)z - v) + 1 : 0;
    }
};
/* the rule's sink over a string */
struct StringSink {
    std::string& s;
    void put(const char* p, uint32_t n) { s.append(p, n); }
    void copy(const uint8_t* p, uint64_t n) { s.append((const char*)p, (size_t)n); }
    uint64_t size() const { return s.size(); }
};
}  // namespace

bool parse_comment_tags(const std::string& list, BamCommentSelection& sel) {
    if (list == "*") return rule::make_selection(nullptr, -1, sel);
    std::string tags;
    for (size_t at = 0;;) {
        const size_t comma = std::min(list.find(',', at), list.size());
        if (comma - at != 2) return false;
        tags.append(list, at, 2);
        if (comma == list.size()) break;
        at = comma + 1;
    }
    const size_t n = tags.size() / 2;
    return n >= 1 && n <= (size_t)rule::MAX_TAGS && rule::make_selection(tags.data(), (int32_t)n, sel);
}

void add_tag_comments(std::string& text, const BamTagSrc* src, size_t n_src, const BamCommentSelection& sel, uint64_t stats[4]) {
    if (sel.n == 0 || n_src == 0 || text.empty()) return;
    std::string out, tags;
    out.reserve(text.size() + text.size() / 8);
    const char* p = text.data();
    const char* const end = p + text.size();
    auto line_end = [&](const char* at) {
        const char* e = (const char*)memchr(at, '\n', (size_t)(end - at));
        return e ? e : end;
    };
    for (size_t k = 0; p < end; k++) {
        const char* name_e = line_end(p);
        out.append(p, (size_t)(name_e - p));
        if (k < n_src && src[k].rec) {
            tags.clear();
            bam_record_tags(src[k], tags, nullptr, nullptr);
            StringSink sink{out};
            const rule::Counts c = rule::comment_text((const uint8_t*)tags.data(), tags.size(), sel, MemScan(), sink);
            if (c.fields) stats[0]++;
            stats[1] += c.fields, stats[2] += c.bytes, stats[3] += c.left_out;
        }
        /* the line's end and the record's three other lines, as they are */
        const char* q = name_e; /* (at a line end, or at the text's) */
        for (int l = 0; l < 3 && q < end; l++) q = line_end(q + 1);
        if (q < end) q++;
        out.append(name_e, (size_t)(q - name_e));
        p = q;
    }
    text.swap(out);
}

void pieces_add_tag_comments(std::vector<std::string>& pieces, const std::vector<BamTagSrc>& src, const BamCommentSelection& sel, uint64_t stats[4]) {
    if (sel.n == 0) return;
    std::vector<size_t> first(pieces.size() + 1, 0); /* where piece i's records start in src */
    parallel_run((int)pieces.size(), [&](int i) { first[(size_t)i + 1] = fastq_record_count(pieces[(size_t)i]); });
    for (size_t i = 0; i < pieces.size(); i++) first[i + 1] += first[i];
    std::atomic<uint64_t> sum[4];
    for (auto& s : sum) s = 0;
    parallel_run((int)pieces.size(), [&](int i) {
        uint64_t st[4] = {0, 0, 0, 0};
        const size_t a = std::min(first[(size_t)i], src.size()), b = std::min(first[(size_t)i + 1], src.size());
        add_tag_comments(pieces[(size_t)i], src.data() + a, b - a, sel, st);
        for (int k = 0; k < 4; k++) sum[k] += st[k];
    });
    for (int k = 0; k < 4; k++) stats[k] += sum[k];
}

}  // namespace fplh
