/* bam_tags.cpp -- see bam_tags.h */
#include "bam_tags.h"

#include <algorithm>
#include <atomic>

#include "../csrc/bam_tag_rules.h"
#include "pool.h"

namespace fplh {

namespace tagrule = fpl::bamtag;

void bam_tag_sources(const Batch& b, const fpl_read_result* res, uint32_t first, uint32_t last, const FragmentList* fl, bool failed,
                     std::vector<BamTagSrc>& src, bool mods, bool moves) {
    const bool have = b.bam_backed && b.rec_start.size() >= b.n();
    for (uint32_t i = first; i < last && i < b.n(); i++) {
        const fpl_read_result& r = res[i];
        if (r.dropped) continue;
        const uint8_t* rec = have ? b.bam.data() + b.rec_start[i] : nullptr;
        const fpl::bamrule::Fields f = rec ? fpl::bamrule::fields(rec) : fpl::bamrule::Fields{0, 0, 0, 0, 0};
        if (fl) { /* --break / --mask: every record is changed */
            const uint32_t f0 = fl->first[i], f1 = fl->first[i + 1];
            for (uint32_t k = f0; k < f1; k++) {
                const bool pass = fl->frags[k].code == FPL_PASS_FILTER;
                if (failed ? (!pass && f1 - f0 == 1) : pass) src.push_back(BamTagSrc(rec, true, 0, 0, mods, true, moves));
            }
            continue;
        }
        for (int k = 0; k < r.n_frag; k++) {
            const bool pass = r.code[k] == FPL_PASS_FILTER;
            if (!failed && pass)
                src.push_back(BamTagSrc(rec, !tagrule::unchanged(r.n_frag, r.kind[k], r.frag_start[k], r.frag_len[k], f.l_seq, f.flag, false),
                                        r.frag_start[k], r.frag_len[k], mods, false, moves));
            else if (failed && !pass && r.n_frag == 1) /* the trimmed read */
                src.push_back(BamTagSrc(rec, !tagrule::unchanged(1, 0, r.r1_start, r.r1_len, f.l_seq, f.flag, false), r.r1_start, r.r1_len, mods, false,
                                        moves));
        }
    }
}

void pieces_to_bam_records(std::vector<std::string>& pieces, const std::vector<BamTagSrc>& src, uint64_t stats[4], uint64_t* mod_stats,
                           uint64_t* move_stats) {
    std::vector<size_t> first(pieces.size() + 1, 0); /* where piece i's records start in src */
    parallel_run((int)pieces.size(), [&](int i) { first[(size_t)i + 1] = fastq_record_count(pieces[(size_t)i]); });
    for (size_t i = 0; i < pieces.size(); i++) first[i + 1] += first[i];
    std::atomic<uint64_t> sum[12];
    for (auto& s : sum) s = 0;
    parallel_run((int)pieces.size(), [&](int i) {
        std::string& piece = pieces[(size_t)i];
        if (piece.empty()) return;
        std::string rec;
        uint64_t st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        const size_t a = std::min(first[(size_t)i], src.size()), b = std::min(first[(size_t)i + 1], src.size());
        fastq_to_bam_records(piece, src.data() + a, b - a, rec, st, st + 4, st + 8);
        for (int k = 0; k < 12; k++) sum[k] += st[k];
        piece.swap(rec);
    });
    for (int k = 0; k < 4; k++) stats[k] += sum[k];
    if (mod_stats)
        for (int k = 0; k < 4; k++) mod_stats[k] += sum[4 + k];
    if (move_stats)
        for (int k = 0; k < 4; k++) move_stats[k] += sum[8 + k];
}

}  // namespace fplh
