/* bam_out.cpp -- see bam_out.h */
#include "bam_out.h"

#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../csrc/bam_mod_rules.h"
#include "../csrc/bam_move_rules.h"
#include "../csrc/bam_out_rules.h"
#include "../csrc/bam_tag_rules.h"

namespace fplh {

namespace rule = fpl::bamout;
namespace tagrule = fpl::bamtag;
namespace modrule = fpl::bammod;
namespace moverule = fpl::bammove;

namespace {
/* magic, l_text, the text, n_ref = 0 */
std::string header_of(const std::string& text) {
    std::string s("BAM\1", 4);
    const uint32_t l_text = (uint32_t)text.size();
    for (int k = 0; k < 4; k++) s += (char)(l_text >> (8 * k));
    s += text;
    s.append(4, '\0'); /* n_ref */
    return s;
}
/* the Z / H scan of the shared walk, by memchr */
struct MemScan {
    uint64_t operator()(const uint8_t* v, uint64_t left) const {
        const void* z = left ? memchr(v, 0, (size_t)left) : nullptr;
        return z ? (uint64_t)((const uint8_t*)z - v) + 1 : 0;
    }
};
void put32(std::string& out, uint32_t v) {
    for (int b = 0; b < 4; b++) out += (char)(v >> (8 * b));
}
/* --keep_moves: the table of a move-re-indexable record (csrc/bam_move_rules.h) and what this output record gets of it */
struct MovePlan {
    moverule::Found fd;
    moverule::Table T;
    moverule::Cut c;
};
/* the record of s against that rule; move_stats[2], [3]: entries kept, cut away */
bool plan_moves(const BamTagSrc& s, const uint8_t* p, const moverule::Found& fd, MovePlan& M, uint64_t* move_stats) {
    const fpl::bamrule::Fields f = fpl::bamrule::fields(s.rec);
    M.fd = fd;
    if (!moverule::fields_ok(fd, p, f.flag, s.fragment_mode, M.T)) return false;
    const uint8_t* mv = p + fd.mv_at + 9;
    uint64_t ones;
    if (!moverule::count_moves(mv, M.T.m, ones) || ones != f.l_seq) return false;
    uint64_t a, b;
    moverule::clamp_range(s.start, s.len, f.l_seq, a, b);
    moverule::ends(a, b, moverule::position(mv, M.T.m, a + 1), moverule::position(mv, M.T.m, b + 1), M.c);
    if (!moverule::finish(M.T, M.c)) return false;
    if (move_stats) move_stats[2] += M.c.b - M.c.a, move_stats[3] += M.T.m - (M.c.b - M.c.a);
    return true;
}
/* the fields of a changed record, appended to out: the non-positional fields verbatim; with R (--keep_mods, the re-indexable
   record of csrc/bam_mod_rules.h) the three modification fields rewritten for s's range; with M (--keep_moves) mv and ts rewritten;
   all in the fields' order.  lost: another positional field was dropped; mod_stats[2], [3]: positions kept, cut away */
void append_reindexed(const BamTagSrc& s, const uint8_t* p, uint64_t prefix, const modrule::Record* R, const MovePlan* M, std::string& out,
                      bool& lost, uint64_t* mod_stats) {
    const fpl::bamrule::Fields f = fpl::bamrule::fields(s.rec);
    const uint64_t a = std::min<uint64_t>(s.start, f.l_seq), b = std::min<uint64_t>((uint64_t)s.start + s.len, f.l_seq);
    const uint8_t* v = nullptr;
    modrule::Cut cuts[modrule::MAX_GROUPS];
    uint64_t n_ml = 0;
    if (R) {
        const uint8_t* pk = s.rec + fpl::bamrule::qual_offset(f) - ((uint64_t)f.l_seq + 1) / 2;
        v = p + R->fd.mm_at + 3;
        const uint32_t v_len = (uint32_t)(R->fd.mm_len - 4);
        uint64_t c0[5], c1[5];
        bool have[5] = {false, false, false, false, false};
        for (uint32_t k = 0; k < R->n_groups; k++) {
            const modrule::Group& g = R->g[k];
            const uint32_t slot = modrule::code_slot(g.code);
            if (!have[slot]) c0[slot] = modrule::count_bases(pk, a, g.code), c1[slot] = modrule::count_bases(pk, b, g.code), have[slot] = true;
            cuts[k] = modrule::cut(v, v_len, g, c0[slot], c1[slot]);
            n_ml += (uint64_t)(cuts[k].j1 - cuts[k].j0) * g.k;
            if (mod_stats) mod_stats[2] += cuts[k].j1 - cuts[k].j0, mod_stats[3] += g.n_delta - (cuts[k].j1 - cuts[k].j0);
        }
    }
    lost = false;
    for (uint64_t o = 0; o < prefix;) {
        const uint64_t n = tagrule::field_len(p + o, prefix - o, MemScan());
        const char* fp = (const char*)p + o;
        if (R && o == R->fd.mm_at) {
            out.append(fp, 3);
            for (uint32_t k = 0; k < R->n_groups; k++) {
                out.append((const char*)v + R->g[k].at, R->g[k].hdr_len);
                if (cuts[k].j1 > cuts[k].j0) {
                    out += ',';
                    out += std::to_string(cuts[k].first);
                    out.append((const char*)v + cuts[k].rest_at, cuts[k].rest_end - cuts[k].rest_at);
                }
                out += ';';
            }
            out += '\0';
        } else if (R && o == R->fd.ml_at) {
            out.append(fp, 4);
            put32(out, (uint32_t)n_ml);
            for (uint32_t k = 0; k < R->n_groups; k++)
                out.append(fp + 8 + R->g[k].ml_at + (uint64_t)cuts[k].j0 * R->g[k].k, (size_t)(cuts[k].j1 - cuts[k].j0) * R->g[k].k);
        } else if (R && R->fd.n_mn && o == R->fd.mn_at) {
            out.append(fp, 3);
            const uint64_t len = b - a;
            for (uint64_t k = 0; k + 3 < n; k++) out += (char)(len >> (8 * k));
        } else if (M && o == M->fd.mv_at) {
            out.append(fp, 4);
            put32(out, (uint32_t)(1 + M->c.b - M->c.a));
            out += fp[8];
            out.append(fp + 8 + M->c.a, (size_t)(M->c.b - M->c.a));
        } else if (M && M->T.has_ts && o == M->fd.ts_at) {
            out.append(fp, 2);
            out += (char)M->c.ts_type;
            for (uint32_t k = 0; k < tagrule::scalar_size(M->c.ts_type); k++) out += (char)(M->c.ts >> (8 * k));
        } else if (!tagrule::positional(p + o))
            out.append(fp, (size_t)n);
        else
            lost = true;
        o += n;
    }
}
}  // namespace

uint64_t bam_record_tags(const BamTagSrc& s, std::string& out, uint64_t* stats, uint64_t* mod_stats, uint64_t* move_stats) {
    const uint8_t* rec = s.rec;
    const bool changed = s.changed;
    uint64_t at, len;
    tagrule::region(rec, at, len);
    const uint8_t* p = rec + at;
    const tagrule::Walk w = tagrule::walk(p, len, MemScan());
    uint64_t wrote = w.prefix;
    bool lost = changed && w.positional;
    bool done = false;
    /* either switch decides its own fields */
    modrule::Record R;
    MovePlan M;
    bool mods = false, moves = false;
    if (s.mods && changed) {
        const modrule::Found fd = modrule::find(p, w.prefix, MemScan());
        if (modrule::any_found(fd)) {
            mods = modrule::reindexable(rec, p, fd, s.fragment_mode, R);
            if (mod_stats) mod_stats[mods ? 0 : 1]++;
        }
    }
    if (s.moves && changed) {
        const moverule::Found fd = moverule::find(p, w.prefix, MemScan());
        if (moverule::any_found(fd)) {
            moves = plan_moves(s, p, fd, M, move_stats);
            if (move_stats) move_stats[moves ? 0 : 1]++;
        }
    }
    if (mods || moves) {
        const size_t before = out.size();
        append_reindexed(s, p, w.prefix, mods ? &R : nullptr, moves ? &M : nullptr, out, lost, mod_stats);
        wrote = out.size() - before;
        done = true;
    }
    if (done) {
    } else if (!changed || !w.positional) {
        out.append((const char*)p, (size_t)w.prefix);
    } else { /* the non-positional fields, in their order */
        wrote = w.kept;
        for (uint64_t o = 0; o < w.prefix;) {
            const uint64_t n = tagrule::field_len(p + o, w.prefix - o, MemScan());
            if (!tagrule::positional(p + o)) out.append((const char*)p + o, (size_t)n);
            o += n;
        }
    }
    if (stats) {
        stats[lost ? 1 : 0]++;
        stats[2] += wrote;
        if (!w.whole) stats[3]++;
    }
    return wrote;
}

const std::string& bam_header_bytes() {
    static const std::string h = header_of(FPL_BAMOUT_HEADER_TEXT);
    return h;
}
std::string bam_header_bytes(const std::string& read_groups) {
    return header_of(std::string(FPL_BAMOUT_HEADER_HD) + read_groups + FPL_BAMOUT_HEADER_PG);
}
std::string bam_read_group_lines(const std::string& header_text) {
    const size_t end = std::min(header_text.size(), header_text.find('\0'));
    std::string out;
    for (size_t at = 0; at < end;) {
        const size_t nl = header_text.find('\n', at);
        const size_t e = nl == std::string::npos || nl >= end ? end : nl + 1;
        if (e - at >= 4 && header_text.compare(at, 4, "@RG\t") == 0) out.append(header_text, at, e - at);
        at = e;
    }
    if (!out.empty() && out.back() != '\n') out += '\n';
    return out;
}

size_t fastq_record_count(const std::string& text) {
    return (size_t)std::count(text.begin(), text.end(), '\n') / 4;
}

void fastq_to_bam_records(const std::string& text, std::string& out) { fastq_to_bam_records(text, nullptr, 0, out, nullptr); }

void fastq_to_bam_records(const std::string& text, const BamTagSrc* src, size_t n_src, std::string& out, uint64_t* stats, uint64_t* mod_stats,
                          uint64_t* move_stats) {
    size_t k = 0; /* the record's place in the text */
    static const struct Table {
        uint8_t t[256];
        Table() { rule::base_table(t); }
    } tab;
    const uint8_t* p = (const uint8_t*)text.data();
    const uint8_t* const end = p + text.size();
    auto line_end = [&](const uint8_t* at) {
        const uint8_t* e = (const uint8_t*)memchr(at, '\n', (size_t)(end - at));
        return e ? e : end;
    };
    while (p < end) {
        const uint8_t* name_e = line_end(p);
        const uint8_t* seq = name_e < end ? name_e + 1 : end;
        const uint8_t* seq_e = line_end(seq);
        const uint8_t* plus = seq_e < end ? seq_e + 1 : end;
        const uint8_t* plus_e = line_end(plus);
        const uint8_t* qual = plus_e < end ? plus_e + 1 : end;
        const uint8_t* qual_e = line_end(qual);
        /* the name line without its first byte, the '@' */
        const uint8_t* rest = p < name_e ? p + 1 : name_e;
        const uint32_t rest_len = (uint32_t)std::min<size_t>((size_t)(name_e - rest), rule::NAME_BYTES);
        const uint32_t cut = rule::name_cut(rest, rest_len, 0);
        const uint32_t nl = rule::name_len(0, cut);
        const uint32_t l_seq = (uint32_t)(seq_e - seq);
        const size_t at = out.size();
        out.resize(at + (size_t)rule::record_len(nl, l_seq));
        uint8_t* d = (uint8_t*)&out[at];
        for (uint32_t k = 0; k < 9; k++) {
            const uint32_t w = rule::fixed_word(k, nl, l_seq);
            for (int b = 0; b < 4; b++) d[4 * k + b] = (uint8_t)(w >> (8 * b));
        }
        d += rule::FIXED;
        if (cut) memcpy(d, rest, cut);
        else d[0] = '*';
        d[nl] = 0;
        d += nl + 1;
        for (uint32_t i = 0; i + 1 < l_seq; i += 2) *d++ = (uint8_t)((tab.t[seq[i]] << 4) | tab.t[seq[i + 1]]);
        if (l_seq & 1u) *d++ = (uint8_t)(tab.t[seq[l_seq - 1]] << 4);
        /* (a quality line shorter than the bases -- no formatter writes one -- is filled with phred 0) */
        const uint32_t n_q = (uint32_t)std::min<size_t>((size_t)(qual_e - qual), l_seq);
        for (uint32_t i = 0; i < n_q; i++) d[i] = (uint8_t)rule::qual_code(qual[i]);
        for (uint32_t i = n_q; i < l_seq; i++) d[i] = 0;
        if (k < n_src && src[k].rec) { /* (d is no use behind this: out grows) */
            const uint64_t bs = rule::record_len(nl, l_seq) - 4u + bam_record_tags(src[k], out, stats, mod_stats, move_stats);
            for (int b = 0; b < 4; b++) out[at + (size_t)b] = (char)(bs >> (8 * b));
        }
        k++;
        p = qual_e < end ? qual_e + 1 : end;
    }
}

}  // namespace fplh
