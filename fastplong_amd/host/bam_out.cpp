/* bam_out.cpp -- see bam_out.h */
#include "bam_out.h"

#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../csrc/bam_out_rules.h"

namespace fplh {

namespace rule = fpl::bamout;

const std::string& bam_header_bytes() {
    static const std::string h = [] {
        const std::string text = FPL_BAMOUT_HEADER_TEXT;
        std::string s("BAM\1", 4);
        const uint32_t l_text = (uint32_t)text.size();
        for (int k = 0; k < 4; k++) s += (char)(l_text >> (8 * k));
        s += text;
        s.append(4, '\0'); /* n_ref */
        return s;
    }();
    return h;
}

void fastq_to_bam_records(const std::string& text, std::string& out) {
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
        p = qual_e < end ? qual_e + 1 : end;
    }
}

}  // namespace fplh
