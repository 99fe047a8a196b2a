/*
 * TEST INFRASTRUCTURE ONLY -- fmt_float of fastplong_amd/csrc/bam_comment_rules.h against this machine's libc, as a program of
 * its own under AddressSanitizer and UndefinedBehaviorSanitizer: for every input, fmt_float(v) must be the bytes of
 * snprintf("%g", (double)v).  The inputs, for every exponent 0..255 and both signs: the mantissas 0, 1, 0x400000, 0x7FFFFF and
 * 4096 seeded random ones; every n + 0.5 for n in [100000, 999999] (the exact ties at six digits); every 10 k + 5 in
 * [1000005, 9999995].  `prog in out`: in holds the seed (u64); out gets three u64 -- values checked, mismatches, the longest
 * text -- and a line of text per mismatch (the first 20).
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../fastplong_amd/csrc/bam_comment_rules.h"

namespace {
uint64_t checked = 0, bad = 0, longest = 0;
std::string report;

void check_bits(uint32_t bits) {
    float v;
    memcpy(&v, &bits, 4);
    char want[64], got[fpl::bamcomment::FLOAT_TEXT_MAX + 1];
    const int wn = snprintf(want, sizeof want, "%g", (double)v);
    const uint32_t gn = fpl::bamcomment::fmt_float(bits, got); /* (past FLOAT_TEXT_MAX bytes the sanitizer speaks) */
    got[gn] = 0;
    checked++;
    if (gn > longest) longest = gn;
    if ((int)gn != wn || memcmp(want, got, gn) != 0) {
        if (bad++ < 20) {
            char line[160];
            snprintf(line, sizeof line, "%08x: libc '%s', fmt_float '%s'\n", bits, want, got);
            report += line;
        }
    }
}
void check_value(float v) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    check_bits(bits);
    check_bits(bits | 0x80000000u);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    uint64_t seed = 1;
    if (FILE* f = fopen(argv[1], "rb")) {
        if (fread(&seed, 8, 1, f) != 1) seed = 1;
        fclose(f);
    }
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&]() { /* xorshift64* */
        x ^= x >> 12, x ^= x << 25, x ^= x >> 27;
        return (uint32_t)((x * 0x2545F4914F6CDD1Dull) >> 40);
    };
    static const uint32_t fixed[4] = {0, 1, 0x400000u, 0x7FFFFFu};
    for (uint32_t sign = 0; sign < 2; sign++)
        for (uint32_t ex = 0; ex < 256; ex++) {
            const uint32_t hi = sign << 31 | ex << 23;
            for (uint32_t m : fixed) check_bits(hi | m);
            for (int k = 0; k < 4096; k++) check_bits(hi | (next() & 0x7FFFFFu));
        }
    for (uint32_t n = 100000; n <= 999999; n++) check_value((float)n + 0.5f); /* (exact: below 2^23) */
    for (uint32_t v = 1000005; v <= 9999995; v += 10) check_value((float)v);   /* (exact: below 2^24) */
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 3;
    const uint64_t head[3] = {checked, bad, longest};
    fwrite(head, 8, 3, o);
    fwrite(report.data(), 1, report.size(), o);
    return fclose(o) == 0 ? 0 : 3;
}
