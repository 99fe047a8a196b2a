/*
 * main.cpp -- TEST INFRASTRUCTURE ONLY (tests/host_bamout/host_bamout_run, built by tests/host_bamout/build.py).
 * The host's BAM output unit (fastplong_amd/host/bam_out.cpp) as a program of its own under -fsanitize=address,undefined:
 *   host_bamout_run <in> <out>    in: FASTQ text; out: bam_header_bytes(), then fastq_to_bam_records(text)
 * The text is held in a heap block of exactly its size, so a read past its end is a report.
 */
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../fastplong_amd/host/bam_out.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char* buf = (char*)malloc(n > 0 ? (size_t)n : 1);
    if (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    std::string text(buf, (size_t)n), out;
    text.shrink_to_fit();
    free(buf);
    fplh::fastq_to_bam_records(text, out);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const std::string& h = fplh::bam_header_bytes();
    fwrite(h.data(), 1, h.size(), f);
    fwrite(out.data(), 1, out.size(), f);
    return fclose(f) == 0 ? 0 : 2;
}
