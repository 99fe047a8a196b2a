#!/usr/bin/env python3
"""Do the directed tests of the packed statistics counters bite?  CPU only, not part of the test run.

For every entry of MUTANTS: copy the tree's sources to a temporary directory, apply the entry's edits there (to kernels.h or to
pipeline.h: every edit names its file, and its search text must occur exactly as often as the entry says), run ONLY
tests/test_stats_emu.py in the copy and report: survived, or killed and by what, and in which test first (tools/mutant_runner.py).
Exit status 0 when every mutant was killed by an assertion.

    python tools/stats_mutants.py [-j JOBS] [--only NAME ...] [-k EXPR] [--markdown] [--tests FILE]

--tests tests/test_kernels_emu.py asks the same of the emulator tests that were there before (-k picks a part of either file).
docs/kernels.md ("Directed tests for the packed statistics counters") holds both tables as printed with --markdown."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutant_runner  # noqa: E402

K = os.path.join("fastplong_amd", "csrc", "kernels.h")
P = os.path.join("fastplong_amd", "csrc", "pipeline.h")
TESTS = os.path.join("tests", "test_stats_emu.py")

# name, what it does, [(file, search text, replacement, number of sites)]
MUTANTS = [
    ("group_never", "k_stats_sorted: a group's slab is never handed over in pieces",
     [(K, "if (open && held + rows > max_rows) {", "if (false && open && held + rows > max_rows) {", 1)]),
    ("group_plus1", "k_stats_sorted: a group's slab takes one row too many",
     [(K, "if (open && held + rows > max_rows) {", "if (open && held + rows > max_rows + 1) {", 1)]),
    ("extra_never", "k_stats<EXTRA>: the tables are never emptied",
     [(K, "if (EXTRA && ready && acc + items_per_slice > max_acc) {", "if (false && EXTRA && ready && acc + items_per_slice > max_acc) {", 1)]),
    ("extra_plus1", "k_stats<EXTRA>: the tables take one item too many",
     [(K, "if (EXTRA && ready && acc + items_per_slice > max_acc) {", "if (EXTRA && ready && acc + items_per_slice > max_acc + 1) {", 1)]),
    ("cnt_12", "fs_unpack_add: the count field unpacked 12 bits wide",
     [(K, "cnt += (v >> 22) & 0x3FFF;", "cnt += (v >> 22) & 0x0FFF;", 1)]),
    ("q20_13", "fs_unpack_add: the Q20 field unpacked 13 bits wide",
     [(K, "q20 += (v >> 36) & 0x3FFF;", "q20 += (v >> 36) & 0x1FFF;", 1)]),
    ("q30_13", "fs_unpack_add: the Q30 field unpacked 13 bits wide",
     [(K, "q30 += v >> 50;", "q30 += (v >> 50) & 0x1FFF;", 1)]),
    ("qsum_20", "fs_unpack_add: the quality sum unpacked 20 bits wide",
     [(K, "qsum += v & 0x3FFFFF;", "qsum += v & 0x0FFFFF;", 1)]),
    ("per_16384", "stats_items_per_slice: slices of up to 16 384 reads",
     [(P, "constexpr u32 per_max = CS_MAX_ITEMS_PER_SLICE / 64 * 64;", "constexpr u32 per_max = 16384;", 1)]),
    ("rows_clamp", "enqueue_batch: FPL_STATS_GROUP_ROWS is taken as it is",
     [(P, "        if (max_rows > CS_MAX_ITEMS_PER_SLICE) max_rows = CS_MAX_ITEMS_PER_SLICE;\n", "", 1)]),
    ("k6_last", "kmer_flush: the 6-mers that END with the 5-mer and start with an A are left out",
     [(K, "k6[4 * i + 3] + k6[i] + k6[i + 1024]", "k6[4 * i + 3] + k6[i + 1024]", 1)]),
]


def main():
    ap = mutant_runner.arguments(TESTS)
    ap.add_argument("--tests", default=TESTS, help="the test file to run against the mutants (default: %s)" % TESTS)
    a = ap.parse_args()
    return 1 if mutant_runner.run_table(MUTANTS, a.tests, a) else 0


if __name__ == "__main__":
    sys.exit(main())
