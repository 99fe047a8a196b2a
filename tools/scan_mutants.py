#!/usr/bin/env python3
"""Do the directed scan tests bite?  CPU only, not part of the test run.

For every entry of MUTANTS: copy the tree's sources to a temporary directory, apply the entry's edits to fastplong_amd/csrc/kernels.h there
(each search text must occur exactly as often as the entry says: a stale entry fails loudly), run ONLY tests/test_scan_emu.py in
the copy -- the emulator library builds itself from the mutated header -- and report: survived, or killed and by what (a failed
assertion, a crash of the emulator, a time-out) and in which test first (tools/mutant_runner.py, shared with tools/stats_mutants.py).
Exit status 0 when every mutant was killed by an assertion.

    python tools/scan_mutants.py [-j JOBS] [--only NAME ...] [-k EXPR] [--markdown] [--with-crashing]

docs/kernels.md ("Directed tests for the middle-adapter scan") holds the table this prints with --markdown."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutant_runner  # noqa: E402

HEADER = os.path.join("fastplong_amd", "csrc", "kernels.h")
TESTS = os.path.join("tests", "test_scan_emu.py")

# name, what it does, [(search text, replacement, number of sites)]
MUTANTS = [
    ("pg_n", "code planes: an N in the read counts as a G",
     [("PG = cH & cL & ~cN;", "PG = cH & cL;", 1)]),
    ("fold16", "the 16-bit pair of N count and complexity sum, one length too far",
     [("if (!LEAN && blen < 65536)", "if (!LEAN && blen <= 65536)", 1)]),
    ("ripple_top", "match_counts: carries never reach the top count plane",
     [("for (int b = 3; b < NB; b++) {\n            if (b < lvl) continue;", "for (int b = 3; b < NB - 1; b++) {\n            if (b < lvl) continue;", 1)]),
    ("v_all", "build_planes: every byte is a valid base",
     [("const u32 V = ~X;", "const u32 V = ~0u;", 1)]),
    ("tie_ge", "a lane's later tile wins a tie",
     [("} else if (val > bm0) {", "} else if (val >= bm0) {", 1)]),
    ("byte_tie", "byte-wise scan: a later window wins a tie",
     [("if (j0 + j < npos0 && mm < bmm0) {", "if (j0 + j < npos0 && mm <= bmm0) {", 1)]),
    ("nv_plus1", "the last tile tests one window too many",
     [("const int nv = npos0 - j0;", "const int nv = npos0 - j0 + 1;", 1)]),
    # (the key and its decoding together: the key's half alone decodes to a position outside the read, and the emulator then dies
    #  of the access instead of failing an assertion)
    ("tie_lane", "across lanes the LARGEST position wins a tie",
     [("const u32 k0 = wave_max_u32(((u32)(bm0 + 1) << 24) | (0xFFFFFFu - (u32)bp0));", "const u32 k0 = wave_max_u32(((u32)(bm0 + 1) << 24) | (u32)bp0);", 1),
      ("if (m0) key0 = ((u64)(u32)(ad0->len - (int)(m0 - 1)) << 32) | (0xFFFFFFu - (k0 & 0xFFFFFFu));",
       "if (m0) key0 = ((u64)(u32)(ad0->len - (int)(m0 - 1)) << 32) | (k0 & 0xFFFFFFu);", 1)]),
    ("npct_ge", "filter_code: the N percentage limit with >= for >",
     [("else if ((long long)sm.nn * 100 > (long long)len * cfg->n_pct_limit)", "else if ((long long)sm.nn * 100 >= (long long)len * cfg->n_pct_limit)", 1)]),
    ("q20_gt", "the statistics passes' Q20 limit with > for >=",
     [("(q >= '5')", "(q > '5')", 4)]),
    # ---- further ones ----
    ("cp_nbit", "code_planes: the N bit of every fourth base is lost",
     [("nb = udot4(w & 0x08080808u, wt, nb);", "nb = udot4(w & 0x08080800u, wt, nb);", 1)]),
    ("acgtn_diff_n", "sums32_acgtn: a G beside an N does not differ from it",
     [("const u32 dm = ((L ^ (L << 1)) | (H ^ (H << 1)) | (N ^ (N << 1))) & ~1u & vm;", "const u32 dm = ((L ^ (L << 1)) | (H ^ (H << 1))) & ~1u & vm;", 1)]),
    ("mc_c16", "match_counts: the sixteens carry enters one plane too high",
     [("ripple(c16, 4);", "ripple(c16, 5);", 1)]),
    ("mc_f2", "match_counts: the second fours carry of a group of eight is dropped",
     [("csa(e, B[2], B[2], f1, f2);", "csa(e, B[2], B[2], f1, 0u);", 1)]),
    ("sm_last", "sliced_max: the LAST position of a lane's chunk holding the maximum",
     [("first = __ffs(cand) - 1;", "first = 31 - __builtin_clz(cand);", 1)]),
    ("sm_low", "sliced_max: the lowest count plane is not looked at",
     [("for (int b = NB - 1; b >= 0; b--) { /* branch-free", "for (int b = NB - 1; b >= 1; b--) { /* branch-free", 1)]),
    ("pair_bm", "PairCarry: the best count of a read's head is forgotten",
     [("bm0 = pio->in.bm0;", "bm0 = -1;", 1)]),
    ("pair_bp", "PairCarry: the best position of a read's head is forgotten",
     [("bp0 = pio->in.bp0;", "bp0 = 0;", 1)]),
    ("pair_vm", "a head's lanes take the host read's mask of testable windows",
     [("if (head) vm = act_mask; /* (a head is followed by more of its read than any window is long) */\n                    if (vm) {\n                        int val, first;\n                        sliced_max(B, vm, val, first);\n                        if (packed && head) { /* (its first and only tile so far) */\n                            h_bm0 = val;",
       "if (vm) {\n                        int val, first;\n                        sliced_max(B, vm, val, first);\n                        if (packed && head) { /* (its first and only tile so far) */\n                            h_bm0 = val;", 1)]),
    ("tie_ge1", "a lane's later tile wins a tie, second adapter",
     [("} else if (val > bm1) {", "} else if (val >= bm1) {", 1)]),
    ("byte_tie1", "byte-wise scan: a later window wins a tie, second adapter",
     [("if (j0 + j < npos1 && mm < bmm1) {", "if (j0 + j < npos1 && mm <= bmm1) {", 1)]),
    ("pair_bm1", "PairCarry: the best count of a read's head is forgotten, second adapter",
     [("bm1 = pio->in.bm1;", "bm1 = -1;", 1)]),
    ("redo_right", "k_redo: the right piece is scanned from one base early",
     [("const int fa = f == 0 ? s : (f == 1 ? s + gs + glen : s + gs);", "const int fa = f == 0 ? s : (f == 1 ? s + gs + glen - 1 : s + gs);", 1)]),
    ("redo_left", "k_redo: the left piece is scanned one base short",
     [("const int flen = f == 0 ? len1 : (f == 1 ? len2 : glen);", "const int flen = f == 0 ? len1 - 1 : (f == 1 ? len2 : glen);", 1)]),
]

# The issue's own form of tie_lane, the key without its decoding: NOT part of the count above.  It decodes to a position far
# outside the read and the emulator dies of the access, so it is stopped by a crash, whatever the tests assert; run and reported
# (--with-crashing) so that the record of it does not rest on a document alone.
CRASHING = [
    ("tie_lane_key", "tie_lane's key alone, decoded as before: a position outside the read",
     [MUTANTS[7][2][0]]),
]


def _entry(m):
    """the runner's form of an entry: every edit names its file"""
    return m[0], m[1], [(HEADER,) + e for e in m[2]]


def main():
    ap = mutant_runner.arguments(TESTS)
    ap.add_argument("--with-crashing", action="store_true", help="also run CRASHING, which must be stopped by a crash")
    a = ap.parse_args()
    bad = mutant_runner.run_table([_entry(m) for m in MUTANTS], TESTS, a)
    if a.with_crashing:
        for name, what, how, test in (mutant_runner.run_mutant(_entry(m), TESTS) for m in CRASHING):
            print("%-13s %-28s %s   (expected: a crash)" % (name, how, test))
            if not how.startswith("crash"):
                bad.append(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
