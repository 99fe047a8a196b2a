#!/usr/bin/env python3
"""Do the directed tests of the quality cuts and the polyX scan bite?  CPU only, not part of the test run.

For every entry of MUTANTS: copy the tree's sources to a temporary directory, apply the entry's one-line edit of
fastplong_amd/csrc/kernels.h there (its search text must occur exactly as often as the entry says), run ONLY tests/test_cut_emu.py
in the copy and report: survived, or killed and by what, and in which test first (tools/mutant_runner.py).  Exit status 0 when every
mutant was killed by an assertion.

    python tools/cut_mutants.py [-j JOBS] [--only NAME ...] [-k EXPR] [--markdown] [--tests FILE]

--tests tests/test_kernels_emu.py asks the same of the emulator tests that were there before.  docs/kernels.md ("Directed tests for
the quality cuts and the polyX scan") holds both tables as printed with --markdown.

Left out as equivalent: `pos > 8` for `pos >= 8` in the lane loop and in the block steps (a break put off at position 8 is taken
at 9, and P + 1 < compareReq either way); `int i = rlen - P` in the way back (the base that stops the scan is never the dominant
one); any change of WHEN the block path is taken (the byte loop gives the same answer)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutant_runner  # noqa: E402

K = os.path.join("fastplong_amd", "csrc", "kernels.h")
TESTS = os.path.join("tests", "test_cut_emu.py")

# name, what it does, [(file, search text, replacement, number of sites)]
MUTANTS = [
    # ---- the six that the emulator tests of before did not notice
    ("tie_T", "trim_polyx_lanes: T wins a tie with A",
     [(K, "if (cT > maxc) { maxc = cT; poly = 1; }", "if (cT >= maxc) { maxc = cT; poly = 1; }", 1)]),
    ("lost_N", "trim_polyx_lanes, byte loop: an N beyond step 32 no longer counts for A",
     [(K, "        cA += (c == 'A' || c == 'N');", "        cA += (c == 'A');", 1)]),
    ("cf_past", "FPL_CF_STEP: the block steps of cut_front run one window past the last",
     [(K, "        const bool out = run && s >= lim; ", "        const bool out = run && s > lim;  ", 1)]),
    ("tail_n_front", "trim_and_cut_lanes: the tail's N skip stops at front",
     [(K, "        while (alive && !slow && t >= 0 && sq[t] == 'N') {", "        while (alive && !slow && t > front && sq[t] == 'N') {", 1)]),
    ("head_late", "k_trim_ends: the start window is staged again one byte late",
     [(K, "                if (s + wl > TRIM_WIN) {", "                if (s + wl > TRIM_WIN + 1) {", 1)]),
    ("tail_late", "k_trim_ends: the end window is staged again one byte late",
     [(K, "                if (e - wl < tail0) {", "                if (e - wl < tail0 - 1) {", 1)]),
    # ---- the ten that some random case of before happened to stop
    ("allow6_wave", "trim_polyx_wave: up to six mismatches",
     [(K, "        const int allowed = min(5, cmp / 8);", "        const int allowed = min(6, cmp / 8);", 1)]),
    ("allow6_lanes", "trim_polyx_lanes: up to six mismatches",
     [(K, "allowed = cmp / 8 < 5 ? cmp / 8 : 5; ", "allowed = cmp / 8 < 6 ? cmp / 8 : 6; ", 1),
      (K, "        const int cmp = pos + 1, allowed = min(5, cmp / 8);", "        const int cmp = pos + 1, allowed = min(6, cmp / 8);", 1)]),
    ("head_w", "trim_and_cut_wave: the head test forgets the window's width",
     [(K, "if (vq.in_head(s0, min(s0 + 63, lim - 1) + w - 1)) {", "if (vq.in_head(s0, min(s0 + 63, lim - 1))) {", 1)]),
    ("tail_w", "trim_and_cut_wave: the tail test forgets the window's width",
     [(K, "if (vq.in_tail(max(t0 - 63, tlow) - (w - 1), t0)) {", "if (vq.in_tail(max(t0 - 63, tlow), t0)) {", 1)]),
    ("px_tail_hi", "trim_polyx_wave: the tail test looks at the round's first byte only",
     [(K, "if (vs.in_tail(max(hi - 63, s0), hi)) {", "if (vs.in_tail(hi, hi)) {", 1)]),
    ("ct_short", "FPL_CT_STEP: the block steps of cut_tail stop one window early",
     [(K, "        const bool out = run && t - w < front; ", "        const bool out = run && t - w <= front;", 1)]),
    ("req_lanes", "trim_polyx_lanes: P < compareReq",
     [(K, "if (!active || slow || P + 1 < compareReq) return rlen;", "if (!active || slow || P < compareReq) return rlen;", 1)]),
    ("front_end", "trim_and_cut_lanes: front > l - 1",
     [(K, "    if (rlen <= 0 || front >= l - 1) alive = false;", "    if (rlen <= 0 || front > l - 1) alive = false;", 1)]),
    ("s_quirk", "both forms: `if (s > 0)` rewritten as `if (s > front)`",
     [(K, "        if (s > 0) s = s + w - 1;", "        if (s > front) s = s + w - 1;", 2)]),
    ("t_quirk", "both forms: `if (t < l - 1)` rewritten as `if (t < l - tail - 1)`",
     [(K, "        if (t < l - 1) t = t - w + 1;", "        if (t < l - tail - 1) t = t - w + 1;", 2)]),
    # ---- more of the same kind
    ("req_wave", "trim_polyx_wave: P < compareReq",
     [(K, "    if (P + 1 < compareReq) return rlen; /* :57 */", "    if (P < compareReq) return rlen; /* :57 */", 1)]),
    ("front_end_wave", "trim_and_cut_wave: front > l - 1",
     [(K, "    if (rlen <= 0 || front >= l - 1) return false;", "    if (rlen <= 0 || front > l - 1) return false;", 1)]),
    ("ct_byte", "FPL_CT_STEP: the tail block's entering byte taken one place low",
     [(K, "(int)byte16<15 - K>(A)", "(int)byte16<14 - K>(A)", 1)]),
    ("ct_warm", "trim_and_cut_lanes: the tail block's warm-up sums w bytes",
     [(K, "total = (int)sum_last_bytes(S, w - 1);", "total = (int)sum_last_bytes(S, w);", 1)]),
    ("px_block", "trim_polyx_lanes: the second block loaded one byte high",
     [(K, "R1 = load16(r + rlen - 32);", "R1 = load16(r + rlen - 31);", 1)]),
    ("px_carry", "trim_polyx_wave: the A count is not carried into the next round",
     [(K, "        carry[0] = cnt[0];", "        carry[0] = 0;", 1)]),
    ("px_src", "trim_polyx_wave: a round without a break hands on lane 62's counts",
     [(K, "const int src = m ? (__ffsll(m) - 1) : 63;", "const int src = m ? (__ffsll(m) - 1) : 62;", 1)]),
]


def main():
    ap = mutant_runner.arguments(TESTS)
    ap.add_argument("--tests", default=TESTS, help="the test file to run against the mutants (default: %s)" % TESTS)
    a = ap.parse_args()
    return 1 if mutant_runner.run_table(MUTANTS, a.tests, a) else 0


if __name__ == "__main__":
    sys.exit(main())
