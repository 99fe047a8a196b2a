#!/usr/bin/env python3
"""Do the directed tests of the partial-pattern searches and the edit-distance confirmations bite?  CPU only, not part of the test run.

For every entry of MUTANTS: copy the tree's sources to a temporary directory, apply the entry's one-line edit of
fastplong_amd/csrc/kernels.h there (its search text must occur exactly as often as the entry says), run ONLY
tests/test_partial_emu.py in the copy and report: survived, or killed and by what, and in which test first (tools/mutant_runner.py).
Exit status 0 when every mutant was killed by an assertion.

    python tools/partial_mutants.py [-j JOBS] [--only NAME ...] [-k EXPR] [--markdown] [--tests FILE] [--with-crashing]

--tests tests/test_kernels_emu.py (or tests/test_trim_scan_emu.py) asks the same of the emulator tests that were there before.
docs/kernels.md ("Directed tests for the partial-pattern searches and the edit-distance confirmations") holds the tables as printed
with --markdown.

Left out as equivalent: `(mm - t)` style slack in an exit bound of lev_round32 / lev_round64 (the loop only exits later, the result is
exact either way); `it == PART_CAND_CAP + 1` (a cap one round long gives the same results: it only moves one counter); `ed <= mined`
for `edb > mined` rewritten as `edb >= mined + 1`; any change of WHICH lanes run lev16_lanes without `ok` (their result is not read).
Also left out: `left_after` dropped in lev_round32 (the end trims confirm m <= 32 pattern columns against a text of the same length:
one round, left_after = 0; only lev_round64 sees a second round, with the 70-base adapter)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutant_runner  # noqa: E402

K = os.path.join("fastplong_amd", "csrc", "kernels.h")
TESTS = os.path.join("tests", "test_partial_emu.py")

# name, what it does, [(file, search text, replacement, number of sites)]
MUTANTS = [
    # ---- lev_lanes32 / lev_lanes64
    ("ll_lt_thr", "lev_lanes32 / lev_lanes64: score < thr",
     [(K, "    return need && score <= thr;", "    return need && score < thr;", 2)]),
    ("ll32_topsh", "lev_lanes32: topsh = mm",
     [(K, "    const u32 mask = mm >= 32 ? ~0u : ((1u << mm) - 1u);\n    const u32 topsh = mm > 0 ? (u32)(mm - 1) : 0u;",
       "    const u32 mask = mm >= 32 ? ~0u : ((1u << mm) - 1u);\n    const u32 topsh = mm > 0 ? (u32)(mm) : 0u;", 1)]),
    ("ll64_topsh", "lev_lanes64: topsh = mm",
     [(K, "    const u64 mask = mm >= 64 ? ~0ull : ((1ull << mm) - 1ull);\n    const u32 topsh = mm > 0 ? (u32)(mm - 1) : 0u;",
       "    const u64 mask = mm >= 64 ? ~0ull : ((1ull << mm) - 1ull);\n    const u32 topsh = mm > 0 ? (u32)(mm) : 0u;", 1)]),
    ("ll32_mask", "lev_lanes32: the mask one bit short",
     [(K, "    const u32 mask = mm >= 32 ? ~0u : ((1u << mm) - 1u);", "    const u32 mask = mm >= 33 ? ~0u : ((1u << (mm - 1)) - 1u);", 1)]),
    ("ll64_mask", "lev_lanes64: the mask one bit short",
     [(K, "    const u64 mask = mm >= 64 ? ~0ull : ((1ull << mm) - 1ull);", "    const u64 mask = mm >= 65 ? ~0ull : ((1ull << (mm - 1)) - 1ull);", 1)]),
    ("ll32_act", "lev_lanes32: act = t <= mm",
     [(K, "            const bool act = t < mm; /* this lane's text has a column t */\n            score = act ? sc : score;\n            const u32 nPv",
       "            const bool act = t <= mm; /* this lane's text has a column t */\n            score = act ? sc : score;\n            const u32 nPv", 1)]),
    ("ll64_act", "lev_lanes64: act = t <= mm",
     [(K, "            const bool act = t < mm; /* this lane's text has a column t */\n            score = act ? sc : score;\n            const u64 nPv",
       "            const bool act = t <= mm; /* this lane's text has a column t */\n            score = act ? sc : score;\n            const u64 nPv", 1)]),
    ("ll32_shift", "lev_lanes32: the shift ignored",
     [(K, "            const u32 Eq = (u32)(peqf[c][0] >> shift) & mask;", "            const u32 Eq = (u32)(peqf[c][0]) & mask;", 1)]),
    ("ll64_shift", "lev_lanes64: the shift ignored",
     [(K, "            const u64 Eq = (peqf[c][0] >> shift) & mask;", "            const u64 Eq = (peqf[c][0]) & mask;", 1)]),
    ("ll64_block", "lev_lanes64: a 16-byte block skipped when t0 + 16 >= mm",
     [(K, "    int score = mm;\n    for (int t0 = 0; t0 < mmax; t0 += 16) { /* wave-uniform */\n        u32 w[4] = {0, 0, 0, 0};\n        if (need && t0 < mm) {",
       "    int score = mm;\n    for (int t0 = 0; t0 < mmax; t0 += 16) { /* wave-uniform */\n        u32 w[4] = {0, 0, 0, 0};\n        if (need && t0 + 16 < mm) {", 1)]),
    ("ll32_block", "lev_lanes32: the second 16-byte block left out",
     [(K, "        const u32x4 a = load16_guard(text, seq_end), b = load16_guard(text + 16, seq_end);\n        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;\n        w[4] = b.x;",
       "        const u32x4 a = load16_guard(text, seq_end), b = load16_guard(text, seq_end);\n        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;\n        w[4] = b.x;", 1)]),
    # ---- lev_round32 / lev_round64
    ("lr32_ge", "lev_round32: the exits with >= thr",
     [(K, "        if (score - (left_after + cnt - FPL_LEV_UNROLL - t) > thr) return true; /* wave-uniform */",
       "        if (score - (left_after + cnt - FPL_LEV_UNROLL - t) >= thr) return true; /* wave-uniform */", 1),
      (K, "    if (score - left_after > thr) return true;", "    if (score - left_after >= thr) return true;", 1)]),
    ("lr64_ge", "lev_round64: the exit with >= thr",
     [(K, "        if (score - (left_after + cnt - 1 - t) > thr) return true;", "        if (score - (left_after + cnt - 1 - t) >= thr) return true;", 1)]),
    ("lr64_left", "lev_round64: left_after dropped",
     [(K, "        if (score - (left_after + cnt - 1 - t) > thr) return true;", "        if (score - (cnt - 1 - t) > thr) return true;", 1)]),
    # ---- partial16_candidates
    ("pc_x", "partial16_candidates: x = 16 - thr",
     [(K, "    int x = 16 - (thr + 1);", "    int x = 16 - thr;", 1)]),
    ("pc_ph14", "partial16_candidates: Ph >> 14",
     [(K, "            x += (int)((Ph >> 15) & 1u) - (int)((Mh >> 15) & 1u);\n            Ph <<= 1;\n            Pv = lshl_or<1>",
       "            x += (int)((Ph >> 14) & 1u) - (int)((Mh >> 15) & 1u);\n            Ph <<= 1;\n            Pv = lshl_or<1>", 1)]),
    ("pc_nv", "partial16_candidates: the nv mask one column long",
     [(K, "(nv >= 16 ? 0xFFFFu : (nv <= 0 ? 0u : ((1u << nv) - 1u)));", "(nv >= 15 ? 0xFFFFu : (nv < 0 ? 0u : ((2u << nv) - 1u)));", 1)]),
    ("pc_tail", "partial16_candidates: the tail word dropped",
     [(K, "    if (nmax > 0 && !((nmax - 1) & 16)) { /* the last block was the low half of its word */",
       "    if (false && nmax > 0 && !((nmax - 1) & 16)) { /* the last block was the low half of its word */", 1)]),
    ("pc_halves", "partial16_candidates: the halves of a word swapped",
     [(K, "            const u32 word = lo | (h << 16);", "            const u32 word = h | (lo << 16);", 1)]),
    # ---- partial16_resolve_lanes
    ("pr_start_le", "partial16_resolve_lanes: ed <= mined at the start",
     [(K, "                if (ed < mined) { /* (ascending p: the first of equals stays) */", "                if (ed <= mined) { /* (ascending p: the first of equals stays) */", 1)]),
    ("pr_end_lt", "partial16_resolve_lanes: ed < mined at the end",
     [(K, "            } else if (pos < 0 || ed <= mined) {", "            } else if (pos < 0 || ed < mined) {", 1)]),
    ("pr_lim", "partial16_resolve_lanes: p <= lim",
     [(K, "        const bool ok = has && p >= 0 && p < lim;", "        const bool ok = has && p >= 0 && p <= lim;", 1)]),
    ("pr_p16", "partial16_resolve_lanes: p = j - 16",
     [(K, "        const int p = START ? j - 15 : n - 1 - j;", "        const int p = START ? j - 16 : n - 1 - j;", 1)]),
    ("pr_pend", "partial16_resolve_lanes: p = n - j at the end",
     [(K, "        const int p = START ? j - 15 : n - 1 - j;", "        const int p = START ? j - 15 : n - j;", 1)]),
    ("pr_over", "partial16_resolve_lanes: over = false",
     [(K, "            over = has;\n            break;", "            over = false;\n            break;", 1)]),
    ("pr_cap", "partial16_resolve_lanes: the cap one round short",
     [(K, "        if (it == PART_CAND_CAP) {", "        if (it == PART_CAND_CAP - 1) {", 1)]),
    ("pr_words", "partial16_resolve_lanes: the word order reversed",
     [(K, "            k = START ? (int)__ffs((int)nz) - 1 : 31 - (int)__clz((int)nz);", "            k = !START ? (int)__ffs((int)nz) - 1 : 31 - (int)__clz((int)nz);", 1)]),
    ("pr_stop", "partial16_resolve_lanes: the stop rule dropped",
     [(K, "            } else {\n                stop = true;\n            }\n        }\n        if (stop) {", "            } else {\n                stop = false;\n            }\n        }\n        if (stop) {", 1)]),
    # ---- P4 / P8 of k_trim_ends_batched
    ("p4_thrA", "P4: thrA0 for thr[cmplen]",
     [(K, "cmplen, alen0 - cmplen, thr_lds[need ? cmplen : 0], need,", "cmplen, alen0 - cmplen, thrA0, need,", 1)]),
    ("p8_thrA", "P8: thrA1 for thr[cmplen]",
     [(K, "(rlen - plen - v_ppos), cmplen, 0, thr_lds[need ? cmplen : 0], need, lds.peqf[1],", "(rlen - plen - v_ppos), cmplen, 0, thrA1, need, lds.peqf[1],", 1)]),
    ("p4_shift", "P4: the shift alen - cmplen dropped",
     [(K, "cmplen, alen0 - cmplen, thr_lds[need ? cmplen : 0], need,", "cmplen, 0, thr_lds[need ? cmplen : 0], need,", 1)]),
    ("p4_min", "P4: the min(.., rlen - alen) dropped",
     [(K, "                const int pos = min(v_ppos + ext, rlen - alen0);", "                const int pos = v_ppos + ext;", 1)]),
    ("p4_min_plen", "P4: min(.., rlen - plen) for rlen - alen",
     [(K, "                const int pos = min(v_ppos + ext, rlen - alen0);", "                const int pos = min(v_ppos + ext, rlen - plen);", 1)]),
    ("p8_min", "P8: the min(.., rlen - plen) dropped",
     [(K, "                const int pos = min(v_ppos + ext, rlen - plen);", "                const int pos = v_ppos + ext;", 1)]),
    ("p8_min_alen", "P8: min(.., rlen - alen) for rlen - plen",
     [(K, "                const int pos = min(v_ppos + ext, rlen - plen);", "                const int pos = min(v_ppos + ext, rlen - alen1);", 1)]),
    ("p4_neg", "P4: if (n < 0) dropped",
     [(K, "                if (n < 0) v_s = v_e;\n                else v_s += n;", "                v_s += n;", 1)]),
    ("p7_pos0", "P7, lane form: pos >= 0 for pos > 0",
     [(K, "                    v_ppos = pos > 0 ? pos : -1; /* :288 strict */", "                    v_ppos = pos >= 0 ? pos : -1; /* :288 strict */", 1)]),
    ("p7w_pos0", "P7, wave fallback: pos >= 0 for pos > 0",
     [(K, "                lane_set(v_ppos, j, pos > 0 ? pos : -1); /* :288 strict */", "                lane_set(v_ppos, j, pos >= 0 ? pos : -1); /* :288 strict */", 1)]),
    ("p7w_ge", "P7, wave fallback: edb >= mined",
     [(K, "                        } else if (edb > mined) {\n                            stop = true;", "                        } else if (edb >= mined) {\n                            stop = true;", 1)]),
    ("p3w_key", "P3, wave fallback: the key with ed and p swapped",
     [(K, "                            const u64 k = ((u64)(u32)ed[u] << 32) | (u32)pp[u];\n                            best = k < best ? k : best;\n                        }\n                }\n                best = wave_min_u64(best);\n                lane_set",
       "                            const u64 k = ((u64)(u32)pp[u] << 32) | (u32)ed[u];\n                            best = k < best ? k : best;\n                        }\n                }\n                best = wave_min_u64(best);\n                lane_set", 1)]),
    # ---- trim_start_wave / trim_end_wave
    ("tw_thrA", "both wave forms: thrA for thr[cmplen]",
     [(K, "        if (ed <= cfg->thr[cmplen]) {", "        if (ed <= thrA) {", 2),
      (K, "win, pos + plen - cmplen, cmplen, cfg->thr[cmplen]);", "win, pos + plen - cmplen, cmplen, thrA);", 1),
      (K, "win, rlen - plen - pos, cmplen, cfg->thr[cmplen]);", "win, rlen - plen - pos, cmplen, thrA);", 1)]),
    ("tsw_shift", "trim_start_wave: the shift alen - cmplen dropped",
     [(K, "lev_wave_win<MODE>(peqf, alen - cmplen, cmplen, win,", "lev_wave_win<MODE>(peqf, 0, cmplen, win,", 1)]),
    ("tsw_min", "trim_start_wave: the min(.., rlen - alen) dropped",
     [(K, "            pos = min(pos + ext, rlen - alen);", "            pos = pos + ext;", 1)]),
    ("tew_min", "trim_end_wave: min(.., rlen - alen) for rlen - plen",
     [(K, "            pos = min(pos + ext, rlen - plen);", "            pos = min(pos + ext, rlen - alen);", 1)]),
    ("tsw_neg", "trim_start_wave: if (n < 0) dropped",
     [(K, "            if (n < 0) s = e;\n            else s += n;", "            s += n;", 1)]),
    ("tew_pos0", "trim_end_wave: pos >= 0 for pos > 0",
     [(K, "    if (pos > 0) { /* :288 strict */", "    if (pos >= 0) { /* :288 strict */", 1)]),
    ("tew_ge", "trim_end_wave: edb >= mined",
     [(K, "            } else if (edb > mined) {\n                stop = true;", "            } else if (edb >= mined) {\n                stop = true;", 1)]),
    ("tsw_key", "trim_start_wave: the key with ed and p swapped",
     [(K, "                const u64 k = ((u64)(u32)ed[u] << 32) | (u32)pp[u];\n                best = k < best ? k : best;\n            }\n    }\n    best = wave_min_u64(best);\n    if (best != ~0ull) { /* :218-233 */\n        int pos = (int)(u32)best;",
       "                const u64 k = ((u64)(u32)pp[u] << 32) | (u32)ed[u];\n                best = k < best ? k : best;\n            }\n    }\n    best = wave_min_u64(best);\n    if (best != ~0ull) { /* :218-233 */\n        int pos = (int)(u32)(best >> 32);", 1)]),
    ("tsw_hint", "trim_start_wave, hinted round: p < hint_hi",
     [(K, "        if (p <= hint_hi && p < lim && ed <= thrP) best", "        if (p < hint_hi && p < lim && ed <= thrP) best", 1)]),
    ("tew_hint", "trim_end_wave, hinted round: the last position left out",
     [(K, "last = one_round ? min(lim, hint_hi + 1) : lim;", "last = one_round ? min(lim, hint_hi) : lim;", 1)]),
]

MUTANTS += [
    # ---- the confirmations of k_resolve
    ("g32_lt", "lev_lanes32_acgt_w: the exit test with < thr",
     [(K, "                alive = alive && score - (mm - 1 - t) <= thr;", "                alive = alive && score - (mm - 1 - t) < thr;", 1)]),
    ("g64_lt", "lev_lanes64_acgt: the exit test with < thr",
     [(K, "alive = alive && (t >= mm || score - (mm - 1 - t) <= thr);", "alive = alive && (t >= mm || score - (mm - 1 - t) < thr);", 1)]),
    ("g32_m2", "lev_lanes32_acgt_w: (mm - 2 - t)",
     [(K, "                alive = alive && score - (mm - 1 - t) <= thr;", "                alive = alive && score - (mm - 2 - t) <= thr;", 1)]),
    ("g64_m2", "lev_lanes64_acgt: (mm - 2 - t)",
     [(K, "alive = alive && (t >= mm || score - (mm - 1 - t) <= thr);", "alive = alive && (t >= mm || score - (mm - 2 - t) <= thr);", 1)]),
    ("g_ret_lt", "lev_lanes32_acgt_w / lev_lanes64_acgt: score < thr in the end",
     [(K, "    return alive && score <= thr;", "    return alive && score < thr;", 2)]),
    ("g32_peq4", "peq4_lookup without the letter check",
     [(K, "== b ? tbl[code] : 0u;", "== b || true ? tbl[code] : 0u;", 1)]),
    ("g64_peq4", "peq4_lookup64 without the letter check",
     [(K, "== b ? tbl[code] : 0ull;", "== b || true ? tbl[code] : 0ull;", 1)]),
    ("g_any_thr", "lev_lanes_any: ed < thr",
     [(K, "        if (lane_id() == j) ok = ed <= thr;", "        if (lane_id() == j) ok = ed < thr;", 1)]),
    # ---- one window less: of the 184, and where r1 ends
    ("tw_lim184", "both wave forms: 183 windows",
     [(K, "    const int lim = may_part ? min(rlen - plen, FPL_END_WINDOW - plen) : 0;", "    const int lim = may_part ? min(rlen - plen, FPL_END_WINDOW - plen - 1) : 0;", 2)]),
    ("lane_lim184", "P3 / P7, lane form: 183 windows",
     [(K, "n, min(rl - plen, FPL_END_WINDOW - plen), thrP, nzc,", "n, min(rl - plen, FPL_END_WINDOW - plen - 1), thrP, nzc,", 1),
      (K, "wlf, min(rl - plen, FPL_END_WINDOW - plen), thrP,", "wlf, min(rl - plen, FPL_END_WINDOW - plen - 1), thrP,", 1)]),
    ("tw_lim_r", "both wave forms: rlen - plen - 1 windows",
     [(K, "    const int lim = may_part ? min(rlen - plen, FPL_END_WINDOW - plen) : 0;", "    const int lim = may_part ? min(rlen - plen - 1, FPL_END_WINDOW - plen) : 0;", 2)]),
    ("lane_lim_r", "P3 / P7, lane form: rl - plen - 1 windows",
     [(K, "n, min(rl - plen, FPL_END_WINDOW - plen), thrP, nzc,", "n, min(rl - plen - 1, FPL_END_WINDOW - plen), thrP, nzc,", 1),
      (K, "wlf, min(rl - plen, FPL_END_WINDOW - plen), thrP,", "wlf, min(rl - plen - 1, FPL_END_WINDOW - plen), thrP,", 1)]),
]

CRASHING = []  # edits that stop the emulator with a crash or a time-out rather than a failed assertion: asked for by name


def main():
    ap = mutant_runner.arguments(TESTS)
    ap.add_argument("--tests", default=TESTS, help="the test file to run against the mutants (default: %s)" % TESTS)
    ap.add_argument("--with-crashing", action="store_true", help="also the edits that stop the emulator with a crash")
    a = ap.parse_args()
    return 1 if mutant_runner.run_table(MUTANTS + (CRASHING if a.with_crashing else []), a.tests, a) else 0


if __name__ == "__main__":
    sys.exit(main())
