"""The oracle's adapter code (oracle/fpl_oracle.c) and the second reading (tests/second_reading.py) against the REAL
AdapterTrimmer and Sequence objects of oracle/_ref/ref_harness -- compiled from the reference's own adaptertrimmer.cpp and
sequence.cpp against the scalar Highway stand-in of oracle/standin (skipped where the harness was not built).

Besides the seeded cases of tests/adapter_cases.py, exhaustive batteries aimed at where a window search goes wrong: every
adapter length 1-70 against reads one shorter to two longer than it, copies planted with exactly `thr` and `thr + 1`
mismatches, the best window at the last position p = rlen - alen (which the reference's default mode never visits),
equal-Hamming windows whose first fails the edit-distance confirmation, and ed_max values where ed_max * alen lands on .5."""
import numpy as np
import pytest

from fastplong_amd import synth
from tests import adapter_cases as ac
from tests import second_reading as sr

ED_MAX = [0.0, 0.1, 0.25, 0.3, 0.4, 0.5, 1.0]
MODES = ((False, False), (True, False), (False, True), (True, True))


def _subst(rng, ad, k):
    """`ad` with exactly k substitutions (at distinct positions, each to another base)"""
    b = bytearray(ad)
    for i in rng.choice(len(b), size=k, replace=False) if k else ():
        b[i] = b"ACGT"[("ACGT".index(chr(b[i])) + int(rng.integers(1, 4))) % 4] if chr(b[i]) in "ACGT" else ord("A")
    return bytes(b)


def _check_search(ref, orc, cases, second_every=0):
    """searchAdapter: reference == oracle on every case, == the second reading on every `second_every`-th"""
    want = ref.search_adapter(cases)
    for i, (c, w) in enumerate(zip(cases, want)):
        assert orc.search_adapter(*c) == w, c
        if second_every and i % second_every == 0:
            assert sr.search_adapter(*c) == w, c
    return want


def _check_trims(ref, orc, cases, second_every=0):
    """trimBySequenceStart / trimBySequenceEnd: the read left over, the value returned, the key length"""
    out = {}
    for name in ("trim_start", "trim_end"):
        want = getattr(ref, name)(cases)
        for i, (c, w) in enumerate(zip(cases, want)):
            got = getattr(orc, name)(*c)
            assert (got[0].encode("latin-1"), got[1], got[2]) == w, (name, c, got, w)
            if second_every and i % second_every == 0:
                assert getattr(sr, name)(*c) == w, (name, c)
        out[name] = want
    return out


def _check_middle(ref, orc, cases, second_every=0):
    want = ref.find_middle(cases)
    for i, (c, w) in enumerate(zip(cases, want)):
        got = orc.find_middle(*c)
        assert got[0] == w[0] and (not w[0] or got[1:] == w[1:]), (c, got, w)
        if second_every and i % second_every == 0:
            s = sr.find_middle(*c)
            assert s[0] == w[0] and (not w[0] or tuple(s[1:]) == w[1:]), (c, s, w)
    return want


@pytest.mark.parametrize("seed", range(3))
def test_seeded_cases_vs_reference(ref, orc, seed):
    """the generators of tests/test_second_reading.py: default and window modes, both end trims, findMiddleAdapters"""
    rng = np.random.default_rng(8000 + seed)
    search, trims, middle = [], [], []
    for _ in range(1500):
        sa, ea = ac.adapter(rng), ac.adapter(rng)
        if rng.random() < 0.2 and sa:
            ea = synth.revcomp(sa.decode()).encode()
        seq = ac.read_with(rng, sa if rng.random() < 0.5 else ea)
        ed, ext = float(rng.choice(ED_MAX)), int(rng.choice([0, 0, 5, 10, 30, 500]))
        start = int(rng.choice([0, 0, max(0, len(seq) - 200), int(rng.integers(0, len(seq) + 5))]))
        length = int(rng.choice([-1, 0, 200, int(rng.integers(1, 400))]))
        for l, r in MODES:
            search.append((seq, sa, ed, start, length, l, r))
        search.append((seq, ea, ed, 0, -1, False, False))
        trims.append((seq, sa, ed, ext))
        middle.append((seq, sa, ea, ed, ext))
    hits = _check_search(ref, orc, search, second_every=23)
    assert sum(h >= 0 for h in hits) > 1000
    t = _check_trims(ref, orc, trims, second_every=37)
    assert sum(w[2] > 0 for w in t["trim_start"]) > 100 and sum(0 < w[2] < len(c[1]) for w, c in zip(t["trim_end"], trims)) > 10
    m = _check_middle(ref, orc, middle, second_every=29)
    assert sum(w[0] for w in m) > 300


def test_every_adapter_length_around_the_read_length(ref, orc):
    """adapter lengths 1-70 (random, homopolymer, period 2 and 3) against reads of alen-1 ... alen+2 bases that hold
    nothing, an exact copy at 0, an exact copy at the last position or a one-mismatch copy in the middle"""
    rng = np.random.default_rng(8100)
    search, trims = [], []
    for alen in range(1, 71):
        ads = [ac.rnd(rng, alen), ac.rnd(rng, 1) * alen, (ac.rnd(rng, 2) * alen)[:alen], (ac.rnd(rng, 3) * alen)[:alen]]
        for ad in ads:
            for rlen in range(max(0, alen - 1), alen + 3):
                bg = ac.rnd(rng, rlen)
                reads = [bg]
                if rlen >= alen:
                    reads += [ad + bg[alen:], bg[:rlen - alen] + ad, bg[:(rlen - alen) // 2] + _subst(rng, ad, 1)
                              + bg[(rlen - alen) // 2 + alen:]]
                for seq in reads:
                    assert len(seq) == rlen
                    for ed in (0.0, 0.3, 1.0):
                        for l, r in MODES:
                            search.append((seq, ad, ed, 0, -1, l, r))
                    trims.append((seq, ad, 0.3, 10))
                    trims.append((seq, ad, 0.0, 0))
    hits = _check_search(ref, orc, search, second_every=41)
    assert sum(h >= 0 for h in hits) > 5000
    _check_trims(ref, orc, trims, second_every=53)


def test_copies_at_exactly_the_threshold(ref, orc):
    """a copy with exactly thr = round(ed_max * alen) substitutions is found, one with thr + 1 is not (unless the background
    matches better): planted at 0, in the middle, at p = rlen - alen - 1 (the last window the default mode visits) and at
    p = rlen - alen"""
    rng = np.random.default_rng(8200)
    search, trims, meta = [], [], []
    for alen in (4, 5, 7, 8, 12, 15, 16, 17, 24, 29, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 70):
        for ed in (0.1, 0.2, 0.25, 0.3, 0.4, 0.5):
            thr = sr.c_round(ed * alen)
            if thr + 1 > alen:
                continue
            ad = ac.rnd(rng, alen)
            for extra in (0, 1):
                for rlen in (alen + 1, alen + 2, alen + 40, 200 + alen):
                    for where in ("first", "middle", "second_last", "last"):
                        at = {"first": 0, "middle": (rlen - alen) // 2, "second_last": rlen - alen - 1, "last": rlen - alen}[where]
                        bg = bytearray(ac.rnd(rng, rlen))
                        bg[at:at + alen] = _subst(rng, ad, thr + extra)
                        seq = bytes(bg)
                        for l, r in MODES:
                            search.append((seq, ad, ed, 0, -1, l, r))
                            meta.append((extra, where, l, r))
                        search.append((seq, ad, ed, max(0, rlen - 200), 200, True, False))  # as trimBySequenceEnd asks
                        search.append((seq, ad, ed, 0, 200, False, True))  # as trimBySequenceStart asks
                        meta += [(extra, where, None, None)] * 2
                        trims.append((seq, ad, ed, 10))
    want = _check_search(ref, orc, search, second_every=17)
    # a copy with exactly thr mismatches is found by the default mode anywhere but at the last position (a window with at
    # most thr mismatches has an edit distance of at most thr, so the first strict minimum always passes), and by the
    # right-to-left mode everywhere; at the last position the default mode finds only what the background holds
    default_at_thr = [w for w, m in zip(want, meta) if m == (0, m[1], False, False) and m[1] != "last"]
    right_at_thr = [w for w, m in zip(want, meta) if m[0] == 0 and m[2:] == (False, True)]
    assert len(default_at_thr) > 300 and all(w >= 0 for w in default_at_thr)
    assert len(right_at_thr) > 400 and all(w >= 0 for w in right_at_thr)
    _check_trims(ref, orc, trims, second_every=19)


def test_best_window_at_the_last_position(ref, orc):
    """an exact copy at p = rlen - alen over a background that matches nowhere: the default mode's loop stops at
    p < rlen - alen, so the reference does not return it; the window modes (asRightAsPossible visits it) do"""
    rng = np.random.default_rng(8300)
    cases = []
    for alen in list(range(4, 71)) + [100, 250]:
        ad = ac.rnd(rng, alen)
        for extra in (1, 2, 5, 33, 200):
            seq = ac.rnd(rng, extra) + ad
            for ed in (0.0, 0.3):
                cases.append((seq, ad, ed, 0, -1, False, False))
                cases.append((seq, ad, ed, 0, -1, False, True))
    want = _check_search(ref, orc, cases, second_every=7)
    for c, w in zip(cases, want):
        last = len(c[0]) - len(c[1])
        if c[6]:
            assert w == last, c
        else:
            assert w != last, c


def test_equal_hamming_windows_first_fails_the_edit_distance(ref, orc):
    """two windows with the same (minimum) mismatch count: the first one differs by substitutions (edit distance > thr),
    the later one by an indel (edit distance <= thr).  The default mode confirms only the first strict minimum, so the
    reference answers -1 where a later window would have passed"""
    rng = np.random.default_rng(8400)
    cases = []
    for alen in (16, 20, 24, 31, 32, 33, 40, 48, 63, 64, 65, 70):
        for _ in range(12):
            ad = ac.rnd(rng, alen)
            i = int(rng.integers(2, alen // 2))
            j = i + int(rng.integers(4, 9))
            # one deletion at i and one insertion after j: edit distance <= 2, the bases between shifted by one
            w2 = ad[:i] + ad[i + 1:j + 1] + b"ACGT"[int(rng.integers(4))].to_bytes(1, "big") + ad[j + 1:]
            h = int(sr.window_mismatches(w2, ad)[0])
            if h < 3:
                continue
            w1 = _subst(rng, ad, h)
            ed = 2.4 / alen  # thr = 2
            seq = ac.rnd(rng, 7) + w1 + ac.rnd(rng, int(rng.integers(0, 20))) + w2 + ac.rnd(rng, 5)
            mm = sr.window_mismatches(seq, ad)[:len(seq) - alen]
            if mm.min() != h or sr.levenshtein(w1, ad) <= 2:
                continue
            cases.append((seq, ad, ed, 0, -1, False, False))
            cases.append((seq, ad, ed, 0, -1, True, False))
    assert len(cases) > 100
    want = _check_search(ref, orc, cases, second_every=3)
    assert sum(w == -1 for c, w in zip(cases, want) if not c[5]) > 40


def test_ed_max_on_the_rounding_half(ref, orc):
    """ed_max * alen landing on k + .5 (round() rounds half away from zero), and ed_max 0 and 1, with copies of k, k + 1 and
    k + 2 mismatches"""
    rng = np.random.default_rng(8500)
    cases, trims = [], []
    for alen in range(1, 71):
        ad = ac.rnd(rng, alen)
        eds = [0.0, 1.0] + [(k + 0.5) / alen for k in range(0, alen, max(1, alen // 12))]
        for ed in eds:
            k = int(ed * alen)
            for m in (k, k + 1, k + 2):
                if m > alen:
                    continue
                seq = ac.rnd(rng, 9) + _subst(rng, ad, m) + ac.rnd(rng, 9)
                for l, r in ((False, False), (True, False), (False, True)):
                    cases.append((seq, ad, ed, 0, -1, l, r))
                trims.append((seq, ad, ed, 0))
    _check_search(ref, orc, cases, second_every=11)
    _check_trims(ref, orc, trims, second_every=13)


def test_trim_by_multi_sequences_is_the_end_trims_in_turn(ref, orc):
    """trimByMultiSequences (-a): for each adapter in list order, trimBySequenceStart then trimBySequenceEnd on what is left"""
    rng = np.random.default_rng(8600)
    cases = []
    for _ in range(400):
        ads = [a for a in (ac.adapter(rng) for _ in range(int(rng.integers(1, 20)))) if a]
        seq = ac.read_with(rng, ads[0] if ads else b"", rlen_max=600)
        for a in ads[1:4]:
            if rng.random() < 0.5 and len(seq) > 40:
                at = int(rng.integers(0, len(seq)))
                seq = seq[:at] + ac.mutated(rng, a, 0.05) + seq[at:]
        cases.append((seq, ads, float(rng.choice(ED_MAX)), int(rng.choice([0, 10, 30]))))
    want = ref.trim_multi(cases)
    trimmed = 0
    for (seq, ads, ed, ext), w in zip(cases, want):
        s, total = seq, 0
        for a in ads:
            for f in (orc.trim_start, orc.trim_end):
                left, t, _ = f(s, a, ed, ext)
                s, total = left.encode("latin-1"), total + t
        assert (s, total) == w, (seq, ads, ed, ext)
        trimmed += total > 0
    assert trimmed > 100


def test_reverse_complement_every_byte_every_length(ref):
    """Sequence::reverseComplement on all 256 byte values at lengths 0-70 (the stand-in's full-vector path from 16 bytes on
    and its tail path) against the Python restatement the tests build their configurations with (fastplong_amd.synth.revcomp).
    The CLI's own derivation of -e from -s (host/cli.cpp) is compared with the reference program's in
    tests/test_cli_vs_ref_binary_stub.py::test_end_adapter_derived_from_start_adapter."""
    seqs = [b""]
    for n in range(1, 71):
        for j in range((256 + n - 1) // n):
            seqs.append(bytes((j * n + i * 37 + n) % 256 for i in range(n)))
        seqs.append(bytes(range(256))[:n])
    seen = set()
    for s in seqs:
        seen.update(s)
    assert len(seen) == 256
    want = ref.reverse_complement(seqs)
    for s, w in zip(seqs, want):
        assert len(w) == len(s)
        assert w == synth.revcomp(s.decode("latin-1")).encode("latin-1"), s
