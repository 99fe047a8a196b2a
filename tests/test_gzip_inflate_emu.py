"""The four kernels of the single-member inflate (fastplong_amd/csrc/gzip_inflate.h) and the fold behind them, compiled for the
emulator under AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu_gzip), against zlib.  Every buffer the kernels see is a
heap block of exactly its size, so the bounds a decode of garbage has to keep are checked, not trusted: a run that leaves one ends
with a report and the test fails.  The streams and the rules are tests/gzip_cases.py, shared with the device test."""
import os
import zlib

import pytest

from tests import gzip_cases as gc
from tests.emu_gzip import build as emu

PARTS = max(1, min(16, os.cpu_count() or 1))


def batch_call(jobs):
    """the jobs of one round, in PARTS sanitized processes side by side"""
    started = [(k, emu.start(jobs[k::PARTS])) for k in range(PARTS) if jobs[k::PARTS]]
    res = [None] * len(jobs)
    for k, job in started:
        res[k::PARTS] = emu.finish(job)
    return res


@pytest.fixture(scope="module", autouse=True)
def built():
    emu.build()


def test_the_streams_hold_what_their_names_say():
    seen = set()
    for c in gc.zlib_cases():
        if c.comp in seen:
            continue
        seen.add(c.comp)
        d = gc.describe(c.comp)
        assert d["out"] == len(c.data) and d["end_bit"] + 7 >> 3 == len(c.comp), c.name
        for k, v in c.must.items():
            assert d[k] == v if k in ("max_dist", "last_block_bits") else d[k] >= v, (c.name, k, d)
    sizes = sorted(len(c.data) for c in gc.zlib_cases())
    assert sizes[0] == 0 and 1 in sizes and 70000 in sizes
    for c in gc.zlib_cases():  # several windows pass dictionaries along, several chunks in each
        if len(c.data) > 70000:
            assert len(c.comp) > 2 * c.window or "run" in c.name, c.name
    emb = gc.doubt_cases()[0]
    d = gc.describe(emb.comp)
    assert d["dynamic"] == 0 and d["stored"] > 10 and emb.whole


def test_zlib_writes_these():
    runs = gc.run_members(gc.zlib_cases(), batch_call)
    gc.check_zlib_list(runs)
    for r in runs:
        if len(r.case.data) > 70000 and "run" not in r.case.name:
            assert len(r.windows) >= 3, (r.case.name, len(r.windows))
        if r.case.name.startswith(("level", "spliced", "far_matches", "sync_flush")):  # the chain went through guessed starts
            assert max(w["chunks"] for w in r.windows) >= 2, r.case.name


@pytest.fixture(scope="module")
def doubt_runs(built):
    """list (b) through its windows, once for the tests that look at it"""
    return gc.run_members(gc.doubt_cases(), batch_call)


@pytest.fixture(scope="module")
def stream_res(built):
    """the hand-made and the refused streams of the BGZF tests, one window each"""
    return batch_call(gc.stream_jobs())


def test_must_not_be_believed(doubt_runs):
    runs = doubt_runs
    gc.check_doubt_list(runs)
    by = {r.case.name: r for r in runs}
    for ch in gc.CHUNKS:
        r = by["right_dict/c%d" % ch]
        assert r.final and r.refused == 0 and r.out == r.case.data
        e = by["embedded_stream/c%d" % ch]  # correct or refused: never the inner stream's text for the stored bytes
        assert e.refused or (e.final and e.out == e.case.data)
        assert not by["out_cap_short/c%d" % ch].final
    assert all(not r.final for r in runs if r.case.name.startswith("cut/"))


def test_recorded_window_results_are_this_run_s(doubt_runs, stream_res):
    """tests/golden/gzip_window_results.json: every window's rc, status, byte count, end bit, CRC-32, final flag and chunk count, of
    list (b) and of the BGZF tests' hand-made and refused streams.  A check that moved inside the decoder shows here."""
    gc.check_doubt_record(doubt_runs)
    gc.check_stream_record(stream_res)


def test_the_two_decoders_differ_where_they_must_and_nowhere_else(stream_res):
    """the same streams through this decoder and through k_bgzf_inflate (tests/emu_bgzf): the single 1-bit distance code, the
    distance that reaches before the output's start, and the hand-made streams both take"""
    from tests import bgzf_cases as bc
    from tests.emu_bgzf import build as emu_bgzf

    emu_bgzf.build()
    cases = gc.stream_cases()
    gc.check_stream_rules(stream_res)
    comp, blocks, out = bc.pack(cases, 12)
    got, done = emu_bgzf.inflate(comp, blocks, out)
    bc.check(cases, blocks, got, done["status"])  # (a status 0 there means zlib's bytes: the same as this decoder's)
    st = {c.name: int(s) for c, s in zip(cases, done["status"])}
    assert st["refuse/single_distance_code"] == 1 and st["refuse/distance_before_start"] == 1  # FPL_BGZF_MALFORMED
    assert all(s == 0 for n, s in st.items() if n.startswith("hand/"))


def test_eight_megabytes_at_the_default_sizes():
    c = gc.big_case()
    (r,) = gc.run_members([c], batch_call)
    gc.check_zlib_list([r])
    assert sum(w["chunks"] for w in r.windows) > 20


def test_arguments_are_refused():
    comp = gc.raw(b"hello hello hello")
    bad = [dict(comp=comp, out_cap=100, chunk_bytes=63), dict(comp=comp, out_cap=100, chunk_bytes=(1 << 24) + 1),
           dict(comp=comp, out_cap=100, start_bit=8 * len(comp)), dict(comp=b"", out_cap=100)]
    assert [r["rc"] for r in emu.inflate(bad)] == [-1] * len(bad)
    (ok,) = emu.inflate([dict(comp=comp, out_cap=100)])
    assert ok["rc"] == 0 and ok["status"] == 0 and ok["final"] and ok["data"] == b"hello hello hello" and ok["crc32"] == zlib.crc32(ok["data"])
