"""--keep_mods on the host (README "BAM output"): the shared rule (fastplong_amd/csrc/bam_mod_rules.h) in the host form
(host/bam_tags.cpp, host/bam_out.cpp), through its test hook, against the two plain-Python pieces of tests/bam_mod_cases.py: the
byte rule, byte for byte, for --out and --failed_out, the decoder's semantic property on every re-indexed record, the counters."""
import ctypes as C

import numpy as np
import pytest

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.gzcheck import load_hostlib

FORM_ARGS = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
             C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    lib = load_hostlib()
    lib.fplh_bam_tag_form.restype = lib.fplh_bam_mod_form.restype = C.c_int
    lib.fplh_bam_tag_form.argtypes = FORM_ARGS
    lib.fplh_bam_mod_form.argtypes = FORM_ARGS + [C.POINTER(C.c_uint64)]
    return lib


@pytest.fixture(scope="module")
def cases():
    recs, res, _ = mc.case_list()
    return recs, res, mc.expected(recs, res)


def host_form(L, tmp_path, recs, res, threads, mods=True, frags=None):
    """-> (--out records, --failed_out records, tag stats of each, mod stats of each)"""
    data = tc.input_bam(recs, block=20000)
    p = tmp_path / "in.bam"
    p.write_bytes(data)
    seq, qual, off, _ = bamio.twin_csr(data)
    res = np.ascontiguousarray(res)
    assert len(off) - 1 == len(res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    stats, ms = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    seq, qual = np.ascontiguousarray(seq), np.ascontiguousarray(qual)
    regs = np.zeros(0, np.dtype(abi.REGION_DTYPE))
    fr, nf = (None, 0xFFFFFFFF) if frags is None else (frags.ctypes.data, len(frags))
    args = [str(p).encode(), seq.ctypes.data, qual.ctypes.data, res.ctypes.data, len(res), fr, nf, regs.ctypes.data if nf != 0xFFFFFFFF else None, 0,
            threads, C.byref(out), C.byref(n), C.byref(fo), C.byref(fn), stats]
    assert (L.fplh_bam_mod_form(*args, ms) if mods else L.fplh_bam_tag_form(*args)) == 0
    got = C.string_at(out, n.value), C.string_at(fo, fn.value), list(stats[:4]), list(stats[4:]), list(ms[:4]), list(ms[4:])
    L.fplh_free(out), L.fplh_free(fo)
    return got


@pytest.mark.parametrize("threads", [1, 5])
def test_host_form_equals_the_byte_rule_on_the_case_list(L, tmp_path, cases, threads):
    recs, res, want = cases
    got = host_form(L, tmp_path, recs, res, threads)
    assert got[4:] == (want[4], want[5]) and got[2:4] == (want[2], want[3])
    assert got[0] == want[0] and got[1] == want[1]


def test_the_decoder_reads_the_same_calls_out_of_every_re_indexed_record(L, tmp_path, cases):
    """(b): the host's bytes equal the model's (the test above), and here the model's bytes of every re-indexed record decode to the
    input's calls inside the fragment; the host's records are cut apart again and their regions compared one by one"""
    recs, res, want = cases
    got = host_form(L, tmp_path, recs, res, 3)
    regions, raw = [], got[0] + got[1]
    while raw:
        n = 4 + int.from_bytes(raw[:4], "little")
        regions.append(tc.aux_region(raw[:n]))
        raw = raw[n:]
    assert not raw
    calls = 0
    for name, region, codes, s, n, t in want[6]:
        assert t in regions, name
        calls += mc.check_semantics(region, codes, s, n, t)
    assert calls > 10000 and len(want[6]) == want[4][0] + want[5][0]


def test_a_failed_read_trimmed_to_nothing_keeps_its_headers_and_no_position(L, tmp_path):
    rng = np.random.default_rng(3)
    codes = rng.choice(np.array([1, 2, 4, 8], np.uint8), 40).tobytes()
    tags = mc.fields_of(codes, [(b"C+mh?", mc.every(codes, b"C", 1)), (b"N+n", [0, 5])], rng)
    rec = (b"gone", 0x4, codes, bytes([20]) * 40, bamio.encode_record(b"gone", 0x4, codes, bytes([20]) * 40, tags=tags))
    r = tc.result_of("fails", 40)
    r["r1_start"], r["r1_len"] = 17, 0
    r["frag_start"][0], r["frag_len"][0] = 17, 0
    res = np.array([r], np.dtype(abi.RESULT_DTYPE))
    want = mc.expected([rec], res)
    got = host_form(L, tmp_path, [rec], res, 1)
    assert got[1] == want[1] and got[0] == b"" and got[5] == want[5] == [1, 0, 0, len(mc.every(codes, b"C", 1)) + 2]
    region = tc.aux_region(got[1])
    assert b"MMZC+mh?;N+n;\0" in region and b"MLBC\0\0\0\0" in region and tc.scalar(b"MN", b"i", 0) in region
    mc.check_semantics(tags, codes, 17, 0, region)


def test_regions_that_do_not_parse_behind_the_mm_go_the_old_way(L, tmp_path):
    recs, res = mc.malformed_list()
    want, old = mc.expected(recs, res), tc.expected(recs, res)
    got = host_form(L, tmp_path, recs, res, 2)
    assert got[:2] == want[:2] == old[:2] and got[2:4] == (old[2], old[3])
    assert got[4] == want[4] == [0, 3, 0, 0] and got[5] == want[5] == [0, 1, 0, 0]


def test_switch_off_is_the_tagged_form_and_break_mask_runs_re_index_nothing(L, tmp_path, cases):
    recs, res, want = cases
    old = tc.expected(recs, res)
    got = host_form(L, tmp_path, recs, res, 3, mods=False)
    assert got[:4] == (old[0], old[1], old[2], old[3]) and got[4:] == ([0] * 4, [0] * 4)
    assert got[0] != want[0] and got[1] != want[1]
    # a --break / --mask run with the switch on: every record changed, none re-indexable, the ones with the fields counted
    sub = [r for r in recs[:150]]
    sres = res[:len(sub)].copy()
    frags = []
    for i, (r, rec) in enumerate(zip(sres, sub)):
        r["n_frag"], r["frag_start"], r["frag_len"] = 255, 0, 0
        if r["dropped"]:
            continue
        code = abi.FPL_PASS_FILTER if i % 3 else abi.FPL_FAIL_QUALITY
        frags.append((i, 0, int(r["r1_start"]), int(r["r1_len"]), 0, 0, 0, code, 0, 30, (0, 0, 0)))
    frags = np.array(frags, np.dtype(abi.FRAGMENT_DTYPE))
    old = tc.expected(sub, sres, fragment_mode=True, frags=frags)
    got = host_form(L, tmp_path, sub, sres, 2, frags=frags)
    assert got[:4] == (old[0], old[1], old[2], old[3])
    n_out, n_failed = len(frags[frags["code"] == abi.FPL_PASS_FILTER]), len(frags[frags["code"] != abi.FPL_PASS_FILTER])
    assert got[4] == [0, n_out, 0, 0] and got[5] == [0, n_failed, 0, 0] and n_out > 50 and n_failed > 20  # (all of them carry the fields)
