"""--keep_moves on the host (README "BAM output"): the shared rule (fastplong_amd/csrc/bam_move_rules.h) in the host form
(host/bam_tags.cpp, host/bam_out.cpp), through its test hook, against the plain-Python pieces of tests/bam_move_cases.py: the byte
rule, byte for byte, for --out and --failed_out, the decoder's semantic property on every re-indexed record, the counters; the
switch crossed with --keep_mods; with the switch off, the bytes of the forms before it."""
import ctypes as C

import numpy as np
import pytest

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_move_cases as vc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.gzcheck import load_hostlib
from tests.test_host_bam_mods import FORM_ARGS


@pytest.fixture(scope="module")
def L():
    lib = load_hostlib()
    lib.fplh_bam_move_form.restype = C.c_int
    lib.fplh_bam_move_form.argtypes = FORM_ARGS + [C.c_int, C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64)]
    return lib


@pytest.fixture(scope="module")
def cases():
    recs, res, _ = vc.case_list()
    return recs, res, vc.expected(recs, res)


def host_form(L, tmp_path, recs, res, threads, mods=False, moves=True, frags=None):
    """-> (--out records, --failed_out records, tag stats of each, mod stats of each, move stats of each)"""
    data = tc.input_bam(recs, block=20000)
    p = tmp_path / "in.bam"
    p.write_bytes(data)
    seq, qual, off, _ = bamio.twin_csr(data)
    res = np.ascontiguousarray(res)
    assert len(off) - 1 == len(res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    stats, ms, vs = (C.c_uint64 * 8)(), (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    seq, qual = np.ascontiguousarray(seq), np.ascontiguousarray(qual)
    regs = np.zeros(0, np.dtype(abi.REGION_DTYPE))
    fr, nf = (None, 0xFFFFFFFF) if frags is None else (frags.ctypes.data, len(frags))
    args = [str(p).encode(), seq.ctypes.data, qual.ctypes.data, res.ctypes.data, len(res), fr, nf, regs.ctypes.data if nf != 0xFFFFFFFF else None, 0,
            threads, C.byref(out), C.byref(n), C.byref(fo), C.byref(fn), stats]
    assert L.fplh_bam_move_form(*args, int(mods), ms, int(moves), vs) == 0
    got = (C.string_at(out, n.value), C.string_at(fo, fn.value), list(stats[:4]), list(stats[4:]), list(ms[:4]), list(ms[4:]), list(vs[:4]),
           list(vs[4:]))
    L.fplh_free(out), L.fplh_free(fo)
    return got


def regions_of(raw):
    """the aux regions of a stream of records"""
    out = []
    while raw:
        n = 4 + int.from_bytes(raw[:4], "little")
        out.append(tc.aux_region(raw[:n]))
        raw = raw[n:]
    return out


@pytest.mark.parametrize("threads", [1, 5])
def test_host_form_equals_the_byte_rule_on_the_case_list(L, tmp_path, cases, threads):
    recs, res, want = cases
    got = host_form(L, tmp_path, recs, res, threads)
    assert got[2:] == tuple(want[2:8])
    assert got[0] == want[0] and got[1] == want[1]


def test_the_decoder_finds_every_base_where_it_was(L, tmp_path, cases):
    """(b): the host's bytes equal the model's (the test above); here every re-indexed record of the host's is looked up among the
    model's and decoded: base j of the record has the samples of base s + j of its read"""
    recs, res, want = cases
    got = host_form(L, tmp_path, recs, res, 3)
    regions = set(regions_of(got[0] + got[1]))
    bases = 0
    for name, region, s, n, t in want[8]:
        assert t in regions, name
        bases += vc.check_semantics(region, s, n, t)
    assert bases > 20000 and len(want[8]) == want[6][0] + want[7][0] >= 40


@pytest.mark.parametrize("mods", [False, True])
@pytest.mark.parametrize("moves", [False, True])
def test_the_two_switches_cross(L, tmp_path, cases, mods, moves):
    """each switch decides its own fields: all four combinations against the composed rule, on this list and on --keep_mods' own"""
    recs, res, _ = cases
    more, mres, _ = mc.case_list()
    keep = [i for i, r in enumerate(more) if len(r[2]) <= 1030]
    recs, res = recs + [more[i] for i in keep], np.concatenate([res, mres[keep]])
    want = vc.expected(recs, res, mods=mods, moves=moves)
    got = host_form(L, tmp_path, recs, res, 4, mods=mods, moves=moves)
    assert got[2:] == tuple(want[2:8])
    assert got[0] == want[0] and got[1] == want[1]
    assert (want[4][0] > 40) == mods and (want[6][0] > 40) == moves
    if mods and not moves:  # today's --keep_mods
        old = mc.expected(recs, res)
        assert got[:6] == (old[0], old[1], old[2], old[3], old[4], old[5])
    if not mods and not moves:  # today's --keep_tags
        old = tc.expected(recs, res)
        assert got[:4] == (old[0], old[1], old[2], old[3]) and got[4:] == ([0] * 4,) * 4
    if mods and moves:  # a record with both kinds of fields and no other array keeps every field
        both = [i for i, r in enumerate(recs) if r[0].startswith(b"both.77.") or r[0].startswith(b"both.and_another_array.77.")]
        w = vc.expected([recs[i] for i in both], res[both], mods=True)
        assert w[2][0] >= 4 and w[2][1] >= 4 and w[4][1] == w[6][1] == 0


def test_regions_that_do_not_parse_behind_the_table(L, tmp_path):
    """the parsed prefix holds one mv and no ts: re-indexable by itself, and the ts behind the break is not written at all"""
    recs, res = vc.malformed_list()
    more, mres = mc.malformed_list()
    recs, res = recs + more, np.concatenate([res, mres])
    want = vc.expected(recs, res, mods=True)
    got = host_form(L, tmp_path, recs, res, 2, mods=True)
    assert got[:2] == want[:2] and got[2:] == tuple(want[2:8])
    assert want[6] == [3, 0, want[6][2], want[6][3]] and want[7][0] == 1 and want[2][3] == 8 and b"ts" not in got[0]


def test_break_and_mask_runs_re_index_nothing(L, tmp_path, cases):
    recs, res, want = cases
    sub = recs[:150]
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
    assert got[6] == [0, n_out, 0, 0] and got[7] == [0, n_failed, 0, 0] and n_out > 50 and n_failed > 20  # (all of them carry a table)
