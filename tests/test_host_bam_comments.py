"""--comment_tags on the host (README "Tags as FASTQ comments"): the shared rule (fastplong_amd/csrc/bam_comment_rules.h) in the host
form (host/bam_comments.cpp) through its test hook, against the plain-Python model of tests/bam_comment_cases.py, byte for byte, for
--out and --failed_out, every selection and every plan; the counters; and a property check against code the project already
trusts: the tags of the records fastq_to_bam_records makes with tags and mods on, formatted, are the same comments."""
import ctypes as C

import numpy as np
import pytest

from fastplong_amd import abi
from tests import bam_comment_cases as cc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.gzcheck import load_hostlib
from tests.test_host_bam_mods import FORM_ARGS

COMMENT_ARGS = FORM_ARGS[:10] + [C.c_char_p, C.c_int] + FORM_ARGS[10:]


@pytest.fixture(scope="module")
def L():
    lib = load_hostlib()
    lib.fplh_bam_comment_form.restype = lib.fplh_bam_mod_form.restype = lib.fplh_bam_comment_text.restype = lib.fplh_comment_tag_list.restype = C.c_int
    lib.fplh_bam_comment_form.argtypes = COMMENT_ARGS
    lib.fplh_bam_mod_form.argtypes = FORM_ARGS + [C.POINTER(C.c_uint64)]
    lib.fplh_bam_comment_text.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fplh_comment_tag_list.argtypes = [C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """the case list, its input file and what the reader makes of it, once"""
    recs, res = cc.case_list()
    data = tc.input_bam(recs, block=20000)
    p = tmp_path_factory.mktemp("comments") / "in.bam"
    p.write_bytes(data)
    seq, qual, off, _ = bamio.twin_csr(data)
    assert len(off) - 1 == len(res)
    return recs, res, p, np.ascontiguousarray(seq), np.ascontiguousarray(qual)


def host_form(L, case, sel, threads, frags=None, res=None, mod_form=False):
    """-> (--out text, --failed_out text, the four counts of each); mod_form: the BAM records of --keep_tags --keep_mods instead"""
    recs, res0, p, seq, qual = case
    res = np.ascontiguousarray(res0 if res is None else res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    stats, ms = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    regs = np.zeros(0, np.dtype(abi.REGION_DTYPE))
    fr, nf = (None, 0xFFFFFFFF) if frags is None else (frags.ctypes.data, len(frags))
    head = [str(p).encode(), seq.ctypes.data, qual.ctypes.data, res.ctypes.data, len(res), fr, nf, regs.ctypes.data if nf != 0xFFFFFFFF else None, 0, threads]
    tail = [C.byref(out), C.byref(n), C.byref(fo), C.byref(fn), stats]
    if mod_form:
        assert L.fplh_bam_mod_form(*head, *tail, ms) == 0
    else:
        assert L.fplh_bam_comment_form(*head, *cc.selection_args(sel), *tail) == 0
    got = C.string_at(out, n.value), C.string_at(fo, fn.value), list(stats[:4]), list(stats[4:])
    L.fplh_free(out), L.fplh_free(fo)
    return got


def rule_text(L, tag_bytes, sel):
    out, n, counts = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 3)()
    assert L.fplh_bam_comment_text(tag_bytes, len(tag_bytes), *cc.selection_args(sel), C.byref(out), C.byref(n), counts) == 0
    got = C.string_at(out, n.value)
    L.fplh_free(out)
    return got, list(counts)


@pytest.mark.parametrize("name", sorted(cc.SELECTIONS))
def test_host_form_equals_the_model_for_every_plan(L, cases, name):
    """whole, front, tail, split, failed and dropped reads all occur in the list (tc.PLANS rotate through it)"""
    sel = cc.SELECTIONS[name]
    want = cc.expected(cases[0], cases[1], sel)
    got = host_form(L, cases, sel, 1 if name == "first" else 5)
    assert got[2:] == (want[2], want[3])
    assert got[0] == want[0] and got[1] == want[1]
    if name == "all":
        assert want[2][0] > 300 and want[3][0] > 50 and want[2][3] >= 4 and want[2][2] > 200000
        assert b"split-by-adapter-right-" in want[0] and b" failed_too_short\t" in want[1] and b"\tMM:Z:" in want[1]
        assert max(len(l) for l in want[0].split(b"\n")) > 49152 + 16384  # (the long ML's comment)
    if name == "nothing":
        assert got[2] == got[3] == [0, 0, 0, 0] and b"\t" not in got[0]


def test_switch_off_is_the_formatter_s_text(L, cases):
    off = host_form(L, cases, None, 3)
    nothing = host_form(L, cases, cc.SELECTIONS["nothing"], 3)
    assert off == nothing and off[2] == [0] * 4
    # ... which is the text the records of the no-tag rule are made from
    assert bc.records(off[0]) == bc.records(cc.expected(cases[0], cases[1], None)[0])
    assert off[0] == cc.expected(cases[0], cases[1], None)[0] and off[1] == cc.expected(cases[0], cases[1], None)[1]


def test_the_issue_s_examples_and_the_left_out_fields(L):
    for v, text in cc.FLOAT_EXAMPLES:
        assert rule_text(L, tc.scalar(b"xf", b"f", v), "*") == (b"\txf:f:" + text, [1, 6 + len(text), 0])
    assert rule_text(L, cc.ffield(b"xf", 0xFFC00000), "*")[0] == b"\txf:f:-nan"
    assert rule_text(L, cc.REGIONS["z_tab"], "*") == (b"\tqs:f:17.25\tch:i:407", [2, 20, 1])
    got = rule_text(L, cc.REGIONS["z_del_and_a_ctl"], "*")
    assert got == (b"\tok:A:~", [1, 7, 3])
    assert rule_text(L, cc.REGIONS["integers"], "*")[0] == cc.comment(cc.REGIONS["integers"], "*")[0]
    assert b"\tl4:i:-2147483648" in cc.comment(cc.REGIONS["integers"], "*")[0] and b"\th1:i:4294967295" in cc.comment(cc.REGIONS["integers"], "*")[0]
    assert rule_text(L, tc.barray(b"xb", b"C", []), [b"xb"])[0] == b"\txb:B:C"
    assert rule_text(L, tc.P1 + tc.zfield(b"Mm", b"C+m;"), [b"MM"])[0] == b"\tMM:Z:C+m,5,12,0;"  # (MM is not Mm)


def test_the_5x_bound_holds_for_every_record_of_the_list(L, cases):
    assert cc.bound_holds(cases[0])
    # ... and for the worst field there is
    worst = tc.barray(b"wc", b"c", [-128] * 1000)
    text = rule_text(L, worst, "*")[0]
    assert len(text) == 7 + 5 * 1000 <= 5 * len(worst)


def test_the_tags_of_the_bam_records_give_the_same_comments(L, cases):
    """the property: what --keep_tags --keep_mods puts into a record, formatted by the rule, is the record's comment"""
    bam = host_form(L, cases, None, 4, mod_form=True)
    fq = host_form(L, cases, "*", 4)
    n = 0
    for records, text in zip(bam[:2], fq[:2]):
        lines = [r[0] for r in bc.fastq_records(text)]
        at = 0
        for line in lines:
            size = 4 + int.from_bytes(records[at:at + 4], "little")
            tags = tc.aux_region(records[at:at + size])
            at += size
            c, _ = rule_text(L, tags, "*")
            assert line.endswith(c) and c == cc.comment(tags, "*")[0]
            assert len(c) <= 5 * len(tags)
            n += bool(c)
        assert at == len(records)
    assert n > 400


def test_a_break_mask_run_re_indexes_nothing(L, cases):
    res = cases[1][:150].copy()
    frags = []
    for i, r in enumerate(res):
        r["n_frag"], r["frag_start"], r["frag_len"] = 255, 0, 0
        if r["dropped"]:
            continue
        code = abi.FPL_PASS_FILTER if i % 3 else abi.FPL_FAIL_QUALITY
        frags.append((i, 0, int(r["r1_start"]), int(r["r1_len"]), 0, 0, 0, code, 0, 30, (0, 0, 0)))
    frags = np.array(frags, np.dtype(abi.FRAGMENT_DTYPE))
    # (the hook reads the whole file: the results behind the first 150 are dropped reads)
    full = cases[1].copy()
    full[:150] = res
    full[150:]["dropped"], full[150:]["n_frag"] = 1, 0
    want = cc.expected(cases[0], full, "*", fragment_mode=True, frags=frags)
    got = host_form(L, cases, "*", 2, frags=frags, res=full)
    assert got == want
    assert b"\tMM:Z:" not in got[0] and b"\tML:B:" not in got[1] and b"\tRG:Z:run7_grp" in got[0] and got[2][0] > 50 and got[3][0] > 20


def test_the_cli_s_reading_of_a_list(L):
    assert L.fplh_comment_tag_list(b"*") == -1 and L.fplh_comment_tag_list(b"MM,ML") == 2 and L.fplh_comment_tag_list(b"x9") == 1
    assert L.fplh_comment_tag_list(b",".join(cc.TAGS_32)) == 32
    for bad in (b"", b"M", b"MM,", b",MM", b"MM,,ML", b"MML", b"9M", b"M_", b"**", b"MM ML", b",".join(cc.TAGS_32 + [b"zq"])):
        assert L.fplh_comment_tag_list(bad) == -2, bad
