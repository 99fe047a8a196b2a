"""--reindex_comments on the host (README "Comments of a FASTQ input"): the shared rule (fastplong_amd/csrc/fq_comment_rules.h) in the
host form (host/fq_comments.cpp) through its test hooks, against the plain-Python model of tests/fq_comment_cases.py, byte for byte,
for --out and --failed_out with given results arrays, on the whole case list; the five counts; a --break / --mask run; and the
formatter's text wherever the rule says the line stays."""
import ctypes as C

import numpy as np
import pytest

from fastplong_amd import abi
from tests import fq_comment_cases as fc
from tests.gzcheck import load_hostlib


@pytest.fixture(scope="module")
def L():
    lib = load_hostlib()
    lib.fplh_fq_comment_form.restype = lib.fplh_fq_comment_line.restype = C.c_int
    lib.fplh_fq_comment_form.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fplh_fq_comment_line.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fplh_format_batch_parallel.restype = C.c_int
    lib.fplh_format_batch_parallel.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_uint64)]
    return lib


def read_batch(L, tmp, reads, crlf=()):
    p = tmp / "in.fq"
    p.write_bytes(fc.fastq(reads, crlf))
    b = L.fplh_batch_read(str(p).encode(), 1 << 40, 0x3FFFFFFF)
    assert b and L.fplh_batch_n(b) == len(reads)
    return b


@pytest.fixture(scope="module")
def cases(L, tmp_path_factory):
    """the case list, read by the host's reader as one batch, and what the model makes of it, once"""
    reads, res, _ = fc.case_list()
    b = read_batch(L, tmp_path_factory.mktemp("fqc"), reads, fc.CRLF)
    yield reads, res, b, fc.expected(reads, res)
    L.fplh_batch_free(b)


def host_form(L, b, res, threads, frags=None):
    """-> (--out text, --failed_out text, the five counts of each)"""
    res = np.ascontiguousarray(res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    stats = (C.c_uint64 * 10)()
    regs = np.zeros(1, np.dtype(abi.REGION_DTYPE))
    fr, nf = (None, 0xFFFFFFFF) if frags is None else (frags.ctypes.data, len(frags))
    assert L.fplh_fq_comment_form(b, res.ctypes.data, fr, nf, regs.ctypes.data, 0, threads, C.byref(out), C.byref(n), C.byref(fo), C.byref(fn), stats) == 0
    got = C.string_at(out, n.value), C.string_at(fo, fn.value), list(stats[:5]), list(stats[5:])
    L.fplh_free(out), L.fplh_free(fo)
    return got


def formatter_text(L, b, res, threads=3):
    res = np.ascontiguousarray(res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    assert L.fplh_format_batch_parallel(b, res.ctypes.data, threads, C.byref(out), C.byref(n), C.byref(fo), C.byref(fn)) == 0
    got = C.string_at(out, n.value), C.string_at(fo, fn.value)
    L.fplh_free(out), L.fplh_free(fo)
    return got


def rule_line(L, fmt, line, bases, s, n, changed, failed=False, fragment_mode=False):
    out, k, counts = C.c_void_p(), C.c_uint64(), (C.c_uint64 * 5)()
    assert L.fplh_fq_comment_line(fmt, len(fmt), line, len(line), bases, len(bases), s, n, changed, failed, fragment_mode, C.byref(out), C.byref(k), counts) == 0
    got = C.string_at(out, k.value)
    L.fplh_free(out)
    return got, list(counts)


def test_the_worked_example(L):
    line, bases, s, n, want = fc.WORKED
    assert rule_line(L, line, line, bases, s, n, True) == (want, [1, 0, 2, 1, 0])
    assert rule_line(L, line, line, bases, 0, 12, False) == (line, [0] * 5)
    # --failed_out: the word goes behind the name part, for an unchanged record too
    assert rule_line(L, line + b" failed_too_short", line, bases, s, n, True, failed=True)[0] == want.replace(b"@r1\t", b"@r1 failed_too_short\t")
    assert rule_line(L, line + b" failed_quality_filter", line, bases, 0, 12, False, failed=True)[0] == line.replace(b"@r1\t", b"@r1 failed_quality_filter\t")
    # a split prefix stays behind the '@'
    fmt = b"@split-by-adapter-left-" + line[1:]
    assert rule_line(L, fmt, line, bases, 0, 7, True)[0] == b"@split-by-adapter-left-r1\tRG:Z:a\tMM:Z:C+m?,1,0;\tML:B:C,10,20\tMN:i:7"
    # --break / --mask: nothing is re-indexed, the positional fields go
    assert rule_line(L, b"@r2-" + line[1:], line, bases, 4, 8, True, fragment_mode=True) == (b"@r2-r1\tRG:Z:a", [0, 1, 0, 0, 0])
    # not tags, no TAB: the formatter's line
    bad = line + b"\t"
    assert rule_line(L, bad + b" failed_too_short", bad, bases, s, n, True, failed=True) == (bad + b" failed_too_short", [0, 0, 0, 0, 1])
    assert rule_line(L, b"@r1 a=b", b"@r1 a=b", bases, s, n, True) == (b"@r1 a=b", [0] * 5)


@pytest.mark.parametrize("threads", [1, 5])
def test_host_form_equals_the_model_on_the_case_list(L, cases, threads):
    reads, res, b, want = cases
    got = host_form(L, b, res, threads)
    assert got[2:] == (want[2], want[3])
    assert got[0] == want[0] and got[1] == want[1]
    assert b"split-by-adapter-right-" in got[0] and b" failed_too_short\tRG:Z:run7_grp\tMM:Z:" in got[1] and b"\r" not in got[0]


def test_lines_the_rule_leaves_are_the_formatter_s(L, cases):
    """unchanged reads, reads without a TAB and reads whose region is not tags: byte for byte the text of a run without the flag
    (a --failed_out record of a tagged read differs only in where its failure word stands)"""
    reads, res, b, _ = cases
    got, plain = host_form(L, b, res, 4), formatter_text(L, b, res)
    a, p = got[0].split(b"\n"), plain[0].split(b"\n")
    assert len(a) == len(p) and a[1::4] == p[1::4] and a[2::4] == p[2::4] and a[3::4] == p[3::4]
    same = sum(x == y for x, y in zip(a[::4], p[::4]))
    assert 150 < same < len(a) // 4 - 500
    assert all(len(x) <= len(y) for x, y in zip(a[::4], p[::4]))  # (the rule's SIZE argument)
    for x, y in zip(got[1].split(b"\n")[::4], plain[1].split(b"\n")[::4]):
        assert len(x) <= len(y) and (b"\t" not in y or x.split(b"\t")[0].startswith(y.split(b"\t")[0]))


def test_nothing_passes(L, tmp_path):
    reads, res = fc.nothing_passes()
    b = read_batch(L, tmp_path, reads)
    want = fc.expected(reads, res)
    got = host_form(L, b, res, 3)
    L.fplh_batch_free(b)
    assert got == want and got[0] == b"" and got[2] == [0] * 5 and len(got[1]) > 1000


def test_a_break_mask_run_re_indexes_nothing(L, cases):
    reads, res0, b, _ = cases
    res = res0.copy()
    frags = []
    for i, r in enumerate(res):
        if i >= 400:
            r["dropped"], r["n_frag"] = 1, 0
        r["n_frag"], r["frag_start"], r["frag_len"] = 255, 0, 0
        if r["dropped"]:
            continue
        h = int(r["r1_len"]) // 2
        if i % 3 == 0 and h > 4:  # two output reads, the second behind a break
            frags.append((i, 0, int(r["r1_start"]), h, 0, 0, 0, abi.FPL_PASS_FILTER, 0, 30, (0, 0, 0)))
            frags.append((i, 1, int(r["r1_start"]) + h, int(r["r1_len"]) - h, 0, 0, 1, abi.FPL_PASS_FILTER, 0, 30, (0, 0, 0)))
        else:
            code = abi.FPL_PASS_FILTER if i % 3 == 1 else abi.FPL_FAIL_QUALITY
            frags.append((i, 0, int(r["r1_start"]), int(r["r1_len"]), 0, 0, 0, code, 0, 30, (0, 0, 0)))
    frags = np.array(frags, np.dtype(abi.FRAGMENT_DTYPE))
    want = fc.expected(reads, res, fragment_mode=True, frags=frags)
    got = host_form(L, b, res, 2, frags=frags)
    assert got == want
    assert b"\tMM:Z:" not in got[0].replace(b"\tMM:Z:C+m;", b"") and b"\tML:B:" not in got[1] and b"\tRG:Z:run7_grp" in got[0] and b"@r1-" in got[0]
    assert got[2][0] == got[3][0] == 0 and got[2][1] > 50 and got[3][1] > 20 and got[2][4] > 10
