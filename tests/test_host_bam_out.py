"""fplh::fastq_to_bam_records and fplh::bam_header_bytes (fastplong_amd/host/bam_out.cpp) through their test hooks, and the same
unit as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/host_bamout): formatted FASTQ text ->
the records of README "BAM output".  Expected bytes come from the plain-Python restatement of the rule in tests/bam_out_cases.py;
the file made of them is read back by tests/bamio.py."""
import ctypes as C

import numpy as np
import pytest

from tests import bam_out_cases as bc
from tests import bamio
from tests.gzcheck import load_hostlib
from tests.host_bamout import build as sanitized


@pytest.fixture(scope="module")
def hostlib():
    L = load_hostlib()
    L.fplh_fastq_to_bam_records.restype = C.c_int
    L.fplh_fastq_to_bam_records.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.fplh_bam_header_bytes.restype = C.c_int
    L.fplh_bam_header_bytes.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.fplh_bam_base_table.argtypes = [C.c_void_p]
    return L


def to_records(L, text):
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_fastq_to_bam_records(text, len(text), C.byref(out), C.byref(n)) == 0
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    return s


def convert(L, text):
    """the records by the library's hook and by the sanitized program: the same bytes, the rule's fixed fields"""
    got = to_records(L, text)
    hdr, san = sanitized.convert(text)
    assert hdr == bc.HEADER_RAW and san == got
    assert bc.check_fixed_fields(got) == len(bc.fastq_records(text))
    return got


def fq(name, seq, qual=None, plus=b"+"):
    return name + b"\n" + seq + b"\n" + plus + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def test_header(hostlib):
    out, n = C.c_void_p(), C.c_uint64()
    assert hostlib.fplh_bam_header_bytes(C.byref(out), C.byref(n)) == 0
    h = C.string_at(out, n.value)
    hostlib.fplh_free(out)
    assert h == bc.HEADER_RAW == b"BAM\1" + (len(bc.HEADER_TEXT)).to_bytes(4, "little") + bc.HEADER_TEXT + b"\0\0\0\0"
    assert bamio.parse(bc.file_bytes(b"")) == []  # a file no read reached: the header block and the EOF block


def test_all_256_base_values(hostlib):
    tab = (C.c_uint8 * 256)()
    hostlib.fplh_bam_base_table(tab)
    assert list(tab) == bc.TABLE
    assert [i for i in range(256) if bc.TABLE[i] != 15] == sorted(b"=ACMGRSVTWYHKDBacmgrsvtwyhkdb")  # (N is 15 like all the rest)
    assert [bc.TABLE[c] for c in b"=ACMGRSVTWYHKDBN"] == list(range(16))
    # ... and through a record: every byte a line can hold (all but the line end), at an even and at an odd place
    vals = bytes(v for v in range(256) if v != 10)
    for seq in (vals, b"A" + vals):
        text = fq(b"@all", seq)
        got = convert(hostlib, text)
        assert got == bc.records(text)
        (_, name, flag, codes, qual), = bamio.parse(bc.file_bytes(bamio.bgzf_block(got)))
        assert list(codes) == [bc.TABLE[c] for c in seq]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255])
def test_lengths(hostlib, n):
    rng = np.random.default_rng(n)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes()
    qual = rng.integers(33, 127, n, dtype=np.uint8).tobytes()
    text = fq(b"@r%d" % n, seq, qual) + fq(b"@behind", b"ACG", b"#$%")
    got = convert(hostlib, text)
    assert got == bc.records(text)
    assert len(got) == (36 + len(b"r%d" % n) + 1 + (n + 1) // 2 + n) + (36 + 7 + 2 + 3)
    assert bamio.bam_to_fastq(bc.file_bytes(bamio.bgzf_block(got))) == text


NAMES = {
    "space": (b"@read1 runid=7 ch=2", b"read1"),
    "tab_at_byte_0": (b"@\tx", b"*"),
    "tab": (b"@a\tb c", b"a"),
    "254": (b"@" + b"n" * 254, b"n" * 254),
    "255": (b"@" + b"n" * 255, b"n" * 254),
    "300": (b"@" + b"m" * 300, b"m" * 254),
    "300_space_behind_254": (b"@" + b"m" * 260 + b" x", b"m" * 254),
    "empty": (b"@", b"*"),
    "empty_line": (b"", b"*"),
    "left": (b"@split-by-adapter-left-r9 ch=1", b"split-by-adapter-left-r9"),
    "right": (b"@split-by-adapter-right-" + b"k" * 250, b"split-by-adapter-right-" + b"k" * 231),
    "failed": (b"@r5 failed_too_short", b"r5"),
}


@pytest.mark.parametrize("case", sorted(NAMES))
def test_names(hostlib, case):
    line, want = NAMES[case]
    assert bc.cut_name(line) == want
    text = fq(line, b"ACGTA", b"!#5I~", plus=b"+" + line[1:]) + fq(b"@next", b"TT")
    got = convert(hostlib, text)
    assert got == bc.records(text)
    recs = bamio.parse(bc.file_bytes(bamio.bgzf_block(got)))
    assert [r[1] for r in recs] == [want, b"next"]
    assert bamio.bam_to_fastq(bc.file_bytes(bamio.bgzf_block(got))) == fq(b"@" + want, b"ACGTA", b"!#5I~") + fq(b"@next", b"TT")


def test_quality_range(hostlib):
    q = bytes([33, 126, 34, 125, 32, 0, 255, 11])  # the two ends, their neighbours, and what lies outside
    text = fq(b"@q", b"ACGTACGT", q)
    got = convert(hostlib, text)
    assert got == bc.records(text)
    assert got[-8:] == bytes([0, 93, 1, 92, 0, 0, 222, 0])


def test_round_trip_of_many_records(hostlib):
    rng = np.random.default_rng(5)
    text = b""
    for i in range(400):
        n = int(rng.choice([0, 1, 2, 3, 15, 16, 17, 31, 32, 33, int(rng.integers(34, 3000))]))
        text += fq(b"@r%d %s" % (i, b"x" * int(rng.integers(0, 40))), rng.choice(np.frombuffer(bamio.CODES[1:], np.uint8), n).tobytes(),
                   rng.integers(33, 127, n, dtype=np.uint8).tobytes(), plus=b"+" if i % 3 else b"+again")
    got = convert(hostlib, text)
    assert got == bc.records(text)
    data = bc.file_bytes(bamio.bgzf(got, eof=False))
    assert bamio.bam_to_fastq(data) == bc.cut_text(text)
