"""--keep_tags on the host (README "BAM output"): the shared rule (fastplong_amd/csrc/bam_tag_rules.h), the host form
(host/bam_tags.cpp, host/bam_out.cpp), the header with the input's @RG lines and the reader's check of the auxiliary fields, through
their test hooks, against the plain-Python model of tests/bam_tag_cases.py, byte for byte."""
import ctypes as C
import gzip

import numpy as np
import pytest

from fastplong_amd import bgzf
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.bgzf_out_cases import split_blocks
from tests.gzcheck import load_hostlib


@pytest.fixture(scope="module")
def L():
    lib = load_hostlib()
    lib.fplh_bam_tag_walk.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.fplh_bam_tag_region.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.fplh_bam_header_rg.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    lib.fplh_bam_tag_form.restype = C.c_int
    lib.fplh_bam_tag_form.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
    lib.fplh_bgzf_into.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for f in ("fplh_bam_read_all", "fplh_bam_read_all_tags"):
        getattr(lib, f).restype = C.c_void_p
        getattr(lib, f).argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64]
    lib.fplh_bam_all_n.restype = C.c_uint32
    lib.fplh_bam_all_n.argtypes = [C.c_void_p]
    lib.fplh_bam_all_error.restype = C.c_char_p
    lib.fplh_bam_all_error.argtypes = [C.c_void_p]
    lib.fplh_bam_all_header.restype = C.c_void_p
    lib.fplh_bam_all_header.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fplh_bam_all_free.argtypes = [C.c_void_p]
    return lib


def taken(L, out, n):
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    return s


def lib_walk(L, region):
    """(prefix, kept, positional, whole) by the shared rule; the region sits at the end of an exact-size buffer"""
    out = (C.c_uint64 * 4)()
    L.fplh_bam_tag_walk(C.create_string_buffer(region, len(region)).raw, len(region), out)
    return tuple(out)


def model_walk(region):
    fields, prefix = tc.walk(region)
    return prefix, sum(n for _, n, pos in fields if not pos), int(any(pos for _, _, pos in fields)), int(prefix == len(region))


def test_the_walk_on_every_region_and_every_cut_of_it(L):
    for key, region in tc.REGIONS.items():
        assert lib_walk(L, region) == model_walk(region), key
        assert model_walk(region)[3] == 1, key  # (the case list's regions all parse)
    for key, (region, prefix) in tc.MALFORMED.items():
        assert lib_walk(L, region) == model_walk(region), key
        assert model_walk(region)[0] == prefix and model_walk(region)[3] == 0, key
    # a region cut at every byte: the prefix never passes the cut, and is the model's
    for key in ("scalars", "alternating", "mods", "Z_9", "H_8", "Bs_1", "Bf_0", "len_33", "len_34"):
        region = tc.REGIONS[key]
        for cut in range(len(region) + 1):
            got = lib_walk(L, region[:cut])
            assert got == model_walk(region[:cut]) and got[0] <= cut, (key, cut)


def test_positional_set_and_region_of_a_record(L):
    for tag in (b"MM", b"Mm", b"ML", b"Ml", b"MN"):
        assert lib_walk(L, tc.scalar(tag, b"i", 1))[1:3] == (0, 1)
    for tag in (b"Mn", b"mM", b"MX", b"NM", b"mv", b"ml"):
        assert lib_walk(L, tc.scalar(tag, b"i", 1))[1:3] == (7, 0)
    assert lib_walk(L, tc.barray(b"xx", b"C", []))[1:3] == (0, 1)  # every B array
    rng = np.random.default_rng(2)
    for l_seq in (0, 1, 2, 33):
        for n_cigar in (0, 2):
            tags = tc.K1 + tc.P2
            rec = bamio.encode_record(b"nm%d" % l_seq, 4, rng.integers(0, 16, l_seq, dtype=np.uint8).tobytes(), bytes(l_seq), n_cigar=n_cigar, tags=tags)
            at, n = C.c_uint64(), C.c_uint64()
            L.fplh_bam_tag_region(rec, C.byref(at), C.byref(n))
            assert rec[at.value:at.value + n.value] == tags == tc.aux_region(rec) and at.value + n.value == len(rec)


def host_form(L, tmp_path, recs, res, threads, frags=None, regs=None):
    data = tc.input_bam(recs, block=20000)
    p = tmp_path / "in.bam"
    p.write_bytes(data)
    seq, qual, off, _ = bamio.twin_csr(data)
    res = np.ascontiguousarray(res)
    assert len(off) - 1 == len(res)
    out, n, fo, fn = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    stats = (C.c_uint64 * 8)()
    seq, qual = np.ascontiguousarray(seq), np.ascontiguousarray(qual)
    if frags is None:
        fr, nf, rg, nr = None, 0xFFFFFFFF, None, 0
    else:
        frags, regs = np.ascontiguousarray(frags), np.ascontiguousarray(regs)
        fr, nf, rg, nr = frags.ctypes.data, len(frags), regs.ctypes.data, len(regs)
    assert L.fplh_bam_tag_form(str(p).encode(), seq.ctypes.data, qual.ctypes.data, res.ctypes.data, len(res), fr, nf, rg, nr, threads,
                               C.byref(out), C.byref(n), C.byref(fo), C.byref(fn), stats) == 0
    return taken(L, out, n), taken(L, fo, fn), list(stats[:4]), list(stats[4:])


@pytest.mark.parametrize("threads", [1, 7])
def test_host_form_equals_the_model_on_the_case_list(L, tmp_path, threads):
    recs, res = tc.case_list(malformed=True)
    want = tc.expected(recs, res)
    got = host_form(L, tmp_path, recs, res, threads)
    assert got[2:] == (want[2], want[3])
    assert got[0] == want[0] and got[1] == want[1]
    assert want[2][0] > 50 and want[2][1] > 50 and want[2][3] > 5 and want[3][0] > 5 and want[3][1] >= 3  # every counter moves
    # the records still read back as the reads they are: bamio ignores what follows the qualities
    plain = tc.expected([(n, f, c, q, bamio.encode_record(n, f, c, q)) for n, f, c, q, _ in recs], res)
    strip = lambda raw: [r[1:] for r in bamio.parse(bc.file_bytes(bamio.bgzf(raw, eof=False)))]
    assert strip(got[0]) == strip(plain[0]) and len(got[0]) - len(plain[0]) == want[2][2]


def test_break_and_mask_runs_change_every_record(L, tmp_path):
    from fastplong_amd import abi
    recs, res = tc.case_list()
    recs, res = recs[:60], res[:len([r for r in recs[:60] if not r[1] & 0x900])].copy()
    kept = [r for r in recs if not r[1] & 0x900]
    frags = []
    for i, (r, rec) in enumerate(zip(res, kept)):
        l_seq = len(rec[2])
        r["n_frag"], r["frag_start"], r["frag_len"] = 255, 0, 0
        if r["dropped"]:
            continue
        if i % 3 == 0 and l_seq > 20:  # two output reads
            frags += [(i, 0, 0, 9, 0, 0, 1, abi.FPL_PASS_FILTER, 0, 30, (0, 0, 0)), (i, 1, 12, l_seq - 12, 0, 0, 2, abi.FPL_PASS_FILTER, 0, 30, (0, 0, 0))]
        elif i % 3 == 1:
            frags.append((i, 0, 0, l_seq, 0, 0, 0, abi.FPL_PASS_FILTER, 0, 30, (0, 0, 0)))  # the whole read: changed all the same
        else:
            frags.append((i, 0, int(r["r1_start"]), int(r["r1_len"]), 0, 0, 0, abi.FPL_FAIL_QUALITY, 0, 30, (0, 0, 0)))
    frags = np.array(frags, np.dtype(abi.FRAGMENT_DTYPE))
    regs = np.zeros(0, np.dtype(abi.REGION_DTYPE))
    want = tc.expected(recs, res, fragment_mode=True, frags=frags)
    got = host_form(L, tmp_path, recs, res, 3, frags, regs)
    assert got == (want[0], want[1], want[2], want[3]) and want[2][1] > 3 and len(want[1]) > 100


def lib_header(L, text, mode=0):
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_bam_header_rg(text, len(text), mode, C.byref(out), C.byref(n)) == 0
    return taken(L, out, n)


@pytest.mark.parametrize("n_rg", [0, 1, 2, 1500])
def test_header_with_read_groups(L, n_rg):
    lines = [b"@RG\tID:group%d\tPL:ONT\tDS:%s\n" % (k, b"x" * 30) for k in range(n_rg)]
    text = b"@HD\tVN:1.6\tSO:unknown\n" + b"@PG\tID:a\n".join(lines) + b"@CO\tbetween\n"
    want = tc.header_raw(text)
    assert tc.read_group_lines(text) == b"".join(lines)
    assert lib_header(L, text) == want == lib_header(L, b"".join(lines), mode=1)
    if n_rg == 0:
        assert want == bc.HEADER_RAW
    # the Python front end's block, and the host's blocks: nothing but header, several when it passes 65 280 bytes
    assert gzip.decompress(bgzf.bam_header(read_groups=b"".join(lines))) == want
    assert bgzf.bam_header() == bgzf.bam_header(read_groups=b"") and gzip.decompress(bgzf.bam_header()) == bc.HEADER_RAW
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_bgzf_into(want, len(want), 4, C.byref(out), C.byref(n)) == 0
    blocks = split_blocks(taken(L, out, n), eof=False)
    assert b"".join(gzip.decompress(b) for b in blocks) == want
    assert len(blocks) == (len(want) + 65279) // 65280 and (n_rg < 1500 or len(blocks) == 2)
    assert all(len(b) <= 65536 for b in bgzf_blocks_of(bgzf.bam_header(read_groups=b"".join(lines))))


def bgzf_blocks_of(data):
    return split_blocks(data, eof=False)


def test_read_group_lines_edge_cases(L):
    for text, want in [(b"", b""), (b"@RG\tID:a", b"@RG\tID:a\n"), (b"@RG\tID:a\n@HD\tx\n@RG\tID:b", b"@RG\tID:a\n@RG\tID:b\n"),
                       (b"@RG ID:a\n@RGX\tID:a\nx@RG\tID:c\n", b""), (b"@RG\tID:a\n\0\0\0@RG\tID:z\n", b"@RG\tID:a\n"), (tc.RG_HEADER, None)]:
        got = tc.read_group_lines(text)
        assert want is None or got == want
        assert lib_header(L, text) == tc.header_raw(text)
    assert tc.read_group_lines(tc.RG_HEADER).count(b"\n") == 2


def read_all(L, fn, path):
    h = getattr(L, fn)(str(path).encode(), 1 << 20, 0, 0)
    assert h
    n = C.c_uint64()
    p = L.fplh_bam_all_header(h, C.byref(n))
    got = L.fplh_bam_all_n(h), L.fplh_bam_all_error(h).decode(), C.string_at(p, n.value) if n.value else b""
    L.fplh_bam_all_free(h)
    return got


@pytest.mark.parametrize("key", sorted(tc.MALFORMED))
def test_reader_refuses_fields_that_do_not_parse_only_under_the_flag(L, tmp_path, key):
    rng = np.random.default_rng(9)
    good = [(b"g%d" % i, 4, rng.integers(0, 16, 30, dtype=np.uint8).tobytes(), bytes([20] * 30)) for i in range(6)]
    recs = [(n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.REGIONS["alternating"])) for n, f, c, q in good]
    bad = (b"the_bad_one", 4, good[0][2], good[0][3])
    # a skipped record with damaged fields in front of it is not looked at
    skipped = (b"sec", 0x100, good[0][2], good[0][3])
    recs[2:2] = [skipped + (bamio.encode_record(*skipped, tags=b"\1\2"),)]
    recs[4:4] = [bad + (bamio.encode_record(*bad, tags=tc.MALFORMED[key][0]),)]
    p = tmp_path / "bad.bam"
    p.write_bytes(tc.input_bam(recs, header_text=tc.RG_HEADER))
    n, err, hdr = read_all(L, "fplh_bam_read_all_tags", p)
    assert err == "BAM record 4 (the_bad_one): the auxiliary fields do not parse" and hdr == tc.RG_HEADER
    n, err, hdr = read_all(L, "fplh_bam_read_all", p)
    assert (n, err, hdr) == (7, "", tc.RG_HEADER)
    good_file = tmp_path / "good.bam"
    good_file.write_bytes(tc.input_bam([r for r in recs if r[0] != b"the_bad_one"]))
    assert read_all(L, "fplh_bam_read_all_tags", good_file)[:2] == (6, "")
