"""The host side of BAM input (host/bam.cpp): BGZF windows inflated on the worker pool, the record walk and its tables, the
skip and error rules, against bamio's independent reading of the same bytes -- for block cuts of every kind: tiny blocks,
records across two and three blocks, cuts inside the 4-byte block_size, and windows forced small through the test hook."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from fastplong_amd import build
from tests import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    return load_host()


def load_host():
    build.build_host()
    L = C.CDLL(build.HOST_LIB)
    L.fplh_is_bam.restype = C.c_int
    L.fplh_is_bam.argtypes = [C.c_char_p]
    L.fplh_bam_read_all.restype = C.c_void_p
    L.fplh_bam_read_all.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64]
    for f in ("fplh_bam_all_n", "fplh_bam_all_batches"):
        getattr(L, f).restype = C.c_uint32
        getattr(L, f).argtypes = [C.c_void_p]
    for f in ("fplh_bam_all_bytes", "fplh_bam_all_names"):
        getattr(L, f).restype = C.c_void_p
        getattr(L, f).argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    for f in ("fplh_bam_all_rec", "fplh_bam_all_off"):
        getattr(L, f).restype = C.c_void_p
        getattr(L, f).argtypes = [C.c_void_p]
    for f in ("fplh_bam_all_error", "fplh_bam_all_warning"):
        getattr(L, f).restype = C.c_char_p
        getattr(L, f).argtypes = [C.c_void_p]
    L.fplh_bam_all_free.argtypes = [C.c_void_p]
    return L


def read_all(L, path, chunk=1 << 20, max_reads=0, window=0):
    h = L.fplh_bam_read_all(str(path).encode(), chunk, max_reads, window)
    assert h
    try:
        n = L.fplh_bam_all_n(h)
        nb = C.c_uint64()
        p = L.fplh_bam_all_bytes(h, C.byref(nb))
        raw = C.string_at(p, nb.value) if nb.value else b""
        rec = np.ctypeslib.as_array(C.cast(L.fplh_bam_all_rec(h), C.POINTER(C.c_uint64)), (n,)).copy() if n else np.zeros(0, np.uint64)
        off = np.ctypeslib.as_array(C.cast(L.fplh_bam_all_off(h), C.POINTER(C.c_uint64)), (n + 1,)).copy()
        p = L.fplh_bam_all_names(h, C.byref(nb))
        names = C.string_at(p, nb.value).split(b"\n")[:-1] if nb.value else []
        return dict(n=n, batches=L.fplh_bam_all_batches(h), raw=raw, rec=rec, off=off, names=names,
                    err=L.fplh_bam_all_error(h).decode(), warn=L.fplh_bam_all_warning(h).decode())
    finally:
        L.fplh_bam_all_free(h)


def decode_tables(t):
    """the walker's tables read back in Python: each record's (name, flag, codes, qual) at its start"""
    out = []
    raw = t["raw"]
    for i in range(t["n"]):
        r = int(t["rec"][i])
        bs = int.from_bytes(raw[r:r + 4], "little")
        one = bamio.bgzf(bamio.header(b"", ()) + raw[r:r + 4 + bs])
        (_, name, flag, codes, qual), = bamio.parse(one)
        assert int(t["off"][i + 1] - t["off"][i]) == len(codes)
        assert t["names"][i] == b"@" + name
        out.append((name, flag, codes, qual))
    return out


def _recs(seed=3, n=400, max_len=400):
    return bamio.random_records(np.random.default_rng(seed), n, max_len=max_len)


CUTS = {
    "default": dict(),
    "tiny_blocks": dict(block=7),
    "straddle_2_3": dict(block=150),
    "cut_in_block_size": "size",
    "one_block_per_record": "records",
}


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("chunk,window", [(1 << 20, 0), (3000, 0), (3000, 100), (1, 1)])
def test_walker_tables_match_twin(host, tmp_path, cut, chunk, window):
    recs = _recs()
    _, starts, raw = bamio.bam_bytes(recs)
    spec = CUTS[cut]
    if spec == "size":
        kw = dict(cuts=[s + k for s in starts for k in (1, 2, 3)])
    elif spec == "records":
        kw = dict(cuts=starts)
    else:
        kw = spec
    data = bamio.bgzf(raw, **kw)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    assert host.fplh_is_bam(str(path).encode()) == 1
    t = read_all(host, path, chunk=chunk, window=window)
    assert t["err"] == "" and t["warn"] == ""
    assert decode_tables(t) == bamio.twin_records(data)
    if chunk == 1:
        assert t["batches"] == t["n"]  # (one record per batch: every record carried over from a window that held more)


def test_reads_to_process_counts_emitted_records(host, tmp_path):
    recs = _recs(n=300)
    data, _, _ = bamio.bam_bytes(recs, block=500)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    want = bamio.twin_records(data)
    t = read_all(host, path, chunk=1 << 20, max_reads=17)
    assert t["n"] == len(want) and decode_tables(t) == want and t["batches"] == (len(want) + 16) // 17


def test_missing_eof_block_is_a_warning(host, tmp_path):
    data, _, _ = bamio.bam_bytes(_recs(n=50), eof=False)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    t = read_all(host, path)
    assert t["err"] == "" and "no BGZF EOF block" in t["warn"]
    assert decode_tables(t) == bamio.twin_records(data)


def _err(host, tmp_path, data, window=0):
    path = tmp_path / "e.bam"
    path.write_bytes(data)
    return read_all(host, path, window=window)


def test_errors(host, tmp_path):
    good = [(b"ok%d" % i, 0, bytes([1, 2, 4, 8] * 5), bytes([30] * 20)) for i in range(5)]
    # paired
    data, _, _ = bamio.bam_bytes(good[:3] + [(b"pairy", 0x41, bytes([1]), bytes([20]))] + good[3:])
    t = _err(host, tmp_path, data)
    assert "BAM record 3 (pairy)" in t["err"] and "paired" in t["err"]
    with pytest.raises(bamio.BamError):
        bamio.twin_records(data)
    # no qualities
    data, _, _ = bamio.bam_bytes(good[:2] + [(b"noq", 0, bytes([1, 2]), bytes([0xFF, 0xFF]))])
    t = _err(host, tmp_path, data)
    assert "BAM record 2 (noq)" in t["err"] and "no qualities" in t["err"]
    # ... but a secondary record without qualities is skipped, as samtools skips it
    data, _, _ = bamio.bam_bytes(good[:2] + [(b"sec", 0x100, bytes([1, 2]), bytes([0xFF, 0xFF]))])
    assert _err(host, tmp_path, data)["err"] == ""
    # block_size that disagrees with the fields
    bad = bamio.encode_record(b"short", 0, bytes([1] * 10), bytes([30] * 10), block_size_delta=-3)
    raw = bamio.header() + b"".join(bamio.encode_record(*r) for r in good[:1]) + bad
    t = _err(host, tmp_path, bamio.bgzf(raw))
    assert "BAM record 1" in t["err"] and "block_size" in t["err"]
    # cut inside a record
    raw = bamio.header() + b"".join(bamio.encode_record(*r) for r in good)
    t = _err(host, tmp_path, bamio.bgzf(raw[:-7]))
    assert "ends inside record 4" in t["err"]
    # bad CRC
    data = bytearray(bamio.bgzf(raw, block=100))
    blk = bamio.bgzf_block(raw[:100])
    data[len(blk) - 8] ^= 0x55
    t = _err(host, tmp_path, bytes(data), window=1)
    assert "file offset 0 has a bad CRC or size" in t["err"]
    # a block cut short
    t = _err(host, tmp_path, bamio.bgzf(raw, block=100)[:-40])
    assert "cut short" in t["err"]


def test_fastq_and_plain_gzip_are_not_bam(host, tmp_path):
    import gzip
    p = tmp_path / "a.fq.gz"
    p.write_bytes(gzip.compress(b"@a\nACGT\n+\nIIII\n"))
    assert host.fplh_is_bam(str(p).encode()) == 0
    p = tmp_path / "b.fq.gz"
    p.write_bytes(bamio.bgzf(b"@a\nACGT\n+\nIIII\n"))  # (bgzip'ed FASTQ: BGZF, but no BAM\1)
    assert host.fplh_is_bam(str(p).encode()) == 0


def test_damaged_block_size_fails_at_once(host, tmp_path):
    """a block_size far beyond what the record's fields need is reported as soon as the fixed fields are in, not after the
    reader has inflated what it claims"""
    good = [(b"ok%d" % i, 0, bytes([1, 2, 4, 8] * 5), bytes([30] * 20)) for i in range(5)]
    bad = bytearray(bamio.encode_record(b"huge", 0, bytes([1] * 10), bytes([30] * 10)))
    bad[0:4] = (0xFFFFFF00).to_bytes(4, "little")
    raw = bamio.header() + b"".join(bamio.encode_record(*r) for r in good) + bytes(bad) + bamio.encode_record(*good[0]) * 50
    t = _err(host, tmp_path, bamio.bgzf(raw, block=64), window=1)
    assert "BAM record 5 (huge)" in t["err"] and "block_size" in t["err"]


def test_tiny_first_blocks_and_gzip_name_field(host, tmp_path):
    """BAM recognised when its first blocks inflate to fewer than 4 bytes; a member with an FNAME field (outside the BGZF spec,
    written by some tools) inflates on the zlib path as on libdeflate's"""
    recs = _recs(n=40)
    _, starts, raw = bamio.bam_bytes(recs)
    blocks = [bamio.bgzf_block(raw[0:1]), bamio.bgzf_block(raw[1:3])]
    named = bytearray(bamio.bgzf_block(raw[3:500]))
    named[3] |= 8  # FNAME: a NUL-terminated name behind the extra field, BSIZE grown to match
    named = named[:18] + b"part.bam\0" + named[18:]
    bsize = int.from_bytes(named[16:18], "little") + 9
    named[16:18] = bsize.to_bytes(2, "little")
    data = b"".join(blocks) + bytes(named) + bamio.bgzf(raw[500:])
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    assert host.fplh_is_bam(str(path).encode()) == 1
    want = bamio.twin_records(bamio.bgzf(raw))
    t = read_all(host, path, window=1)
    assert t["err"] == "" and decode_tables(t) == want
    # the same through zlib (a process of its own: the choice of inflater is made once per process)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import test_host_bam as T\n"
            "L = T.load_host()\n"
            "t = T.read_all(L, %r, window=1)\n"
            "assert L.fplh_is_bam(%r) == 1 and t['err'] == '' and t['n'] == %d, t['err']\n"
            % (ROOT, str(path), str(path).encode(), len(want)))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FPLH_NO_LIBDEFLATE="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
