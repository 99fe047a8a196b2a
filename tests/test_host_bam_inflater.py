"""BamReader with an inflater (host/bam.h: set_inflater), through the read-all hook with a ctypes callback that inflates with
Python's zlib: whatever the callback does -- vouch for every block, refuse some or all, fail --, the reader gives what it gives
without one: bytes, record starts, offsets, names, batch count, error text, warning text."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import bamio
from tests.bgzf_cases import BLOCK_DTYPE
from tests.test_host_bam import CUTS, _recs, load_host, read_all

CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64)


@pytest.fixture(scope="module")
def host():
    L = load_host()
    L.fplh_bam_read_all_with.restype = C.c_void_p
    L.fplh_bam_read_all_with.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, CB, C.c_void_p]
    for f in ("fplh_bam_all_device", "fplh_bam_all_refused"):
        getattr(L, f).restype = C.c_uint64
        getattr(L, f).argtypes = [C.c_void_p]
    return L


class Inflater:
    """mode "all": every block; "third": refuses every third block it sees; "none": refuses all; "fail": the call fails"""

    def __init__(self, mode):
        self.mode, self.seen, self.calls, self.blocks_per_call = mode, 0, 0, []
        self.cb = CB(self.call)

    def call(self, user, comp, comp_bytes, blocks, n, out, out_bytes):
        self.calls += 1
        self.blocks_per_call.append(n)
        if self.mode == "fail":
            return -3
        comp = C.string_at(comp, comp_bytes)
        blk = np.ctypeslib.as_array(C.cast(blocks, C.POINTER(C.c_uint8)), (32 * n,)).view(BLOCK_DTYPE)
        dst = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (out_bytes,)) if out_bytes else None
        for b in blk:
            self.seen += 1
            assert b["isize"] > 0 and b["out_off"] + b["isize"] <= out_bytes and b["comp_off"] + b["comp_len"] <= comp_bytes
            if self.mode == "none" or (self.mode == "third" and self.seen % 3 == 0):
                b["status"] = 1
                continue
            try:
                d = zlib.decompressobj(-15)
                data = d.decompress(comp[int(b["comp_off"]):int(b["comp_off"]) + int(b["comp_len"])])
                ok = d.eof and len(data) == b["isize"] and zlib.crc32(data) == b["crc32"]
            except zlib.error:
                ok = False
            if ok:
                dst[int(b["out_off"]):int(b["out_off"]) + len(data)] = np.frombuffer(data, np.uint8)
            b["status"] = 0 if ok else 3
        return 0


def read_with(L, path, inf, chunk=1 << 20, max_reads=0, window=0):
    """read_all of tests/test_host_bam.py through the hook that takes a callback -> (tables, blocks on the device, refused)"""
    plain = L.fplh_bam_read_all
    counts = []

    def hooked(p, c, m, w):
        h = L.fplh_bam_read_all_with(p, c, m, w, inf.cb, None)
        if h:
            counts.append((L.fplh_bam_all_device(h), L.fplh_bam_all_refused(h)))
        return h

    L.fplh_bam_read_all = hooked
    try:
        t = read_all(L, path, chunk=chunk, max_reads=max_reads, window=window)
    finally:
        L.fplh_bam_read_all = plain
    return t, counts[0][0], counts[0][1]


def same(a, b):
    assert a["n"] == b["n"] and a["batches"] == b["batches"]
    assert a["raw"] == b["raw"] and a["names"] == b["names"]
    assert np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["off"], b["off"])
    assert a["err"] == b["err"] and a["warn"] == b["warn"]


MODES = ["all", "third", "none", "fail"]


def check_counts(mode, inf, dev, refused, expect_blocks=True):
    if mode == "all":
        assert refused == 0 and (dev > 0 or not expect_blocks)
    elif mode == "third":
        assert dev + refused == inf.seen and refused == inf.seen // 3
    elif mode == "none":
        assert dev == 0 and refused == inf.seen
    else:
        assert dev == 0 and refused == 0 and (inf.calls > 0 or not expect_blocks)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("chunk,window", [(1 << 20, 0), (3000, 0), (3000, 100), (1, 1)])
def test_same_tables_as_without_an_inflater(host, tmp_path, cut, chunk, window, mode):
    recs = _recs()
    _, starts, raw = bamio.bam_bytes(recs)
    spec = CUTS[cut]
    if spec == "size":
        kw = dict(cuts=[s + k for s in starts for k in (1, 2, 3)])
    elif spec == "records":
        kw = dict(cuts=starts)
    else:
        kw = spec
    path = tmp_path / "x.bam"
    path.write_bytes(bamio.bgzf(raw, **kw))
    want = read_all(host, path, chunk=chunk, window=window)
    assert want["err"] == "" and want["n"] > 100
    inf = Inflater(mode)
    got, dev, refused = read_with(host, path, inf, chunk=chunk, window=window)
    same(got, want)
    check_counts(mode, inf, dev, refused)


def test_the_window_is_what_the_batch_still_takes(host, tmp_path):
    """one call carries the blocks of a whole batch, whatever the host path's window is"""
    data, _, _ = bamio.bam_bytes(_recs(n=400), block=500)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    inf = Inflater("all")
    got, dev, _ = read_with(host, path, inf, chunk=1 << 20, window=100)
    same(got, read_all(host, path, chunk=1 << 20, window=100))
    assert got["batches"] == 1 and inf.calls == 1 and inf.blocks_per_call[0] == dev > 50


@pytest.mark.parametrize("mode", MODES)
def test_errors_and_warnings_are_the_host_s(host, tmp_path, mode):
    good = [(b"ok%d" % i, 0, bytes([1, 2, 4, 8] * 5), bytes([30] * 20)) for i in range(5)]
    raw = bamio.header() + b"".join(bamio.encode_record(*r) for r in good)
    files = {}
    # a truly bad CRC, in the third block: the message names its file offset
    blocks = [bamio.bgzf_block(raw[i:i + 100]) for i in range(0, len(raw), 100)]
    bad = bytearray(b"".join(blocks) + bamio.bgzf(b""))
    at = len(blocks[0]) + len(blocks[1])
    bad[at + len(blocks[2]) - 8] ^= 0x55
    files["bad_crc"] = (bytes(bad), "file offset %d has a bad CRC or size" % at)
    # two bad blocks: the smallest offset is reported
    bad2 = bytearray(bad)
    bad2[len(blocks[0]) + len(blocks[1]) - 8] ^= 0x55
    files["bad_crc_twice"] = (bytes(bad2), "file offset %d has a bad CRC or size" % len(blocks[0]))
    # a damaged payload with the trailer left alone
    bad3 = bytearray(bad2)
    bad3[20] ^= 0xFF
    files["bad_payload"] = (bytes(bad3), "file offset 0 has a bad CRC or size")
    files["no_eof"] = (bamio.bam_bytes(_recs(n=50), eof=False)[0], None)
    files["cut_in_record"] = (bamio.bgzf(raw[:-7]), "ends inside record 4")
    files["block_cut_short"] = (bamio.bgzf(raw, block=100)[:-40], "cut short")
    files["paired"] = (bamio.bam_bytes(good[:3] + [(b"pairy", 0x41, bytes([1]), bytes([20]))] + good[3:])[0], "paired")
    for name, (data, text) in files.items():
        path = tmp_path / (name + ".bam")
        path.write_bytes(data)
        for window in (0, 1):
            want = read_all(host, path, window=window)
            if text:
                assert text in want["err"], (name, want["err"])
            else:
                assert want["err"] == "" and "no BGZF EOF block" in want["warn"]
            inf = Inflater(mode)
            got, dev, refused = read_with(host, path, inf, window=window)
            same(got, want)


@pytest.mark.parametrize("mode", MODES)
def test_a_record_larger_than_the_batch(host, tmp_path, mode):
    rng = np.random.default_rng(5)
    big = (b"big", 0, rng.integers(1, 16, 200000, dtype=np.uint8).tobytes(), rng.integers(0, 60, 200000, dtype=np.uint8).tobytes())
    recs = _recs(n=20) + [big] + _recs(seed=4, n=20)
    data, _, _ = bamio.bam_bytes(recs, block=3000)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    for chunk, window in ((5000, 0), (5000, 700)):
        want = read_all(host, path, chunk=chunk, window=window)
        assert want["err"] == "" and want["n"] > 20
        inf = Inflater(mode)
        got, dev, refused = read_with(host, path, inf, chunk=chunk, window=window)
        same(got, want)
        check_counts(mode, inf, dev, refused)


def test_reads_limit(host, tmp_path):
    data, _, _ = bamio.bam_bytes(_recs(n=300), block=500)
    path = tmp_path / "x.bam"
    path.write_bytes(data)
    for mode in MODES:
        same(read_with(host, path, Inflater(mode), chunk=4000, max_reads=7)[0], read_all(host, path, chunk=4000, max_reads=7))
