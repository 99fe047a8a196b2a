"""The single-member lane of the host's gzip expansion with an inflater hook (host/gzip.h: set_gzip_inflater), through the test
hooks with a ctypes callback backed by Python's zlib: whatever the callback does -- vouch for every window, refuse every third,
refuse all, fail --, the lane gives the memory it gives without one, and a damaged file is reported by the same reader with the
same words."""
import ctypes as C
import zlib

import numpy as np
import pytest

from fastplong_amd import build
from tests import gzip_cases as gc

CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p)
WINDOW = 20000
MODES = ["all", "third", "none", "fail"]


@pytest.fixture(scope="module")
def host():
    build.build_host()
    L = C.CDLL(build.HOST_LIB)
    L.fplh_gunzip_to_memory.restype = C.c_void_p
    L.fplh_gunzip_to_memory.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fplh_gunzip_release.argtypes = [C.c_void_p, C.c_uint64]
    L.fplh_set_gzip_inflater.argtypes = [CB, C.c_void_p, C.c_uint64]
    L.fplh_gzip_inflater_counts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.fplh_read_error.restype = C.c_int
    L.fplh_read_error.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.fplh_have_libdeflate.restype = C.c_int
    return L


_ends = {}


class Inflater:
    """a stand-in for fpl_inflate_gzip that knows the member: the block ends of its payload (gzip_cases.describe) and its text.  A
    window is inflated up to the last block that ends inside it.  The calls come in order, so it knows where it stands."""

    def __init__(self, mode, payload, text, tail=b""):
        self.mode, self.payload, self.text = mode, payload + tail, text  # (tail: what follows the payload in the file, the trailer)
        if payload not in _ends:  # (the reader is plain Python: once per stream)
            _ends[payload] = [(0, 0)] + gc.describe(payload)["ends"]
        self.ends = _ends[payload]
        self.bit, self.calls, self.refusals = 0, 0, 0
        self.cb = CB(self.call)

    def call(self, user, comp, comp_bytes, start_bit, zdict, dict_len, out, out_cap, chunk_bytes, res):
        self.calls += 1
        if self.mode == "fail":
            return -3
        r = np.ctypeslib.as_array(C.cast(res, C.POINTER(C.c_uint8)), (32,)).view(np.dtype([("out_bytes", "<u8"), ("end_bit", "<u8"), ("status", "<u4"),
                                                                                             ("crc32", "<u4"), ("final_block", "<u4"), ("chunks", "<u4")]))
        at = self.bit >> 3
        assert start_bit == self.bit & 7 and C.string_at(comp, comp_bytes) == self.payload[at:at + comp_bytes]
        made = dict(self.ends)[self.bit]
        assert C.string_at(zdict, dict_len) == self.text[:made][-32768:]
        inside = [(e, n) for e, n in self.ends if self.bit < e <= 8 * (at + comp_bytes)]
        if self.mode == "none" or (self.mode == "third" and self.calls % 3 == 0) or not inside or inside[-1][1] - made > out_cap:
            self.refusals += 1
            r["status"][0] = 1
            return 0
        end, upto = inside[-1]
        data = self.text[made:upto]
        C.memmove(out, data, len(data))
        r["out_bytes"][0], r["end_bit"][0], r["status"][0], r["crc32"][0] = len(data), end - 8 * at, 0, zlib.crc32(data)
        r["final_block"][0] = 1 if end == self.ends[-1][0] else 0
        self.bit = end
        return 0


def records():
    """about 300 KB of whole FASTQ records"""
    t = gc.text(300000, 1)
    return t[:t.rfind(b"\n@read") + 1]


def expand(L, path):
    n, reserved = C.c_uint64(), C.c_uint64()
    p = L.fplh_gunzip_to_memory(str(path).encode(), 4, 1 << 30, C.byref(n), C.byref(reserved))
    if not p:
        return None
    try:
        return C.string_at(p, n.value)
    finally:
        L.fplh_gunzip_release(p, reserved.value)


def counts(L):
    w, r = C.c_uint64(), C.c_uint64()
    L.fplh_gzip_inflater_counts(C.byref(w), C.byref(r))
    return w.value, r.value


def member(text, level=6, mem=4, name=None):
    payload = gc.raw(text, level, mem)
    head = b"\x1f\x8b\x08" + (b"\x08" if name else b"\x00") + b"\0\0\0\0\x00\x03" + (name + b"\0" if name else b"")
    return head + payload + zlib.crc32(text).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little"), payload, len(head)


def read_error(L, path):
    msg = C.create_string_buffer(512)
    return L.fplh_read_error(str(path).encode(), msg, 512), msg.value.decode()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [None, b"reads.fastq"])
def test_the_same_memory_whatever_the_inflater_does(host, tmp_path, mode, name):
    text = records()
    gz, payload, _ = member(text, name=name)
    path = tmp_path / "x.fastq.gz"
    path.write_bytes(gz)
    inf = Inflater(mode, payload, text, gz[-8:])
    host.fplh_set_gzip_inflater(inf.cb, None, WINDOW)
    try:
        got = expand(host, path)
    finally:
        host.fplh_set_gzip_inflater(C.cast(None, CB), None, 0)
    w, r = counts(host)
    assert got == text
    assert w == inf.calls
    if mode == "all":
        assert r == 0 and w > 4
    elif mode == "third":
        assert r == 1 and w == 3
    else:
        assert r == 1 and w == 1
    if host.fplh_have_libdeflate():  # (without the hook the lane needs libdeflate; with it, it does not)
        assert expand(host, path) == text
    assert counts(host) == (0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_damaged_files_are_the_host_s_to_report(host, tmp_path, mode):
    text = records()
    gz, payload, hl = member(text)
    bad_crc = bytearray(gz)
    bad_crc[-8] ^= 0x55
    files = {"truncated": gz[:len(gz) - 5000], "bad_crc": bytes(bad_crc)}
    for what, data in files.items():
        path = tmp_path / (what + ".fastq.gz")
        path.write_bytes(data)
        want_mem, want_err = expand(host, path), read_error(host, path)
        assert want_mem is None and want_err[0] == 1 and want_err[1], (what, want_err)
        inf = Inflater(mode, payload, text, data[hl + len(payload):])
        host.fplh_set_gzip_inflater(inf.cb, None, WINDOW)
        try:
            got_mem, got_err = expand(host, path), read_error(host, path)
        finally:
            host.fplh_set_gzip_inflater(C.cast(None, CB), None, 0)
        counts(host)
        assert got_mem is None and got_err == want_err, (what, got_err, want_err)
        assert inf.calls > 0 or what == "truncated"  # (a file cut short may not even look like one member: its last four bytes are no size)
