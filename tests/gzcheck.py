"""Test helpers shared by the gzip tests (tests/test_gz_emit_emu.py, tests/test_gpu_gz.py): the host's formatter through ctypes,
every inflater at hand, and the golden cases that go through the per-read record path."""
import ctypes as C
import ctypes.util
import gzip
import os
import zlib

import numpy as np

from fastplong_amd import build, synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (c3_break_mask is left out on purpose: --break / --mask output comes from fragment lists, never from a text batch, and keeps
#  the host's deflate -- tests/test_cli_gz_stub.py pins that)
GOLDEN_OPTS = {
    "c1_qualfilter": (dict(adapter_enabled=0), "auto", "auto"),
    "c3_full": (dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1),
                synth.START_ADAPTER, synth.END_ADAPTER),
    "c5_fasta": (dict(ed_max=0.3, trimming_extension=5, required_length=30, n_base_percent_limit=5, avg_qual_req=12),
                 synth.START_ADAPTER, synth.revcomp(synth.START_ADAPTER)),
}


def gz(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def parse_fastq(text):
    lines = text.split(b"\n")
    names, strands, seqs, quals = [], [], [], []
    for i in range(0, len(lines) - 1, 4):
        names.append(lines[i])
        seqs.append(np.frombuffer(lines[i + 1], np.uint8))
        strands.append(lines[i + 2])
        quals.append(np.frombuffer(lines[i + 3], np.uint8))
    seq, qual, off = synth.pack(list(zip(seqs, quals)))
    return seq, qual, off, names, strands


def fasta_list(case):
    p = os.path.join(GOLD, case, "ADAPTERS.fa")
    if not os.path.exists(p):
        return []
    recs, name = {}, None
    for line in open(p):
        line = line.rstrip("\n")
        if line.startswith(">"):
            name = line[1:]
            recs[name] = ""
        else:
            recs[name] += line
    return [recs[k].upper() for k in sorted(recs) if len(recs[k]) >= 6]


def load_hostlib():
    build.build_host()
    L = C.CDLL(build.HOST_LIB)
    L.fplh_batch_read.restype = C.c_void_p
    L.fplh_batch_read.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32]
    L.fplh_batch_n.restype = C.c_uint32
    L.fplh_batch_n.argtypes = [C.c_void_p]
    L.fplh_batch_free.argtypes = [C.c_void_p]
    L.fplh_format_batch.restype = C.c_int
    L.fplh_format_batch.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.fplh_free.argtypes = [C.c_void_p]
    return L


def _libdeflate():
    for name in ("libdeflate.so.0", ctypes.util.find_library("deflate")):
        if not name:
            continue
        try:
            L = C.CDLL(name)
        except OSError:
            continue
        L.libdeflate_alloc_decompressor.restype = C.c_void_p
        L.libdeflate_gzip_decompress.restype = C.c_int
        L.libdeflate_gzip_decompress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.libdeflate_free_decompressor.argtypes = [C.c_void_p]
        return L
    return None


def inflate_all(data, want_len):
    """every inflater at hand over one gzip member; they must agree"""
    outs = [gzip.decompress(data)]
    d = zlib.decompressobj(31)
    outs.append(d.decompress(data) + d.flush())
    assert d.eof and d.unused_data == b""
    L = _libdeflate()
    if L is not None:
        dec = L.libdeflate_alloc_decompressor()
        buf = C.create_string_buffer(max(want_len, 1))
        n = C.c_size_t(0)
        rc = L.libdeflate_gzip_decompress(dec, data, len(data), buf, want_len, C.byref(n))
        L.libdeflate_free_decompressor(dec)
        assert rc == 0, "libdeflate refuses the member: %d" % rc
        outs.append(buf.raw[:n.value])
    assert all(o == outs[0] for o in outs)
    return outs[0]


def host_format(L, tmp_path, text, res):
    p = tmp_path / "in.fq"
    p.write_bytes(text)
    b = L.fplh_batch_read(str(p).encode(), 2 ** 62, 2 ** 30)
    assert b and L.fplh_batch_n(b) == len(res)
    out, n = C.c_void_p(), C.c_uint64()
    res = np.ascontiguousarray(res)
    assert L.fplh_format_batch(b, res.ctypes.data, C.byref(out), C.byref(n), None, None) == 0
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    L.fplh_batch_free(b)
    return s
