"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bamgz/libfpl_emu_bamgz.so: the BAM decode kernel, the BAM forms of the gzip layout and
compose kernels and the block kernels on the host (tests/emu/hip_emu.h)."""
import ctypes as C
import os

import numpy as np

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfpl_emu_bamgz.so")
MEMBER_EXTRA = 23  # fpl::GZ_MEMBER_EXTRA
SLACK = 5          # fpl::GZ_SLACK


def build():
    return cbuild.emu_lib(LIB, "tests/emu_bamgz/driver.cpp", __file__)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_bamgz_emit.restype = C.c_int
        _lib.emu_bamgz_emit.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64]
        for f in ("emu_bamgz_block_bytes", "emu_bamgz_long_line", "emu_bamgz_pad"):
            getattr(_lib, f).restype = C.c_uint32
    return _lib


def block_bytes():
    return int(lib().emu_bamgz_block_bytes())


def long_line():
    return int(lib().emu_bamgz_long_line())


def bound(total, n_blocks):
    """the worst-case size of the member the buffers are sized by (gz_emit.h)"""
    return MEMBER_EXTRA + total + SLACK * n_blocks


def emit(raw, rec_start, off, results):
    """the kernels over an uncompressed BAM record stream, the byte offsets of its records, the CSR offsets of their bases and the
    per-read records (a numpy array of abi.RESULT_DTYPE) -> (gzip bytes, info dict, composed text, block starts)"""
    L = lib()
    buf = np.zeros(len(raw) + int(L.emu_bamgz_pad()), np.uint8)
    buf[:len(raw)] = np.frombuffer(bytes(raw), np.uint8)
    rec_start = np.ascontiguousarray(rec_start, np.uint64)
    off = np.ascontiguousarray(off, np.uint64)
    r = np.ascontiguousarray(results)
    n_rec = len(off) - 1
    assert r.nbytes == 36 * n_rec and len(rec_start) == n_rec
    info = np.zeros(4, np.uint64)
    cap = 4 * int(off[-1]) + 600 * n_rec + 4096
    out = np.zeros(cap, np.uint8)
    comp = np.zeros(cap, np.uint8)
    blk_cap = cap // 1024 + 4 * n_rec + 8
    blk = np.zeros(blk_cap, np.uint64)
    rc = L.emu_bamgz_emit(buf.ctypes.data, rec_start.ctypes.data if n_rec else None, off.ctypes.data, r.ctypes.data if n_rec else None,
                          n_rec, out.ctypes.data, cap, info.ctypes.data, comp.ctypes.data, blk.ctypes.data, blk_cap)
    if rc != 0:
        raise RuntimeError("emu_bamgz_emit: %d" % rc)
    d = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]))
    return out[:d["gz_len"]].tobytes(), d, comp[:d["total"]].tobytes(), [int(x) for x in blk[:d["n_blocks"] + 1]]
