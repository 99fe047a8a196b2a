"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_gz/libfpl_emu_gz.so: the gzip kernels on the host (tests/emu/hip_emu.h)."""
import ctypes as C
import os

import numpy as np

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfpl_emu_gz.so")
MEMBER_EXTRA = 23  # fpl::GZ_MEMBER_EXTRA
SLACK = 5          # fpl::GZ_SLACK


def build():
    return cbuild.emu_lib(LIB, "tests/emu_gz/driver.cpp", __file__)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_gz_emit.restype = C.c_int
        _lib.emu_gz_emit.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        _lib.emu_gz_deflate.restype = C.c_int
        _lib.emu_gz_deflate.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        for f in ("emu_gz_block_bytes", "emu_gz_long_line", "emu_gz_stretch"):
            getattr(_lib, f).restype = C.c_uint32
    return _lib


def block_bytes():
    return int(lib().emu_gz_block_bytes())


def long_line():
    return int(lib().emu_gz_long_line())


def stretch():
    return int(lib().emu_gz_stretch())


def bound(total, n_blocks):
    """the worst-case size of the member the buffers are sized by (gz_emit.h)"""
    return MEMBER_EXTRA + total + SLACK * n_blocks


def emit(text, results, want_composed=False):
    """the kernels over a chunk of regular FASTQ text and its per-read records (a numpy array of abi.RESULT_DTYPE or raw bytes of
    36 per read) -> (gzip bytes, info dict[, composed text])"""
    L = lib()
    t = np.frombuffer(bytes(text), np.uint8)
    r = np.ascontiguousarray(results)
    n_rec = r.nbytes // 36
    info = np.zeros(4, np.uint64)
    cap = 2 * len(t) + 64 * n_rec + 4096
    out = np.zeros(cap, np.uint8)
    comp = np.zeros(cap, np.uint8) if want_composed else None
    rc = L.emu_gz_emit(t.ctypes.data if len(t) else None, len(t), r.ctypes.data if n_rec else None, n_rec, out.ctypes.data, cap,
                       info.ctypes.data, comp.ctypes.data if want_composed else None)
    if rc != 0:
        raise RuntimeError("emu_gz_emit: %d" % rc)
    d = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]))
    gz = out[:d["gz_len"]].tobytes()
    if want_composed:
        return gz, d, comp[:d["total"]].tobytes()
    return gz, d


def deflate(data):
    """k_gz_block / k_gz_finish / k_gz_compact alone over any bytes -> (gzip bytes, info dict)"""
    L = lib()
    t = np.frombuffer(bytes(data), np.uint8)
    info = np.zeros(4, np.uint64)
    cap = len(t) + len(t) // 1024 + 4096
    out = np.zeros(cap, np.uint8)
    rc = L.emu_gz_deflate(t.ctypes.data if len(t) else None, len(t), out.ctypes.data, cap, info.ctypes.data)
    if rc != 0:
        raise RuntimeError("emu_gz_deflate: %d" % rc)
    d = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]))
    return out[:d["gz_len"]].tobytes(), d
