"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_emit/libfpl_emu_emit.so: the emit kernels on the host (tests/emu/hip_emu.h)."""
import ctypes as C
import os

import numpy as np

from fastplong_amd import abi
from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfpl_emu_emit.so")


def build():
    return cbuild.emu_lib(LIB, "tests/emu_emit/driver.cpp", __file__)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_emit.restype = C.c_int
        _lib.emu_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        for f in ("emu_emit_layout_reads", "emu_emit_scan_blocks", "emu_emit_tile", "emu_emit_step"):
            getattr(_lib, f).restype = C.c_uint32
    return _lib


def layout_reads():
    """fpl::EM_LAYOUT_READS: reads per block of the layout"""
    return int(lib().emu_emit_layout_reads())


def scan_blocks():
    """fpl::EM_SCAN_BLOCKS: block sums the scan block takes per step"""
    return int(lib().emu_emit_scan_blocks())


def tile():
    """fpl::EM_TILE: output bytes per tile of the gather"""
    return int(lib().emu_emit_tile())


def step():
    return int(lib().emu_emit_step())


def _ptr(a):
    return a.ctypes.data if a is not None else None


def emit(seq, qual, off, res, seq_out, qual_out, cap_bytes, off_out, cap_reads, src, kind, gather_blocks=3):
    """the four kernels over numpy arrays, the arguments of fpl_emit_batch_device (outputs are written in place; any may be None)
    -> (rc, info as a dict)"""
    info = np.zeros(1, np.dtype(abi.EMIT_INFO_DTYPE))
    n = max(len(off) - 1, 0) if off is not None else 0
    rc = lib().emu_emit(_ptr(seq), _ptr(qual), _ptr(off), n, _ptr(res), _ptr(seq_out), _ptr(qual_out), int(cap_bytes), _ptr(off_out),
                        int(cap_reads), _ptr(src), _ptr(kind), info.ctypes.data, int(gather_blocks))
    r = info[0]
    return rc, dict(n_bytes=int(r["n_bytes"]), n_out=int(r["n_out"]), max_len=int(r["max_len"]), status=int(r["status"]))
