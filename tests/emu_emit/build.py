"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_emit/libfpl_emu_emit.so: the emit kernels on the host (tests/emu/hip_emu.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

from fastplong_amd import abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libfpl_emu_emit.so")
SRCS = [os.path.join(HERE, "driver.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "emit.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "dev_prims.h"),
        os.path.join(ROOT, "include", "fastplong_amd.h")]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        tmp = "%s.tmp.%d" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fPIC", "-shared", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-o", tmp, SRCS[0]])
        os.replace(tmp, LIB)
    return LIB


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
