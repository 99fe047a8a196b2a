"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bam/libfpl_emu_bam.so: the BAM decode kernel on the host (tests/emu/hip_emu.h)."""
import ctypes as C
import os

import numpy as np

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfpl_emu_bam.so")
PAD = 64  # fpl::BAM_PAD


def build():
    return cbuild.emu_lib(LIB, "tests/emu_bam/driver.cpp", __file__)


_lib = None


def decode(raw, rec_start, off):
    """the kernel over an uncompressed record stream: (bases, qualities) of off[-1] bytes"""
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_bam_decode.restype = C.c_int
        _lib.emu_bam_decode.argtypes = [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 2
    buf = np.zeros(len(raw) + PAD, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    rec_start = np.ascontiguousarray(rec_start, np.uint64)
    off = np.ascontiguousarray(off, np.uint64)
    total = int(off[-1])
    seq = np.zeros((total + 15) // 16 * 16 + 16, np.uint8)
    qual = np.zeros_like(seq)
    _lib.emu_bam_decode(buf.ctypes.data, rec_start.ctypes.data, off.ctypes.data, len(off) - 1, seq.ctypes.data, qual.ctypes.data)
    return seq[:total], qual[:total]
