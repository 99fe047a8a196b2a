"""TEST INFRASTRUCTURE ONLY -- builds and drives tests/emu/libfpl_emu.so: the product kernels
compiled for the host on a lock-step thread emulator (hip_emu.h)."""
import ctypes as C
import os

import numpy as np

from fastplong_amd import abi
from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfpl_emu.so")


def build():
    return cbuild.emu_lib(LIB, "tests/emu/emu_driver.cpp", __file__)


LIB_TRIM_STATS = os.path.join(HERE, "libfpl_emu_trimstats.so")
_lib = None
_libs = {}


def use_trim_stats(on):
    """switch process_batch to the build with the FPL_EMU_TRIM_STATS counters of kernels.h (a second cached library; it also
    prints them per batch) and back"""
    global _lib
    _lib = None
    _libs["want"] = LIB_TRIM_STATS if on else LIB


TRIM_STATS = ("groups", "p1b", "p2", "p3_wants", "p3_may", "p6", "p7_wants", "p7_may", "searches", "rounds")


def trim_stats(full=False):
    """-> (groups of 64 reads k_trim_ends_batched took, reads it handed to its wave-per-read fallback) since the last call; full: all
    ten counters, in the order of TRIM_STATS (emu_trim_stats in emu_driver.cpp says what each counts)"""
    out = (C.c_ulonglong * 10)()
    assert lib().emu_trim_stats(out) == 0, "a counter is no multiple of 64 lanes"
    return tuple(int(v) for v in out) if full else (int(out[0]), int(out[1]))


def lib():
    global _lib
    if _lib is None:
        path = _libs.get("want", LIB)
        if path in _libs:
            _lib = _libs[path]
            return _lib
        if path == LIB:
            build()
        else:
            cbuild.emu_lib(path, "tests/emu/emu_driver.cpp", __file__, defines=["FPL_EMU_TRIM_STATS"])
        L = _libs[path] = C.CDLL(path)
        L.emu_process_batch.restype = C.c_int
        L.emu_process_batch.argtypes = [C.POINTER(abi.FplOptions), C.c_char_p, C.c_int, C.c_char_p, C.c_int,
                                        C.POINTER(abi.FplAdapter), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.emu_lev_bp64.restype = C.c_int
        L.emu_lev_bp64.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.emu_lev_wave.restype = C.c_int
        L.emu_lev_wave.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int]
        for f in (L.emu_lev_bp32_start, L.emu_lev_bp32_end):
            f.restype = C.c_int
            f.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        _lib = L
    return _lib


def process_batch(cfg, seq, qual, off, max_cycles, n_cu=2, with_fragments=False):
    """cfg: oracle.Config-like object with .opt, .start, .end, .fasta (bytes)."""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    qual = np.ascontiguousarray(qual, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    # at least one addressable byte so the pointers are never NULL
    if seq.size == 0:
        seq = np.zeros(1, np.uint8)
        qual = np.zeros(1, np.uint8)
    nad = 2 + len(cfg.fasta)
    counters = np.zeros(abi.counters_len(max_cycles, nad), dtype=np.int64)
    res = np.zeros(max(n, 1), dtype=abi.RESULT_DTYPE)
    arr = (abi.FplAdapter * max(1, len(cfg.fasta)))()
    for i, a in enumerate(cfg.fasta):
        arr[i].seq, arr[i].len = a, len(a)
    rc = lib().emu_process_batch(C.byref(cfg.opt), cfg.start, len(cfg.start), cfg.end, len(cfg.end), arr,
                                 len(cfg.fasta), seq.ctypes.data, qual.ctypes.data, off.ctypes.data, n,
                                 counters.ctypes.data, max_cycles, res.ctypes.data, n_cu)
    if rc != 0:
        raise RuntimeError("emu_process_batch rc=%d" % rc)
    if with_fragments:
        L = lib()
        L.emu_fragment_count.restype = C.c_uint32
        L.emu_region_count.restype = C.c_uint32
        nf, nr = L.emu_fragment_count(), L.emu_region_count()
        frags = np.zeros(max(nf, 1), dtype=abi.FRAGMENT_DTYPE)
        regs = np.zeros(max(nr, 1), dtype=abi.REGION_DTYPE)
        L.emu_get_fragments(C.c_void_p(frags.ctypes.data), C.c_void_p(regs.ctypes.data))
        return res[:n], counters, frags[:nf], regs[:nr]
    return res[:n], counters
