"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bammoves/emu_bammoves_run: the --keep_moves kernels (fastplong_amd/csrc/bam_moves.h), with
--keep_mods' plan kernel between them where a job asks for it, around the tagged layout kernel, with the BGZF block kernels behind them on the host (tests/emu/hip_emu.h), with AddressSanitizer and
UndefinedBehaviorSanitizer, as a program of its own (a sanitized shared object cannot be loaded into an unsanitized Python).  A job
goes in and comes out as a file (driver.cpp)."""
import os

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bammoves_run")


def build():
    return cbuild.emu_program(EXE, "tests/emu_bammoves/driver.cpp", __file__)


def start(raw, rec_start, off, results, fragment_mode=False, mods=False):
    """start one sanitized run over an uncompressed BAM record stream, the starts of the records that are not skipped, the CSR
    offsets of their bases and their per-read records (abi.RESULT_DTYPE); mods: --keep_mods beside the switch; finish() collects it"""
    r = np.ascontiguousarray(results)
    n_rec = len(off) - 1
    assert r.nbytes == 36 * n_rec and len(rec_start) == n_rec
    parts = [np.array([len(raw), n_rec, int(fragment_mode), int(mods)], np.uint64).tobytes(), bytes(raw), np.ascontiguousarray(rec_start, np.uint64).tobytes(),
             np.ascontiguousarray(off, np.uint64).tobytes(), r.tobytes()]
    return emujob.start(build(), lambda f: f.write(b"".join(parts)), "emu_bammoves_")


def finish(job):
    """-> (BGZF bytes, composed record bytes, info dict); raises with the sanitizer's report when the run did not end clean"""
    raw = emujob.finish(job, timeout=600)
    head = np.frombuffer(raw[:136], np.uint64)
    inf = dict(total=int(head[0]), gz_len=int(head[1]), n_blocks=int(head[2]), crc=int(head[3]), out_cap=int(head[4]),
               stats=[int(v) for v in head[5:9]], mod_stats=[int(v) for v in head[9:13]], move_stats=[int(v) for v in head[13:17]])
    comp = raw[136:136 + inf["total"]]
    out = raw[136 + inf["total"]:]
    assert len(out) == inf["gz_len"]
    return out, comp, inf
