"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bamout/emu_bamout_run: the BAM record kernels (fastplong_amd/csrc/bam_emit.h) and the
BGZF block kernels behind them on the host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a
program of its own (a sanitized shared object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file
(driver.cpp)."""
import os

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bamout_run")


def build():
    return cbuild.emu_program(EXE, "tests/emu_bamout/driver.cpp", __file__)


def _start(head, parts):
    return emujob.start(build(), lambda f: f.write(np.array(head, np.uint64).tobytes() + b"".join(parts)), "emu_bamout_")


def start_text(text, results):
    """start one sanitized run over a chunk of regular FASTQ text and its per-read records (abi.RESULT_DTYPE); finish() collects it"""
    r = np.ascontiguousarray(results)
    return _start([0, len(text), r.nbytes // 36], [bytes(text), r.tobytes()])


def start_bam(raw, rec_start, off, results):
    """the same over an uncompressed BAM record stream, its records' starts and the CSR offsets of their bases"""
    r = np.ascontiguousarray(results)
    n_rec = len(off) - 1
    assert r.nbytes == 36 * n_rec and len(rec_start) == n_rec
    return _start([1, len(raw), n_rec], [bytes(raw), np.ascontiguousarray(rec_start, np.uint64).tobytes(),
                                         np.ascontiguousarray(off, np.uint64).tobytes(), r.tobytes()])


def finish(job):
    """-> (BGZF bytes, composed record bytes, info dict); raises with the sanitizer's report when the run did not end clean"""
    raw = emujob.finish(job)
    info = np.frombuffer(raw[:40], np.uint64)
    inf = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]), out_cap=int(info[4]))
    comp = raw[40:40 + inf["total"]]
    out = raw[40 + inf["total"]:]
    assert len(out) == inf["gz_len"]
    return out, comp, inf
