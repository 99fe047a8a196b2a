"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bamcomments/emu_bamcomments_run: the kernel chain of fpl_set_bam_comments
(fastplong_amd/csrc/bam_comments.h) with the block kernels of either framing behind it on the host (tests/emu/hip_emu.h), with
AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (a sanitized shared object cannot be loaded into an
unsanitized Python).  A job goes in and comes out as a file (driver.cpp)."""
import os

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bamcomments_run")


def build():
    return cbuild.emu_program(EXE, "tests/emu_bamcomments/driver.cpp", __file__)


def start(raw, rec_start, off, results, tags=b"", n_tags=0, bgzf=False, fragment_mode=False):
    """start one sanitized run over an uncompressed BAM record stream, the starts of the records that are not skipped, the CSR
    offsets of their bases, their per-read records (abi.RESULT_DTYPE) and a selection (n_tags 0: off, -1: every field); finish()
    collects it"""
    r = np.ascontiguousarray(results)
    n_rec = len(off) - 1
    assert r.nbytes == 36 * n_rec and len(rec_start) == n_rec and len(tags) <= 64
    parts = [np.array([len(raw), n_rec, int(fragment_mode), int(bgzf), n_tags % (1 << 64)], np.uint64).tobytes(), bytes(tags).ljust(64, b"\0"), bytes(raw),
             np.ascontiguousarray(rec_start, np.uint64).tobytes(), np.ascontiguousarray(off, np.uint64).tobytes(), r.tobytes()]
    return emujob.start(build(), lambda f: f.write(b"".join(parts)), "emu_bamcomments_")


def finish(job):
    """-> (member or BGZF bytes, composed text, info dict); raises with the sanitizer's report when the run did not end clean"""
    raw = emujob.finish(job, timeout=900)
    head = np.frombuffer(raw[:80], np.uint64)
    inf = dict(total=int(head[0]), gz_len=int(head[1]), n_blocks=int(head[2]), crc=int(head[3]), out_cap=int(head[4]), blk_cap=int(head[5]),
               stats=[int(v) for v in head[6:10]])
    comp = raw[80:80 + inf["total"]]
    out = raw[80 + inf["total"]:]
    assert len(out) == inf["gz_len"]
    return out, comp, inf
