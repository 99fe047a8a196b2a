"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bgzfout/emu_bgzfout_run: the gzip kernels (fastplong_amd/csrc/gz_emit.h) in both
framings on the host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (a
sanitized shared object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file (driver.cpp)."""
import os

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bgzfout_run")
STRIPE = 49152     # fpl::GZ_STRIPE
BGZF_EXTRA = 31    # fpl::GZ_BGZF_EXTRA
MEMBER_EXTRA = 23  # fpl::GZ_MEMBER_EXTRA


def build():
    return cbuild.emu_program(EXE, "tests/emu_bgzfout/driver.cpp", __file__)


def start(text, results, bgzf):
    """start one sanitized run over a chunk of regular FASTQ text and its per-read records (abi.RESULT_DTYPE); finish() collects it"""
    t = bytes(text)
    r = np.ascontiguousarray(results)
    head = np.array([len(t), r.nbytes // 36, 1 if bgzf else 0], np.uint64).tobytes()
    return emujob.start(build(), lambda f: f.write(head + t + r.tobytes()), "emu_bgzfout_")


def finish(job):
    """-> (bytes, info dict); raises with the sanitizer's report when the run did not end clean"""
    raw = emujob.finish(job)
    info = np.frombuffer(raw[:40], np.uint64)
    inf = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]), out_cap=int(info[4]))
    out = raw[40:]
    assert len(out) == inf["gz_len"]
    return out, inf


def emit(text, results, bgzf):
    return finish(start(text, results, bgzf))
