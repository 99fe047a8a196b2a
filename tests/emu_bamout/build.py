"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bamout/emu_bamout_run: the BAM record kernels (fastplong_amd/csrc/bam_emit.h) and the
BGZF block kernels behind them on the host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a
program of its own (a sanitized shared object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file
(driver.cpp)."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "emu_bamout_run")
CSRC = os.path.join(ROOT, "fastplong_amd", "csrc")
SRCS = [os.path.join(HERE, "driver.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"), os.path.join(CSRC, "bam_emit.h"),
        os.path.join(CSRC, "bam_out_rules.h"), os.path.join(CSRC, "gz_emit.h"), os.path.join(CSRC, "bam_decode.h"),
        os.path.join(CSRC, "dev_prims.h"), os.path.join(ROOT, "include", "fastplong_amd.h")]


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in SRCS):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"), "-o", tmp, SRCS[0]])
        os.replace(tmp, EXE)
    return EXE


def _start(head, parts):
    exe = build()
    d = tempfile.mkdtemp(prefix="emu_bamout_")
    fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
    with open(fin, "wb") as f:
        f.write(np.array(head, np.uint64).tobytes())
        for p in parts:
            f.write(p)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env), d


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
    p, d = job
    log = p.communicate()[0].decode(errors="replace")
    try:
        if p.returncode != 0:
            raise RuntimeError("emu_bamout_run ended with %d:\n%s" % (p.returncode, log[-4000:]))
        raw = open(os.path.join(d, "out"), "rb").read()
    finally:
        for f in ("in", "out"):
            try:
                os.unlink(os.path.join(d, f))
            except OSError:
                pass
        os.rmdir(d)
    info = np.frombuffer(raw[:40], np.uint64)
    inf = dict(total=int(info[0]), gz_len=int(info[1]), n_blocks=int(info[2]), crc=int(info[3]), out_cap=int(info[4]))
    comp = raw[40:40 + inf["total"]]
    out = raw[40 + inf["total"]:]
    assert len(out) == inf["gz_len"]
    return out, comp, inf
