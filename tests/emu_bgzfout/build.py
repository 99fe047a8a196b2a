"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bgzfout/emu_bgzfout_run: the gzip kernels (fastplong_amd/csrc/gz_emit.h) in both
framings on the host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (a
sanitized shared object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file (driver.cpp)."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "emu_bgzfout_run")
SRCS = [os.path.join(HERE, "driver.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "gz_emit.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "dev_prims.h"),
        os.path.join(ROOT, "include", "fastplong_amd.h")]
STRIPE = 49152     # fpl::GZ_STRIPE
BGZF_EXTRA = 31    # fpl::GZ_BGZF_EXTRA
MEMBER_EXTRA = 23  # fpl::GZ_MEMBER_EXTRA


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in SRCS):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"), "-o", tmp, SRCS[0]])
        os.replace(tmp, EXE)
    return EXE


def start(text, results, bgzf):
    """start one sanitized run over a chunk of regular FASTQ text and its per-read records (abi.RESULT_DTYPE); finish() collects it"""
    exe = build()
    t = bytes(text)
    r = np.ascontiguousarray(results)
    n_rec = r.nbytes // 36
    d = tempfile.mkdtemp(prefix="emu_bgzfout_")
    fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
    with open(fin, "wb") as f:
        f.write(np.array([len(t), n_rec, 1 if bgzf else 0], np.uint64).tobytes())
        f.write(t)
        f.write(r.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env), d


def finish(job):
    """-> (bytes, info dict); raises with the sanitizer's report when the run did not end clean"""
    p, d = job
    log = p.communicate()[0].decode(errors="replace")
    try:
        if p.returncode != 0:
            raise RuntimeError("emu_bgzfout_run ended with %d:\n%s" % (p.returncode, log[-4000:]))
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
    out = raw[40:]
    assert len(out) == inf["gz_len"]
    return out, inf


def emit(text, results, bgzf):
    return finish(start(text, results, bgzf))
