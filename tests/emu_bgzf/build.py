"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bgzf/emu_bgzf_run: the BGZF inflate kernel (fastplong_amd/csrc/bgzf_inflate.h) on the
host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (a sanitized shared
object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file:
    in:  u64 comp_bytes, out_bytes, n_blocks, grid (0: the driver picks); n_blocks x fpl_bgzf_block; comp; the initial out
    out: n_blocks x fpl_bgzf_block (status filled in); out
The program poisons every byte of comp and out no descriptor covers, so a kernel that leaves its ranges dies with a report."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "emu_bgzf_run")
SRCS = [os.path.join(HERE, "driver.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "bgzf_inflate.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "gz_emit.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "dev_prims.h"), os.path.join(ROOT, "include", "fastplong_amd.h")]
BLOCK_DTYPE = [("comp_off", "<u8"), ("out_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("status", "<u4")]


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in SRCS):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-DEMU_BGZF_MAIN", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-o", tmp, SRCS[0]])
        os.replace(tmp, EXE)
    return EXE


def start(comp, blocks, out, grid=0):
    """start one sanitized run; finish() collects it"""
    exe = build()
    comp = np.ascontiguousarray(comp, np.uint8)
    out = np.ascontiguousarray(out, np.uint8)
    blocks = np.ascontiguousarray(blocks, np.dtype(BLOCK_DTYPE))
    d = tempfile.mkdtemp(prefix="emu_bgzf_")
    fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
    with open(fin, "wb") as f:
        f.write(np.array([len(comp), len(out), len(blocks), grid], np.uint64).tobytes())
        f.write(blocks.tobytes())
        f.write(comp.tobytes())
        f.write(out.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env)
    return p, d, len(blocks), len(out)


def finish(job):
    """-> (out, blocks with status); raises with the sanitizer's report when the run did not end clean"""
    p, d, n, n_out = job
    log = p.communicate()[0].decode(errors="replace")
    try:
        if p.returncode != 0:
            raise RuntimeError("emu_bgzf_run ended with %d:\n%s" % (p.returncode, log[-4000:]))
        raw = open(os.path.join(d, "out"), "rb").read()
    finally:
        for f in ("in", "out"):
            try:
                os.unlink(os.path.join(d, f))
            except OSError:
                pass
        os.rmdir(d)
    blocks = np.frombuffer(raw[:32 * n], np.dtype(BLOCK_DTYPE)).copy()
    out = np.frombuffer(raw[32 * n:], np.uint8).copy()
    assert len(out) == n_out
    return out, blocks


def inflate(comp, blocks, out, grid=0):
    return finish(start(comp, blocks, out, grid))
