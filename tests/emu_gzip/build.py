"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_gzip/emu_gzip_run: the kernels of fastplong_amd/csrc/gzip_inflate.h on the host
(tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.  Jobs go in and come out as
a file:
    in:  u64 n_jobs; per job u64 comp_bytes, start_bit, dict_len, out_cap, chunk_bytes; comp; dict
    out: per job i64 rc (-1: the arguments were refused), fpl_gzip_window, and out[0 .. out_bytes) when rc and status are 0
Every buffer the kernels see is a heap block of exactly its promised size, so leaving one ends the run with a report."""
import os
import struct
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "emu_gzip_run")
SRCS = [os.path.join(HERE, "driver.cpp"), os.path.join(ROOT, "tests", "emu", "hip_emu.h")] + [
    os.path.join(ROOT, "fastplong_amd", "csrc", f) for f in ("gzip_inflate.h", "bgzf_inflate.h", "gz_emit.h", "dev_prims.h")
] + [os.path.join(ROOT, "include", "fastplong_amd.h")]


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in SRCS):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-DEMU_GZIP_MAIN", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"),
                               "-o", tmp, SRCS[0]])
        os.replace(tmp, EXE)
    return EXE


def start(jobs):
    """jobs: dicts with comp, start_bit, dict, out_cap, chunk_bytes -> a running sanitized process; finish() collects it"""
    exe = build()
    d = tempfile.mkdtemp(prefix="emu_gzip_")
    fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<Q", len(jobs)))
        for j in jobs:
            zd = j.get("dict") or b""
            f.write(struct.pack("<5Q", len(j["comp"]), j.get("start_bit", 0), len(zd), j["out_cap"], j.get("chunk_bytes", 0)))
            f.write(j["comp"])
            f.write(zd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env), d, len(jobs)


def finish(job):
    """-> a list of results (tests/gzip_cases.py Result fields as a dict); raises with the sanitizer's report when the run did not end clean"""
    p, d, n = job
    log = p.communicate()[0].decode(errors="replace")
    try:
        if p.returncode != 0:
            raise RuntimeError("emu_gzip_run ended with %d:\n%s" % (p.returncode, log[-4000:]))
        raw = open(os.path.join(d, "out"), "rb").read()
    finally:
        for f in ("in", "out"):
            try:
                os.unlink(os.path.join(d, f))
            except OSError:
                pass
        os.rmdir(d)
    res, at = [], 0
    for _ in range(n):
        rc, out_bytes, end_bit, status, crc, final, chunks = struct.unpack_from("<qQQIIII", raw, at)
        at += 40
        data = b""
        if rc == 0 and status == 0:
            data = raw[at:at + out_bytes]
            at += out_bytes
        res.append(dict(rc=rc, status=status, out_bytes=out_bytes, end_bit=end_bit, crc32=crc, final=final, chunks=chunks, data=data))
    assert at == len(raw)
    return res


def inflate(jobs):
    return finish(start(jobs))
