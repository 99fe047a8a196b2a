"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_gzip/emu_gzip_run: the kernels of fastplong_amd/csrc/gzip_inflate.h on the host
(tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.  Jobs go in and come out as
a file:
    in:  u64 n_jobs; per job u64 comp_bytes, start_bit, dict_len, out_cap, chunk_bytes; comp; dict
    out: per job i64 rc (-1: the arguments were refused), fpl_gzip_window, and out[0 .. out_bytes) when rc and status are 0
Every buffer the kernels see is a heap block of exactly its promised size, so leaving one ends the run with a report."""
import os
import struct

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_gzip_run")


def build():
    return cbuild.emu_program(EXE, "tests/emu_gzip/driver.cpp", __file__, main="EMU_GZIP_MAIN")


def start(jobs):
    """jobs: dicts with comp, start_bit, dict, out_cap, chunk_bytes -> a running sanitized process; finish() collects it"""
    def payload(f):
        f.write(struct.pack("<Q", len(jobs)))
        for j in jobs:
            zd = j.get("dict") or b""
            f.write(struct.pack("<5Q", len(j["comp"]), j.get("start_bit", 0), len(zd), j["out_cap"], j.get("chunk_bytes", 0)))
            f.write(j["comp"])
            f.write(zd)

    return emujob.start(build(), payload, "emu_gzip_"), len(jobs)


def finish(job):
    """-> a list of results (tests/gzip_cases.py Result fields as a dict); raises with the sanitizer's report when the run did not end clean"""
    run, n = job
    raw = emujob.finish(run)
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
