"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bamout/libfastplong_amd.so -- the CPU stand-in of tests/stub (fpl_stub.cpp and the
oracle, unchanged) plus the gzip entry points, fpl_set_gzip_framing and fpl_set_gzip_records of bamout_stand_in.cpp (the host's formatter, a few lines that build records, zlib).
Loaded by the CLI only through LD_LIBRARY_PATH in tests."""
import os
import subprocess

from fastplong_amd import build as fbuild

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libfastplong_amd.so")
SRCS = [os.path.join(HERE, "bamout_stand_in.cpp"), os.path.join(ROOT, "oracle", "fpl_oracle.c"), os.path.join(ROOT, "tests", "stub", "fpl_stub.cpp"),
        os.path.join(ROOT, "oracle", "fpl_oracle.h"), os.path.join(ROOT, "include", "fastplong_amd.h"),
        os.path.join(ROOT, "tests", "stub", "text_stand_in.h"), os.path.join(ROOT, "fastplong_amd", "host", "fastq.h")]


def build():
    host = fbuild.build_host()
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS + [host]):
        obj = os.path.join(HERE, "fpl_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", "-o", obj, SRCS[1]])
        tmp = "%s.tmp.%d" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", tmp, SRCS[0], obj,
                               "-L" + os.path.dirname(host), "-lfastplong_host", "-Wl,-rpath," + os.path.dirname(host), "-lz", "-lm"])
        os.replace(tmp, LIB)
    return LIB
