"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bam/libfastplong_amd.so -- the CPU stand-in of tests/stub (fpl_stub.cpp and the
oracle, unchanged) plus the two BAM entry points of bam_stand_in.cpp.  Loaded by the CLI only through LD_LIBRARY_PATH in tests."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libfastplong_amd.so")
SRCS = [os.path.join(ROOT, "tests", "stub", "fpl_stub.cpp"), os.path.join(ROOT, "oracle", "fpl_oracle.c"), os.path.join(HERE, "bam_stand_in.cpp"),
        os.path.join(ROOT, "oracle", "fpl_oracle.h"), os.path.join(ROOT, "include", "fastplong_amd.h"),
        os.path.join(ROOT, "tests", "stub", "text_stand_in.h")]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        obj = os.path.join(HERE, "fpl_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", "-o", obj, SRCS[1]])
        tmp = "%s.tmp.%d" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, SRCS[0], SRCS[2], obj, "-lm"])
        os.replace(tmp, LIB)
    return LIB
