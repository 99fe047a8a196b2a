"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bgzf/libfastplong_amd.so -- the stand-in of tests/stub_bamgz (unchanged) plus the
three inflater calls of bgzf_stand_in.cpp, whose blocks are inflated by the product's kernel on the emulator
(tests/emu_bgzf/driver.cpp, here without sanitizers: the CLI that loads the library is not sanitized).  Loaded by the CLI only
through LD_LIBRARY_PATH in tests."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libfastplong_amd.so")
SRCS = [os.path.join(HERE, "bgzf_stand_in.cpp"), os.path.join(HERE, "emu_kernels.cpp"), os.path.join(ROOT, "oracle", "fpl_oracle.c"), os.path.join(ROOT, "tests", "emu_bamgz", "driver.cpp"),
        os.path.join(ROOT, "tests", "emu_bgzf", "driver.cpp"), os.path.join(ROOT, "tests", "stub_bamgz", "bamgz_stand_in.cpp"),
        os.path.join(ROOT, "tests", "stub", "fpl_stub.cpp"), os.path.join(ROOT, "oracle", "fpl_oracle.h"), os.path.join(ROOT, "include", "fastplong_amd.h"),
        os.path.join(ROOT, "tests", "stub", "text_stand_in.h"), os.path.join(ROOT, "tests", "emu", "hip_emu.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "gz_emit.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "bam_decode.h"),
        os.path.join(ROOT, "fastplong_amd", "csrc", "bgzf_inflate.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "dev_prims.h")]


def build():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SRCS):
        obj = os.path.join(HERE, "fpl_oracle.o")
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-c", "-o", obj, SRCS[2]])
        objs = [os.path.join(HERE, "emu_kernels.o")]
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-fPIC", "-pthread", "-I" + os.path.join(ROOT, "tests", "emu"), "-c", "-o", objs[0],
                               os.path.join(HERE, "emu_kernels.cpp")])
        tmp = "%s.tmp.%d" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", tmp, SRCS[0], obj] + objs + ["-lm"])
        os.replace(tmp, LIB)
    return LIB
