"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bgzf/libfastplong_amd.so -- the stand-in of tests/stub_bamgz (unchanged) plus the
three inflater calls of bgzf_stand_in.cpp, whose blocks are inflated by the product's kernel on the emulator
(tests/emu_bgzf/driver.cpp, here without sanitizers: the CLI that loads the library is not sanitized).  Loaded by the CLI only
through LD_LIBRARY_PATH in tests."""
import os

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfastplong_amd.so")


def build():
    return cbuild.stand_in(HERE, ["tests/stub_bgzf/bgzf_stand_in.cpp"], __file__, emu_src=("emu_kernels.o", "tests/stub_bgzf/emu_kernels.cpp"))
