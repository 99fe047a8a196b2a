"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bamgz/libfastplong_amd.so -- the CPU stand-in of tests/stub (fpl_stub.cpp and the
oracle, unchanged) plus the BAM and gzip-BAM entry points of bamgz_stand_in.cpp, whose decoded bases and gzip members come from the
product's kernels on the emulator (tests/emu_bamgz/driver.cpp).  Loaded by the CLI only through LD_LIBRARY_PATH in tests."""
import os

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfastplong_amd.so")


def build():
    return cbuild.stand_in(HERE, ["tests/stub_bamgz/bamgz_stand_in.cpp"], __file__, emu_src=("emu_driver.o", "tests/emu_bamgz/driver.cpp"))
