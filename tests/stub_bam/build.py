"""TEST INFRASTRUCTURE ONLY: builds tests/stub_bam/libfastplong_amd.so -- the CPU stand-in of tests/stub (fpl_stub.cpp and the
oracle, unchanged) plus the two BAM entry points of bam_stand_in.cpp.  Loaded by the CLI only through LD_LIBRARY_PATH in tests."""
import os

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfastplong_amd.so")


def build():
    return cbuild.stand_in(HERE, ["tests/stub/fpl_stub.cpp", "tests/stub_bam/bam_stand_in.cpp"], __file__)
