"""TEST INFRASTRUCTURE ONLY: builds tests/stub_gz/libfastplong_amd.so -- the CPU stand-in of tests/stub (fpl_stub.cpp and the
oracle, unchanged) plus the gzip entry points of gz_stand_in.cpp (the host's formatter + zlib).  Loaded by the CLI only through
LD_LIBRARY_PATH in tests."""
import os

from fastplong_amd import build as fbuild
from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfastplong_amd.so")


def build():
    return cbuild.stand_in(HERE, ["tests/stub_gz/gz_stand_in.cpp"], __file__, host_lib=fbuild.build_host())
