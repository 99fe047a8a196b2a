"""TEST INFRASTRUCTURE ONLY: builds tests/stub/libfastplong_amd.so, a stand-in for the C-ABI library whose "devices" compute
with the oracle (see fpl_stub.cpp).  Loaded by the CLI only when a test puts this directory on LD_LIBRARY_PATH."""
import os

from tests import cbuild

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libfastplong_amd.so")


def build():
    return cbuild.stand_in(HERE, ["tests/stub/fpl_stub.cpp"], __file__)


if __name__ == "__main__":
    print(build())
