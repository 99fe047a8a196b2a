"""No-GPU checks of C-ABI version 10 (gzip members of BAM batches): the built library exports the two new calls beside
fpl_get_gzip_batches, reports version 10, and the Python front end declares them."""
import ctypes as C

import pytest

from fastplong_amd import abi, build, engine


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return engine.load_library()


def test_the_gzip_bam_calls_are_exported(lib):
    raw = C.CDLL(engine.LIB_PATH)
    for name in ("fpl_set_bam_gzip", "fpl_wait_bam_gz", "fpl_get_gzip_batches"):
        assert hasattr(raw, name), name
        assert name in engine.EXPORTS


def test_abi_version_is_10(lib):
    assert lib.fpl_abi_version() == 10 == abi.FPL_ABI_VERSION


def test_null_arguments_are_refused(lib):
    gp, gl = C.c_void_p(), C.c_uint64(0)
    assert lib.fpl_set_bam_gzip(None, 1) == abi.FPL_ERR_ARG
    assert lib.fpl_wait_bam_gz(None, C.byref(gp), C.byref(gl)) == abi.FPL_ERR_ARG
