"""fplh::bgzf_into (fastplong_amd/host/gzip.cpp) through its test hook: the host's form of the BGZF container -- the text cut
every 65 280 bytes, every piece a block gzip takes on its own (CRC-32 and ISIZE), none longer than 65 536 bytes, the blocks
joined equal to the input; data that does not deflate is stored and still fits.  Empty input gives no bytes."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.bgzf_out_cases import HOST_PIECE, check_blocks
from tests.gzcheck import GOLD, gz, load_hostlib


@pytest.fixture(scope="module")
def hostlib():
    L = load_hostlib()
    L.fplh_bgzf_into.restype = C.c_int
    L.fplh_bgzf_into.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    return L


def bgzf_into(L, data, level):
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_bgzf_into(data, len(data), level, C.byref(out), C.byref(n)) == 0
    if n.value == 0:
        assert not out.value
        return b""
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    return s


def acgt(n, seed=1):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


TEXTS = {
    "acgt": acgt(300_000),
    "golden": gz(os.path.join(GOLD, "c3_full", "expected.out.fq.gz")),
    "random": np.random.default_rng(2).integers(0, 256, 200_000, dtype=np.uint8).tobytes(),  # stored blocks
}


@pytest.mark.parametrize("level", [1, 4, 9])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_blocks_inflate_to_the_input(hostlib, name, level):
    text = TEXTS[name]
    data = bgzf_into(hostlib, text, level)
    blocks = check_blocks(data, text, piece=HOST_PIECE)
    if name == "random":
        assert max(len(b) for b in blocks) == HOST_PIECE + 5 + 26  # stored, and inside a block
    else:
        assert len(data) < len(text) * 0.6


@pytest.mark.parametrize("level", [1, 4, 9])
@pytest.mark.parametrize("n", [0, 1, 65279, 65280, 65281])
def test_lengths_at_the_piece_edge(hostlib, n, level):
    text = acgt(n, seed=3)
    data = bgzf_into(hostlib, text, level)
    if n == 0:
        assert data == b""
        return
    assert len(check_blocks(data, text, piece=HOST_PIECE)) == (2 if n > HOST_PIECE else 1)


def test_the_zlib_path_writes_the_same_container(hostlib, tmp_path):
    """without libdeflate (FPLH_NO_LIBDEFLATE, read once per process: a child) the pieces go through zlib"""
    import subprocess
    import sys

    code = ("import ctypes as C, sys\n"
            "from tests.test_host_bgzf_out import bgzf_into, TEXTS\n"
            "from tests.gzcheck import load_hostlib\n"
            "L = load_hostlib()\n"
            "L.fplh_bgzf_into.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]\n"
            "assert not L.fplh_have_libdeflate()\n"
            "for k in sorted(TEXTS):\n"
            "    open(sys.argv[1] + k, 'wb').write(bgzf_into(L, TEXTS[k], 4))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code, str(tmp_path) + os.sep], check=True, cwd=root, env=dict(os.environ, FPLH_NO_LIBDEFLATE="1"), timeout=120)
    for k in sorted(TEXTS):
        check_blocks((tmp_path / k).read_bytes(), TEXTS[k], piece=HOST_PIECE)
