"""tests/cbuild.py, the helper every build module under tests/ compiles through: an artefact is rebuilt exactly when a file the
compiler read for it has changed, and it is never left half-written."""
import os
import subprocess

import pytest

from tests import cbuild

FLAGS = ["-O0", "-fPIC", "-shared"]


@pytest.fixture
def tree(tmp_path):
    (tmp_path / "b.h").write_text("#define B 2\n")
    (tmp_path / "a.h").write_text('#include "b.h"\n')
    (tmp_path / "x.cpp").write_text('#include "a.h"\nint x() { return B; }\n')
    out = str(tmp_path / "libx.so")
    assert cbuild.compile(out, FLAGS, [str(tmp_path / "x.cpp")]) == out
    return tmp_path, out


def _build(tmp_path, out):
    cbuild.compile(out, FLAGS, [str(tmp_path / "x.cpp")])
    st = os.stat(out)
    return st.st_ino, st.st_mtime_ns


def test_fresh_artefact_is_not_rebuilt(tree):
    tmp_path, out = tree
    st = os.stat(out)
    assert _build(tmp_path, out) == (st.st_ino, st.st_mtime_ns)


def test_header_of_a_header_rebuilds(tree):
    tmp_path, out = tree
    before = _build(tmp_path, out)
    t = os.path.getmtime(out) + 1
    os.utime(tmp_path / "b.h", (t, t))  # named by no source, only by a.h
    assert str(tmp_path / "b.h") in cbuild.deps(out)
    assert _build(tmp_path, out)[0] != before[0]


def test_missing_dependency_file_rebuilds(tree):
    tmp_path, out = tree
    before = _build(tmp_path, out)
    os.unlink(out + ".d")
    assert _build(tmp_path, out)[0] != before[0] and os.path.exists(out + ".d")


def test_failed_compile_keeps_the_artefact(tree):
    tmp_path, out = tree
    before = _build(tmp_path, out)
    content = open(out, "rb").read()
    t = os.path.getmtime(out) + 1
    (tmp_path / "x.cpp").write_text('#include "a.h"\nint x() { return nothing; }\n')
    os.utime(tmp_path / "x.cpp", (t, t))
    with pytest.raises(subprocess.CalledProcessError):
        cbuild.compile(out, FLAGS, [str(tmp_path / "x.cpp")])
    st = os.stat(out)
    assert (st.st_ino, st.st_mtime_ns) == before and open(out, "rb").read() == content
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]


def test_emulator_library_records_the_adapter_walk():
    """the header that the hand-kept list of tests/emu/emu.py had missed"""
    from tests.emu import emu

    emu.build()
    assert "fastplong_amd/csrc/adapter_pick.h" in [os.path.normpath(d) for d in cbuild.deps(emu.LIB)]
