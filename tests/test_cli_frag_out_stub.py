"""bin/fastplong_amd with --break / --mask, -o x.fq.gz and --device_gzip against libraries WITHOUT fpl_set_fragment_output, on a box
without GPUs: tests/stub (no gzip calls at all) and tests/stub_gz (the v9 gzip calls, whose stand-in logs every member it makes).
The stand-ins are taught nothing: the CLI finds the call by name, does not find it, and silently takes the host path -- the host's
parsers, the host's formatter over the fragment list, the host's deflate -- and writes the golden bytes."""
import gzip

import pytest

from fastplong_amd import build
from tests.stub import build as stub_build
from tests.stub_gz import build as stub_gz_build
from tests.test_cli_gz_stub import SAID, case_input, flags_of, gold, run

CASE = "c3_break_mask"


@pytest.mark.parametrize("which", ["stub", "stub_gz"])
@pytest.mark.parametrize("chunk", [30000, 0])
def test_device_gzip_asked_for_without_the_call(tmp_path, which, chunk):
    build.build_host()
    lib = stub_build.build() if which == "stub" else stub_gz_build.build()
    err, made = run(lib, case_input(tmp_path, CASE), tmp_path / "out.fq.gz", flags_of(CASE), chunk=chunk, extra=["--device_gzip"])
    assert made == [] and SAID not in err and b"device parse:" not in err
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(CASE, "expected.out.fq.gz")
    got = [l for l in (tmp_path / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    assert got == gold(CASE, "expected.json.gz").split(b"\n")
