"""bin/fastplong_amd against the whole reference program (oracle/_ref/fastplong_ref, compiled from the reference's own
sources against the stand-ins of oracle/standin) on the same FASTQ: --out, --failed_out (or --split's files), fastplong.json
and fastplong.html byte for byte, across a flag matrix that reaches adapter auto-detection (DNA and RNA), the full pipeline,
-s only, periodic / homopolymer and N / lower-case adapters, 17 FASTA adapters, -d 0 / 1 with extension 0 / 100, --break /
--mask and --split.  Run on a box without GPUs: the CLI loads tests/stub/libfastplong_amd.so, whose devices compute with the
oracle.  Skipped where the reference program was not built (it needs the reference's sources at build time)."""
import os

import pytest

from fastplong_amd import build
from tests import refbin
from tests.stub import build as stub_build


@pytest.fixture(scope="module")
def env(orc):
    if not orc.have_ref_bin():
        pytest.skip("oracle/_ref/fastplong_ref not built (needs the reference's sources at build time)")
    build.build_host()
    lib = stub_build.build()
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    return e


@pytest.mark.parametrize("name", sorted(refbin.CASES))
def test_cli_equals_reference_binary(tmp_path, env, name):
    kind, _ = refbin.CASES[name]
    inp = tmp_path / "in.fq"
    refbin.write_input(inp, kind)
    fl = refbin.flags_of(name, tmp_path)
    pr = refbin.run_ref(inp, tmp_path / "ref", fl)
    pc = refbin.run_cli(env, inp, tmp_path / "cli", fl, extra_env={"FPLH_CHUNK_BYTES": "200000"})
    want = refbin.outputs(tmp_path / "ref")
    refbin.assert_same(refbin.outputs(tmp_path / "cli"), want)
    assert len(want["out.fq"] if "out.fq" in want else want["0001.out.fq"]) > 0
    if name.startswith("auto"):
        det = refbin.detection_lines(pr)
        assert refbin.detection_lines(pc) == det and len(det) == 2 and all(l.startswith(b"Detected: ") for l in det)


def test_reference_binary_output_does_not_depend_on_threads(tmp_path, env):
    """the yardstick itself: two -w values give the reference identical outputs"""
    inp = tmp_path / "in.fq"
    refbin.write_input(inp, "dna", seed=1)
    fl = refbin.flags_of("full", tmp_path)
    refbin.run_ref(inp, tmp_path / "w1", fl, threads=1)
    refbin.run_ref(inp, tmp_path / "w7", fl, threads=7)
    a, b = refbin.outputs(tmp_path / "w1"), refbin.outputs(tmp_path / "w7")
    for k in ("out.fq", "failed.fq", "json"):
        assert a[k] == b[k], k


def test_end_adapter_derived_from_start_adapter(tmp_path, env):
    """-s without -e: the CLI derives the end adapter with its own reverse complement (host/cli.cpp), the reference with
    Sequence::reverseComplement (src/main.cpp).  -s is validated to A / C / G / T of at least 4 bases by both, so that is
    every input the derivation can get: all lengths 4-70 (the reference's 16-lane body and tail), periodic and homopolymer
    adapters among them.  The end adapter shows in fastplong.json and decides --out."""
    import numpy as np

    rng = np.random.default_rng(23)
    inp = tmp_path / "in.fq"
    refbin.write_input(inp, "dna", n=30, median_len=400)
    for n in range(4, 71):
        k = n % 4
        s = "".join("ACGT"[i] for i in rng.integers(0, 4, n)) if k < 2 else ("ACGT"[n % 4] * n if k == 2 else ("AC" * n)[:n])
        d = tmp_path / ("s%d" % n)
        refbin.run_ref(inp, d / "ref", ["-s", s], threads=1)
        refbin.run_cli(env, inp, d / "cli", ["-s", s], threads=1)
        want, got = refbin.outputs(d / "ref"), refbin.outputs(d / "cli")
        end = [l for l in want["json"] if b'"read_end_adapter"' in l]
        assert end == [b'\t\t"read_end_adapter": "%s",' % s[::-1].translate(str.maketrans("ACGT", "TGCA")).encode()], (s, end)
        refbin.assert_same(got, want)
