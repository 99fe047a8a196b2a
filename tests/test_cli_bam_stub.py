"""bin/fastplong_amd on a BAM input gives exactly what it gives on the input's FASTQ twin (README "BAM input"): --out,
--failed_out, --split*, fastplong.json and fastplong.html, byte for byte -- run on a box without GPUs against
tests/stub_bam/libfastplong_amd.so (the CPU stand-in of tests/stub plus the two BAM entry points).  The BAM inputs are the
golden cases' reads, some stored reverse-complemented (flag 0x10), with secondary / supplementary records mixed in, cut into
small BGZF blocks so that records straddle blocks and, with a small FPLH_CHUNK_BYTES, batches."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from fastplong_amd import build
from tests import bamio, refjson
from tests.stub import build as stub_build
from tests.stub_bam import build as stub_bam_build

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = sorted(d for d in os.listdir(GOLD) if os.path.isdir(os.path.join(GOLD, d)))


@pytest.fixture(scope="module")
def env():
    build.build_host()
    lib = stub_bam_build.build()
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    return e


def case_bam(tmp_path, case, seed=1):
    """the golden reads as a BAM (every third stored reversed, a skipped record every fifth) and the BAM's FASTQ twin"""
    fq = gzip.open(os.path.join(GOLD, case, "in.fq.gz")).read()
    rng = np.random.default_rng(seed)
    recs = []
    for i, (name, _, codes, qual) in enumerate(bamio.fastq_to_records(fq)):
        name = name.replace(b" ", b"_")
        recs.append(bamio.reverse_record(name, codes, qual) if i % 3 == 1 else (name, 0x4, codes, qual))
        if i % 5 == 2:
            recs.append((name + b"_sec", 0x100 if i % 2 else 0x800, codes[:50], qual[:50]))
    data, _, _ = bamio.bam_bytes(recs, block=int(rng.integers(3000, 9000)))
    bam = tmp_path / "x.bam"
    bam.write_bytes(data)
    twin = tmp_path / "twin.fq"
    twin.write_bytes(bamio.bam_to_fastq(data))
    return bam, twin


def run(env, inp, outdir, flags, gpus=1, chunk=None, extra_env=None):
    outdir.mkdir(exist_ok=True)
    cmd = [build.CLI, "-i", str(inp), "-o", str(outdir / "out.fq"), "--failed_out", str(outdir / "failed.fq"),
           "-j", str(outdir / "out.json"), "-h", str(outdir / "out.html"), "--gpus", str(gpus)] + list(flags)
    e = dict(env, FPL_STUB_DEVICES=str(max(gpus, 1)))
    if chunk:
        e["FPLH_CHUNK_BYTES"] = str(chunk)
    e.update(extra_env or {})
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


def outputs(d, names=("out.fq", "failed.fq")):
    got = {}
    for n in names:
        got[n] = (d / n).read_bytes()
    got["json"] = [l for l in (d / "out.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    page = refjson.STAMP.sub(b"<time>", (d / "out.html").read_bytes())
    got["html"] = re.sub(rb"<div id='footer'> <p>.*?</p>", b"<div id='footer'> <p></p>", page, flags=re.S)  # (the command line)
    return got


def flags_of(case):
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    return [f if f != "ADAPTERS.fa" else os.path.join(GOLD, case, "ADAPTERS.fa") for f in meta["flags"]]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("gpus,chunk", [(1, None), (3, 20000)])
def test_cli_bam_equals_twin(tmp_path, env, case, gpus, chunk):
    bam, twin = case_bam(tmp_path, case)
    fl = flags_of(case)
    run(env, twin, tmp_path / "fq", fl, gpus, chunk, {"FPL_STUB_LOG": str(tmp_path / "fq.log")})
    run(env, bam, tmp_path / "bam", fl, gpus, chunk, {"FPL_STUB_LOG": str(tmp_path / "bam.log")})
    assert outputs(tmp_path / "bam") == outputs(tmp_path / "fq")
    if chunk:  # records straddle batches: several batches, dealt over the three devices
        devs = [l.split()[0] for l in open(tmp_path / "bam.log").read().splitlines()]
        assert len(devs) >= 6 and set(devs) == {"0", "1", "2"}


@pytest.mark.parametrize("what", ["gz_out", "split", "split_by_lines", "reads_to_process", "auto_adapters"])
def test_cli_bam_options(tmp_path, env, what):
    case = "c3_full"
    bam, twin = case_bam(tmp_path, case, seed=4)
    fl = flags_of(case)
    names = ("out.fq", "failed.fq")
    if what == "gz_out":
        res = {}
        for tag, inp in (("fq", twin), ("bam", bam)):
            d = tmp_path / tag
            d.mkdir()
            cmd = [build.CLI, "-i", str(inp), "-o", str(d / "o.fq.gz"), "-j", str(d / "out.json"), "-h", str(d / "out.html")] + fl
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(env, FPLH_CHUNK_BYTES="30000"))
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            res[tag] = gzip.decompress((d / "o.fq.gz").read_bytes())
        assert res["bam"] == res["fq"] and len(res["bam"]) > 0
        return
    if what in ("split", "split_by_lines"):
        res = {}
        for tag, inp in (("fq", twin), ("bam", bam)):
            d = tmp_path / tag
            d.mkdir()
            sp = ["--split", "3"] if what == "split" else ["--split_by_lines", "1000"]
            cmd = [build.CLI, "-i", str(inp), "-o", str(d / "o.fq"), "-j", str(d / "out.json"), "-h", str(d / "out.html")] + sp + fl
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(env, FPLH_CHUNK_BYTES="30000"))
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            res[tag] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith("o.fq")}
        assert len(res["bam"]) >= 2 and res["bam"] == res["fq"]
        return
    if what == "reads_to_process":
        fl = fl + ["--reads_to_process", "61"]
    if what == "auto_adapters":
        f0, fl = flags_of(case), []
        for i, f in enumerate(f0):  # (the case's adapters replaced by "auto")
            if f in ("-s", "-e") or (i and f0[i - 1] in ("-s", "-e")):
                continue
            fl.append(f)
        fl += ["-s", "auto", "-e", "auto"]
    pf = run(env, twin, tmp_path / "fq", fl, 1, 30000)
    pb = run(env, bam, tmp_path / "bam", fl, 1, 30000)
    assert outputs(tmp_path / "bam", names) == outputs(tmp_path / "fq", names)
    if what == "auto_adapters":
        det = lambda p: [l for l in p.stderr.split(b"\n") if l.startswith((b"Detected", b"Not detected", b"Found possible"))]
        assert det(pb) == det(pf) and len(det(pb)) == 2


def test_cli_bam_errors_and_warning(tmp_path, env):
    recs = [(b"a%d" % i, 0, bytes([1, 2, 4, 8] * 30), bytes([30] * 120)) for i in range(20)]
    data, _, _ = bamio.bam_bytes(recs[:9] + [(b"pp", 0x1, bytes([1] * 40), bytes([30] * 40))] + recs[9:])
    bam = tmp_path / "p.bam"
    bam.write_bytes(data)
    cmd = [build.CLI, "-i", str(bam), "-o", str(tmp_path / "o.fq"), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode != 0 and b"BAM record 9 (pp)" in p.stderr and b"paired" in p.stderr
    data, _, _ = bamio.bam_bytes(recs, eof=False)
    bam.write_bytes(data)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0 and b"no BGZF EOF block" in p.stderr


def test_cli_without_the_bam_entry_points_says_so(tmp_path):
    """against tests/stub (ABI calls of v7 only): FASTQ runs as before, a BAM input ends with a clear error"""
    build.build_host()
    lib = stub_build.build()
    e = dict(os.environ, LD_LIBRARY_PATH=os.path.dirname(lib) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    recs = [(b"a%d" % i, 0, bytes([1, 2, 4, 8] * 30), bytes([30] * 120)) for i in range(20)]
    data, _, _ = bamio.bam_bytes(recs)
    bam = tmp_path / "x.bam"
    bam.write_bytes(data)
    cmd = [build.CLI, "-i", str(bam), "-o", str(tmp_path / "o.fq"), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    assert p.returncode != 0 and b"fpl_process_bam_async" in p.stderr
