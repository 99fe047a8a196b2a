"""bin/fastplong_amd --device_inflate against tests/stub_bgzf (the inflater calls backed by the product's kernel on the emulator):
the yardstick is the same command without the flag."""
import gzip
import os
import re
import subprocess

import pytest

from fastplong_amd import build
from tests.stub_bam import build as stub_bam_build
from tests.stub_bgzf import build as stub_bgzf_build
from tests.test_cli_bamgz_stub import CASES, GOLD, case_bam, flags_of, reports

LINE = rb"input: BGZF blocks inflated on the device: (\d+) \((\d+) refused, inflated by the host\)"


@pytest.fixture(scope="module")
def lib():
    build.build_host()
    return stub_bgzf_build.build()


def run(lib, inp, d, flags, extra=(), gpus=1, chunk=20000, out="out.fq", rc=0):
    d.mkdir(exist_ok=True)
    e = dict(os.environ, FPL_STUB_DEVICES=str(gpus), FPL_STUB_BGZF_LOG=str(d / "bgzf.log"))
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    if chunk:
        e["FPLH_CHUNK_BYTES"] = str(chunk)
    cmd = [build.CLI, "-i", str(inp), "-o", str(d / out), "--failed_out", str(d / "failed.fq"), "-j", str(d / "out.json"), "-h", str(d / "out.html"),
           "--gpus", str(gpus), "-V"] + list(flags) + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=e)
    assert p.returncode == rc, p.stderr.decode()[-3000:]
    return p.stderr


def outputs(d, out="out.fq"):
    data = (d / out).read_bytes()
    return (gzip.decompress(data) if out.endswith(".gz") else data), (d / "failed.fq").read_bytes(), reports(d)


def counts(err):
    m = re.search(LINE, err)
    return (int(m.group(1)), int(m.group(2))) if m else None


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("case", CASES)
def test_same_outputs_and_reports(lib, tmp_path, case, gpus):
    bam, _ = case_bam(tmp_path, case)
    fl = flags_of(case)
    err0 = run(lib, bam, tmp_path / "host", fl, gpus=gpus)
    err1 = run(lib, bam, tmp_path / "dev", fl, ["--device_inflate"], gpus=gpus)
    assert outputs(tmp_path / "dev") == outputs(tmp_path / "host")
    assert len(outputs(tmp_path / "dev")[0]) > 1000
    assert counts(err0) is None
    dev, refused = counts(err1)
    assert dev > 0 and refused == 0
    log = (tmp_path / "dev" / "bgzf.log").read_text().splitlines()
    assert log and all(l.startswith("0 inflate ") for l in log)  # (one inflater, on the first device)
    assert sum(int(l.split()[2]) for l in log) == dev and not (tmp_path / "host" / "bgzf.log").exists()


def test_with_device_gzip(lib, tmp_path):
    bam, _ = case_bam(tmp_path, "c3_full")
    fl = flags_of("c3_full")
    err0 = run(lib, bam, tmp_path / "host", fl, ["--device_gzip"], out="out.fq.gz")
    err1 = run(lib, bam, tmp_path / "dev", fl, ["--device_gzip", "--device_inflate"], out="out.fq.gz")
    assert (tmp_path / "dev" / "out.fq.gz").read_bytes() == (tmp_path / "host" / "out.fq.gz").read_bytes()
    assert outputs(tmp_path / "dev", "out.fq.gz") == outputs(tmp_path / "host", "out.fq.gz")
    for e in (err0, err1):
        assert b"output: gzip members deflated on the device" in e
    assert counts(err1)[0] > 0 and counts(err1)[1] == 0


def test_split_outputs(lib, tmp_path):
    bam, _ = case_bam(tmp_path, "c1_qualfilter")
    fl = flags_of("c1_qualfilter")
    run(lib, bam, tmp_path / "host", fl, ["--split", "3"])
    run(lib, bam, tmp_path / "dev", fl, ["--split", "3", "--device_inflate"])
    names = sorted(p.name for p in (tmp_path / "host").iterdir() if p.name.endswith("out.fq"))
    assert len(names) == 3
    for n in names:
        assert (tmp_path / "dev" / n).read_bytes() == (tmp_path / "host" / n).read_bytes()


def test_a_library_without_the_calls_keeps_the_host_path(tmp_path):
    build.build_host()
    old = stub_bam_build.build()
    bam, _ = case_bam(tmp_path, "c3_full")
    fl = flags_of("c3_full")
    err0 = run(old, bam, tmp_path / "host", fl)
    err1 = run(old, bam, tmp_path / "dev", fl, ["--device_inflate"])
    assert outputs(tmp_path / "dev") == outputs(tmp_path / "host")
    assert counts(err0) is None and counts(err1) is None


def test_a_corrupt_block_gives_the_host_s_error(lib, tmp_path):
    bam, _ = case_bam(tmp_path, "c1_qualfilter")
    data = bytearray(bam.read_bytes())
    # the fourth block's CRC
    at = 0
    for _ in range(3):
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    size = int.from_bytes(data[at + 16:at + 18], "little") + 1
    data[at + size - 8] ^= 0x40
    bad = tmp_path / "bad.bam"
    bad.write_bytes(bytes(data))
    fl = flags_of("c1_qualfilter")

    def errors(err):
        return [l for l in err.split(b"\n") if l.startswith(b"ERROR")]

    # the exit code of the plain run is the yardstick, whatever it is
    e = dict(os.environ, FPL_STUB_DEVICES="1")
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    outs = []
    for extra in ([], ["--device_inflate"]):
        d = tmp_path / ("e%d" % len(extra))
        d.mkdir()
        p = subprocess.run([build.CLI, "-i", str(bad), "-o", str(d / "out.fq"), "-j", str(d / "o.json"), "-h", str(d / "o.html")] + fl + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=e)
        outs.append((p.returncode, errors(p.stderr)))
    assert outs[0] == outs[1] and outs[0][0] != 0
    assert any(b"the BGZF block at file offset %d has a bad CRC or size" % at in l for l in outs[0][1])


def test_fastq_input_is_untouched_by_the_flag(lib, tmp_path):
    fq = os.path.join(GOLD, "c3_full", "in.fq.gz")
    fl = flags_of("c3_full")
    err0 = run(lib, fq, tmp_path / "a", fl)
    err1 = run(lib, fq, tmp_path / "b", fl, ["--device_inflate"])
    assert outputs(tmp_path / "a") == outputs(tmp_path / "b")
    assert counts(err0) is None and counts(err1) is None
    assert not (tmp_path / "b" / "bgzf.log").exists()
