"""bin/fastplong_amd reading BAM and writing --out *.gz through the gzip-BAM calls of ABI v10, on a box without GPUs: against
tests/stub_bamgz/libfastplong_amd.so (the CPU stand-in; the decoded bases and the members come from the product's kernels on the
emulator).  What is pinned: the inflated output is the plain --out of the run on the BAM's FASTQ twin, every member in the file is the
device's (the form is asked for with --device_gzip: without it a BAM run keeps the host's deflate), reports equal the twin's run, the decoded arrays are asked for only with --failed_out, the conditions under which the
device form is NOT taken, members in input order over three devices, and a library without the v10 symbols (tests/stub_bam) still
serves the CLI on the host path."""
import gzip
import json
import os
import re
import subprocess

import pytest

from fastplong_amd import build
from tests import bamio, refjson
from tests.stub_bam import build as stub_bam_build
from tests.stub_bamgz import build as stub_bamgz_build

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = ["c1_qualfilter", "c3_full", "c5_fasta"]
SAID = b"output: gzip members deflated on the device"


def _records_of(text, keep):
    lines = text.split(b"\n")
    out = []
    for k in range(0, len(lines) - 1, 4):
        name = lines[k][1:].replace(b"split-by-adapter-left-", b"").replace(b"split-by-adapter-right-", b"")
        if name in keep:
            out.append((lines[k], lines[k + 1], b"+", lines[k + 3]))
    return out


def assert_tied_to_the_golden_output(case, twin_out):
    """the twin's plain --out, which the BAM runs are compared with, against the golden expected.out.fq.gz: equal record for record
    once the two things a BAM cannot carry are set aside -- the '+' line is cut to "+", and the few reads whose golden input has
    lower-case bases (which the twin holds in upper case, so adapters are found in them that the golden run does not find) are
    left out of both"""
    lines = gzip.open(os.path.join(GOLD, case, "in.fq.gz")).read().split(b"\n")
    clean = {lines[k][1:] for k in range(0, len(lines) - 1, 4) if lines[k + 1] == lines[k + 1].upper()}
    assert len(clean) >= 0.9 * (len(lines) // 4)
    want = _records_of(gzip.open(os.path.join(GOLD, case, "expected.out.fq.gz")).read(), clean)
    assert len(want) > 20 and _records_of(twin_out, clean) == want


def flags_of(case):
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    return [f if f != "ADAPTERS.fa" else os.path.join(GOLD, case, "ADAPTERS.fa") for f in meta["flags"]]


def case_bam(tmp_path, case):
    """the golden reads as a BAM (every third stored reverse-complemented, secondary / supplementary records mixed in, small BGZF
    blocks so that records straddle blocks) and the BAM's FASTQ twin.  The twin is not the golden input byte for byte -- a BAM
    holds neither lower-case bases nor a '+' line that repeats the name, and the golden inputs have some of both -- so the
    expected bytes are the plain --out of the twin's run, which tests/test_cli_bam_stub.py ties to the same formatter."""
    fq = gzip.open(os.path.join(GOLD, case, "in.fq.gz")).read()
    recs = []
    for i, (name, _, codes, qual) in enumerate(bamio.fastq_to_records(fq)):
        recs.append(bamio.reverse_record(name, codes, qual) if i % 3 == 1 else (name, 0x4, codes, qual))
        if i % 5 == 2:
            recs.append((name + b"_sec", 0x100 if i % 2 else 0x800, codes[:50], qual[:50]))
    data, _, _ = bamio.bam_bytes(recs, block=5000, n_cigar=1, tags=b"RGZa\0")
    bam = tmp_path / "x.bam"
    bam.write_bytes(data)
    twin = tmp_path / "twin.fq"
    twin.write_bytes(bamio.bam_to_fastq(data))
    return bam, twin


def run(lib, inp, outdir, flags, out="out.fq.gz", gpus=1, chunk=20000, extra=("--device_gzip",)):
    """-> (stderr, lines of the stand-in's log)"""
    outdir.mkdir(exist_ok=True)
    log = str(outdir / "bamgz.log")
    e = dict(os.environ, FPL_STUB_DEVICES=str(gpus), FPL_STUB_BAMGZ_LOG=log)
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    if chunk:
        e["FPLH_CHUNK_BYTES"] = str(chunk)
    cmd = [build.CLI, "-i", str(inp), "-o", str(outdir / out), "-j", str(outdir / "out.json"), "-h", str(outdir / "out.html"), "--gpus", str(gpus),
           "-V"] + list(flags) + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=e)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p.stderr, (open(log).read().splitlines() if os.path.exists(log) else [])


def reports(d):
    js = [l for l in (d / "out.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    page = refjson.STAMP.sub(b"<time>", (d / "out.html").read_bytes())
    return js, re.sub(rb"<div id='footer'> <p>.*?</p>", b"<div id='footer'> <p></p>", page, flags=re.S)


def device_count(err):
    m = re.search(rb"device gzip: (\d+) members", err)
    return int(m.group(1)) if m else None


@pytest.fixture(scope="module")
def lib():
    build.build_host()
    return stub_bamgz_build.build()


@pytest.mark.parametrize("chunk", [None, 20000])
@pytest.mark.parametrize("case", CASES)
def test_device_members_inflate_to_the_golden_output(lib, tmp_path, case, chunk):
    bam, twin = case_bam(tmp_path, case)
    fl = flags_of(case)
    run(lib, twin, tmp_path / "fq", fl, out="out.fq", chunk=chunk)
    err, log = run(lib, bam, tmp_path / "bam", fl, chunk=chunk)
    made = [l for l in log if " gz " in l]
    subs = [l for l in log if " bam " in l]
    assert SAID in err and device_count(err) == len(made) >= 1
    if chunk:
        assert len(made) >= 3  # many small batches
    else:
        assert len(subs) == 1  # one batch
    assert all(l.endswith("seq_out=0 gz=1") for l in subs)  # no --failed_out: the decoded arrays never cross the link
    data = (tmp_path / "bam" / "out.fq.gz").read_bytes()
    want = (tmp_path / "fq" / "out.fq").read_bytes()
    assert len(want) > 1000 and gzip.decompress(data) == want
    assert_tied_to_the_golden_output(case, want)
    assert sum(int(l.split()[3]) for l in made) == len(data)  # nothing but the device's members in the file
    assert reports(tmp_path / "bam") == reports(tmp_path / "fq")


@pytest.mark.parametrize("failed", ["f.fq", "f.fq.gz"])
def test_failed_out_is_formatted_on_the_host_from_the_decoded_arrays(lib, tmp_path, failed):
    case = "c3_full"
    bam, twin = case_bam(tmp_path, case)
    fl = flags_of(case)
    run(lib, twin, tmp_path / "fq", fl + ["--failed_out", str(tmp_path / "fq" / "f.fq")], out="out.fq")
    err, log = run(lib, bam, tmp_path / "bam", fl + ["--failed_out", str(tmp_path / "bam" / failed)])
    made = [l for l in log if " gz " in l]
    assert SAID in err and device_count(err) == len(made) >= 3
    assert all(l.endswith("seq_out=1 gz=1") for l in log if " bam " in l)
    data = (tmp_path / "bam" / "out.fq.gz").read_bytes()
    assert gzip.decompress(data) == (tmp_path / "fq" / "out.fq").read_bytes()
    assert sum(int(l.split()[3]) for l in made) == len(data)
    got = (tmp_path / "bam" / failed).read_bytes()
    want = (tmp_path / "fq" / "f.fq").read_bytes()
    assert len(want) > 0 and (gzip.decompress(got) if failed.endswith(".gz") else got) == want
    assert reports(tmp_path / "bam") == reports(tmp_path / "fq")


@pytest.mark.parametrize("off", [["--host_gzip"], ["-z", "6"], ["--split", "3"], ["--break"]])
def test_what_turns_the_device_form_off(lib, tmp_path, off):
    case = "c3_full"
    bam, twin = case_bam(tmp_path, case)
    fl = flags_of(case) + off
    err_t, _ = run(lib, twin, tmp_path / "fq", fl, extra=["--host_gzip"] if off != ["--host_gzip"] else [])
    assert SAID not in err_t
    err, log = run(lib, bam, tmp_path / "bam", fl)
    assert SAID not in err and device_count(err) is None
    assert not [l for l in log if " gz " in l]
    assert all(l.endswith("seq_out=1 gz=0") for l in log if " bam " in l) and log
    names = sorted(f for f in os.listdir(tmp_path / "bam") if f.endswith("out.fq.gz"))
    assert names == sorted(f for f in os.listdir(tmp_path / "fq") if f.endswith("out.fq.gz")) and names
    for f in names:  # (the same inflated bytes as the twin's run through the host's deflate)
        assert gzip.decompress((tmp_path / "bam" / f).read_bytes()) == gzip.decompress((tmp_path / "fq" / f).read_bytes())


def test_without_the_flag_a_bam_run_keeps_the_host_path(lib, tmp_path):
    case = "c3_full"
    bam, twin = case_bam(tmp_path, case)
    run(lib, twin, tmp_path / "fq", flags_of(case), out="out.fq", extra=())
    err, log = run(lib, bam, tmp_path / "bam", flags_of(case), extra=())
    assert SAID not in err and device_count(err) is None and not [l for l in log if " gz " in l]
    assert all(l.endswith("seq_out=1 gz=0") for l in log if " bam " in l) and log
    assert gzip.decompress((tmp_path / "bam" / "out.fq.gz").read_bytes()) == (tmp_path / "fq" / "out.fq").read_bytes()


def test_three_devices_members_in_input_order(lib, tmp_path):
    case = "c5_fasta"
    bam, twin = case_bam(tmp_path, case)
    run(lib, twin, tmp_path / "fq", flags_of(case), out="out.fq")
    err, log = run(lib, bam, tmp_path / "bam", flags_of(case), gpus=3, chunk=15000)
    made = [l for l in log if " gz " in l]
    assert SAID in err and device_count(err) == len(made) >= 6
    assert {int(l.split()[0]) for l in made} == {0, 1, 2}
    data = (tmp_path / "bam" / "out.fq.gz").read_bytes()
    assert gzip.decompress(data) == (tmp_path / "fq" / "out.fq").read_bytes()
    assert sum(int(l.split()[3]) for l in made) == len(data)


def test_a_library_without_the_v10_calls_keeps_the_host_path(tmp_path):
    build.build_host()
    lib = stub_bam_build.build()
    case = "c1_qualfilter"
    bam, twin = case_bam(tmp_path, case)
    run(lib, twin, tmp_path / "fq", flags_of(case), out="out.fq")
    err, log = run(lib, bam, tmp_path / "bam", flags_of(case))
    assert SAID not in err and log == []
    assert gzip.decompress((tmp_path / "bam" / "out.fq.gz").read_bytes()) == (tmp_path / "fq" / "out.fq").read_bytes()
