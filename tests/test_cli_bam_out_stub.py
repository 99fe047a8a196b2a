"""bin/fastplong_amd -o x.bam on a box without GPUs: against tests/stub_bamout/libfastplong_amd.so (the CPU stand-in plus the gzip
calls, fpl_set_gzip_framing and fpl_set_gzip_records, made of the host's formatter, a few independent lines that build records,
and zlib; its blocks hold 49 152 bytes) and against plain tests/stub (no such call: the host converts and frames everything, in
blocks of 65 280).  Pinned: the file is the header block, record blocks and the EOF block; tests/bamio.py reads it back as the
golden output with names cut; the device form and the host form inflate to the same bytes; host blocks lie in order between
device blocks; --failed_out y.bam; --split into BAM is an error; the reports are those of the .fastq run; and a run without .bam
writes what it wrote before."""
import gzip
import os
import subprocess

import pytest

from fastplong_amd import bgzf, build
from tests import bam_out_cases as bc
from tests import bamio
from tests.bgzf_out_cases import HOST_PIECE, STRIPE, split_blocks
from tests.stub import build as stub_build
from tests.stub_bamout import build as stub_bam_build
from tests.test_cli_gz_stub import case_input, flags_of, gold, run

SAID_DEV = b"output: BAM records, packed and deflated on the device"
SAID_HOST = b"output: BAM records, packed and deflated by the host"
CASES = ["c3_full", "c5_fasta"]  # (both write split-by-adapter fragments)


@pytest.fixture(scope="module")
def lib():
    build.build_host()
    return stub_bam_build.build()


@pytest.fixture(scope="module")
def old_lib():
    build.build_host()
    return stub_build.build()


def n_device_blocks(err):
    return int(err.split(b"BAM records: BGZF blocks framed on the device: ")[1].split()[0])


def read_bam(path, want_text):
    """the file's structure and contents -> (uncompressed bytes behind the header, ISIZE of every record block)"""
    data = open(path, "rb").read()
    blocks = split_blocks(data, eof=True)
    assert gzip.decompress(blocks[0]) == bc.HEADER_RAW  # the header block comes first and holds nothing else
    raw = b"".join(gzip.decompress(b) for b in blocks[1:])
    assert raw == bc.records(want_text)
    assert bamio.bam_to_fastq(data) == bc.cut_text(want_text)
    return raw, [int.from_bytes(b[-4:], "little") for b in blocks[1:]]


def reports(d):
    js = [l for l in open(os.path.join(d, "o.json"), "rb").read().split(b"\n") if not l.startswith(b'\t"command":')]
    html = open(os.path.join(d, "o.html"), "rb").read()
    return js, html.split(b"<div id='footer'")[0].count(b"<")


@pytest.mark.parametrize("case", CASES)
def test_device_form_host_form_and_the_fastq_run(lib, tmp_path, case):
    want = gold(case, "expected.out.fq.gz")
    assert b"split-by-adapter-" in want
    inp = case_input(tmp_path, case)
    for sub in ("dev", "host", "one", "fq"):
        (tmp_path / sub).mkdir()
    err, made = run(lib, inp, tmp_path / "dev" / "out.bam", flags_of(case), extra=["--device_gzip"])
    assert SAID_DEV in err and len(made) >= 3 and all(l.split()[1] == "bam" for l in made)
    dev, sizes = read_bam(tmp_path / "dev" / "out.bam", want)
    assert n_device_blocks(err) == len(sizes) == sum(int(l.split()[4]) for l in made)
    assert all(s <= STRIPE for s in sizes) and HOST_PIECE not in sizes
    # without --device_gzip the host form runs: the same bytes inside other blocks
    err, made = run(lib, inp, tmp_path / "host" / "out.bam", flags_of(case))
    assert SAID_HOST in err and made == [] and n_device_blocks(err) == 0
    host, _ = read_bam(tmp_path / "host" / "out.bam", want)
    assert host == dev
    # one chunk: no text batches, the host's form whatever the flag says
    err, made = run(lib, inp, tmp_path / "one" / "out.bam", flags_of(case), chunk=None, extra=["--device_gzip"])
    assert made == [] and read_bam(tmp_path / "one" / "out.bam", want)[0] == dev
    # the reports do not depend on the output's format, and a run without .bam writes what it wrote before
    run(lib, inp, tmp_path / "fq" / "out.fq", flags_of(case))
    assert (tmp_path / "fq" / "out.fq").read_bytes() == want
    assert reports(tmp_path / "dev") == reports(tmp_path / "host") == reports(tmp_path / "fq")
    assert open(tmp_path / "fq" / "o.json", "rb").read().count(b"\n") > 20


def test_a_library_without_the_call_leaves_everything_to_the_host(old_lib, tmp_path):
    case = "c3_full"
    err, made = run(old_lib, case_input(tmp_path, case), tmp_path / "out.bam", flags_of(case), extra=["--device_gzip"])
    assert SAID_HOST in err and made == [] and n_device_blocks(err) == 0
    read_bam(tmp_path / "out.bam", gold(case, "expected.out.fq.gz"))


def test_irregular_chunk_gives_host_blocks_between_device_blocks(lib, tmp_path):
    case = "c3_full"
    lines = gold(case, "in.fq.gz").split(b"\n")
    k = (len(lines) // 8) * 4
    inp = tmp_path / "in.fq"
    inp.write_bytes(b"\n".join(lines[:k]) + b"\n\n" + b"\n".join(lines[k:]))
    err, made = run(lib, inp, tmp_path / "out.bam", flags_of(case), chunk=60000, extra=["--device_gzip"])
    assert b" 0 handed back" not in err and b"handed back to the host's reader" in err
    raw, sizes = read_bam(tmp_path / "out.bam", gold(case, "expected.out.fq.gz"))
    n_dev = n_device_blocks(err)
    assert len(made) >= 2 and 0 < n_dev < len(sizes) and n_dev == sum(int(l.split()[4]) for l in made)


def test_failed_out_is_the_hosts(lib, tmp_path):
    case = "c3_full"
    inp = case_input(tmp_path, case)
    err, made = run(lib, inp, tmp_path / "out.bam", flags_of(case), extra=["--device_gzip", "--failed_out", str(tmp_path / "y.bam")])
    assert SAID_DEV in err and len(made) >= 3
    read_bam(tmp_path / "out.bam", gold(case, "expected.out.fq.gz"))
    failed = gold(case, "expected.failed.fq.gz")
    assert len(failed) > 1000
    read_bam(tmp_path / "y.bam", failed)
    # a FASTQ --out beside a BAM --failed_out
    (tmp_path / "f").mkdir()
    run(lib, inp, tmp_path / "f" / "out.fq", flags_of(case), extra=["--failed_out", str(tmp_path / "f" / "y.bam")])
    assert (tmp_path / "f" / "out.fq").read_bytes() == gold(case, "expected.out.fq.gz")
    read_bam(tmp_path / "f" / "y.bam", failed)


@pytest.mark.parametrize("which", ["new", "old"])
def test_no_read_passes_gives_header_and_eof(lib, old_lib, tmp_path, which):
    case = "c1_qualfilter"
    run(lib if which == "new" else old_lib, case_input(tmp_path, case), tmp_path / "out.bam", flags_of(case),
        extra=["--device_gzip", "--length_required", "100000000"])
    data = (tmp_path / "out.bam").read_bytes()
    blocks = split_blocks(data, eof=True)
    assert len(blocks) == 1 and gzip.decompress(blocks[0]) == bc.HEADER_RAW and bamio.parse(data) == []


def test_split_into_bam_is_an_error(lib, tmp_path):
    case = "c1_qualfilter"
    e = dict(os.environ, FPL_STUB_DEVICES="1")
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    inp = case_input(tmp_path, case)
    for extra in (["--split", "3"], ["--split_by_lines", "400"]):
        p = subprocess.run([build.CLI, "-i", str(inp), "-o", str(tmp_path / "x.bam"), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html")]
                           + extra + flags_of(case), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: ") and b"BAM" in p.stderr
        assert not os.path.exists(tmp_path / "x.bam")


def test_stdout_wins_and_gz_outputs_stay_members(lib, tmp_path):
    case = "c3_full"
    want = gold(case, "expected.out.fq.gz")
    inp = case_input(tmp_path, case)
    e = dict(os.environ, FPL_STUB_DEVICES="1", FPLH_CHUNK_BYTES="30000")
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    p = subprocess.run([build.CLI, "-i", str(inp), "-o", str(tmp_path / "x.bam"), "--stdout", "-j", str(tmp_path / "o.json"), "-h",
                        str(tmp_path / "o.html")] + flags_of(case), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
    assert p.returncode == 0 and p.stdout == want  # FASTQ text, as for -o x.fq.gz --stdout
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case))
    data = (tmp_path / "out.fq.gz").read_bytes()
    assert gzip.decompress(data) == want and not data[3] & 4 and b"BAM" not in err  # no FEXTRA: the members of before
    assert len(made) >= 3 and all(l.split()[1] == "gz" for l in made) and not data.endswith(bgzf.EOF)
