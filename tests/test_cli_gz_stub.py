"""bin/fastplong_amd writing --out *.gz through the device-gzip calls of ABI v9, on a box without GPUs: against
tests/stub_gz/libfastplong_amd.so (the CPU stand-in plus fpl_set_text_gzip / fpl_wait_text_gz made of the host's formatter and
zlib).  What is pinned: the inflated output is the plain run's text whichever form a batch took; host members sit in order
between device members; the conditions under which the device form is NOT taken (the stand-in logs every member it makes); the
project's own multi-member reader takes the file back; and a library without the v9 symbols (tests/stub) still serves the CLI."""
import glob
import gzip
import json
import os
import subprocess

import pytest

from fastplong_amd import build
from tests.stub import build as stub_build
from tests.stub_gz import build as stub_gz_build

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = sorted(d for d in os.listdir(GOLD) if os.path.isdir(os.path.join(GOLD, d)))
# --break / --mask batches are never text batches (their fragment lists come back through the CSR calls): the host's deflate
TEXT_CASES = [c for c in CASES if c != "c3_break_mask"]
SAID = b"output: gzip members deflated on the device"


def gold(case, name):
    return gzip.open(os.path.join(GOLD, case, name)).read()


def flags_of(case):
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    return [f if f != "ADAPTERS.fa" else os.path.join(GOLD, case, "ADAPTERS.fa") for f in meta["flags"]]


def run(lib, inp, out, flags, gpus=1, chunk=30000, extra=()):
    """-> (stderr, lines of the stand-in's member log)"""
    log = str(out) + ".gzlog"
    e = dict(os.environ, FPL_STUB_DEVICES=str(gpus), FPL_STUB_GZ_LOG=log)
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    if chunk:
        e["FPLH_CHUNK_BYTES"] = str(chunk)
    d = os.path.dirname(str(out))
    cmd = [build.CLI, "-i", str(inp), "-o", str(out), "-j", os.path.join(d, "o.json"), "-h", os.path.join(d, "o.html"), "--gpus", str(gpus),
           "--reader_threads", "3", "-V"] + list(flags) + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stderr, (open(log).read().splitlines() if os.path.exists(log) else [])


@pytest.fixture(scope="module")
def lib():
    build.build_host()
    return stub_gz_build.build()


def case_input(tmp_path, case):
    inp = tmp_path / "in.fq"
    inp.write_bytes(gold(case, "in.fq.gz"))
    return inp


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("case", TEXT_CASES)
def test_device_members_inflate_to_the_golden_output(lib, tmp_path, case, gpus):
    inp = case_input(tmp_path, case)
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case), gpus=gpus)
    assert SAID in err and len(made) >= 3  # several chunks, every one a member of the device's
    assert {int(l.split()[0]) for l in made} == set(range(gpus))  # batch k's bytes come from device k mod N
    data = (tmp_path / "out.fq.gz").read_bytes()
    assert gzip.decompress(data) == gold(case, "expected.out.fq.gz")
    assert data.count(b"\x1f\x8b\x08") >= len(made)
    assert sum(int(l.split()[3]) for l in made) == len(data)  # nothing but the device's members in the file


def test_one_chunk_input_keeps_the_host_path(lib, tmp_path):
    case = TEXT_CASES[0]
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), chunk=None)
    assert made == [] and gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(case, "expected.out.fq.gz")


def test_failed_out_gz_beside_it(lib, tmp_path):
    case = "c3_full"
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), extra=["--failed_out", str(tmp_path / "x.fq.gz")])
    assert SAID in err and len(made) >= 3
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(case, "expected.out.fq.gz")
    assert gzip.decompress((tmp_path / "x.fq.gz").read_bytes()) == gold(case, "expected.failed.fq.gz")


def test_irregular_chunk_is_a_host_member_between_device_members(lib, tmp_path):
    """a blank line in the middle of the input: that chunk goes to the host's reader, is formatted and deflated by the host, and
    its member lies in order between the device's"""
    case = "c3_full"
    text = gold(case, "in.fq.gz")
    lines = text.split(b"\n")
    k = (len(lines) // 8) * 4
    text = b"\n".join(lines[:k]) + b"\n\n" + b"\n".join(lines[k:])
    inp = tmp_path / "in.fq"
    inp.write_bytes(text)
    (tmp_path / "p").mkdir()
    run(lib, inp, tmp_path / "p" / "plain.fq", flags_of(case))
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case))
    plain = (tmp_path / "p" / "plain.fq").read_bytes()
    data = (tmp_path / "out.fq.gz").read_bytes()
    assert gzip.decompress(data) == plain == gold(case, "expected.out.fq.gz")
    assert b" 0 handed back" not in err and b"handed back to the host's reader" in err
    assert len(made) >= 2 and sum(int(l.split()[3]) for l in made) < len(data)  # (some members are the host's)


@pytest.mark.parametrize("extra", [["--host_gzip"], ["-z", "6"], ["--host_parse"]])
def test_conditions_that_keep_the_host_deflate(lib, tmp_path, extra):
    case = "c5_fasta"
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), extra=extra)
    assert made == [] and SAID not in err
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(case, "expected.out.fq.gz")


def test_split_keeps_the_host_deflate(lib, tmp_path):
    case = "c3_full"
    inp = case_input(tmp_path, case)
    for sub, name in (("a", "out.fq.gz"), ("b", "out.fq")):
        (tmp_path / sub).mkdir()
        err, made = run(lib, inp, tmp_path / sub / name, flags_of(case), extra=["--split", "4"])
        assert made == [] and SAID not in err
    zipped = sorted(glob.glob(str(tmp_path / "a" / "*out.fq.gz")))
    plain = sorted(glob.glob(str(tmp_path / "b" / "*out.fq")))
    assert len(zipped) == len(plain) == 4
    assert [gzip.open(z).read() for z in zipped] == [open(p, "rb").read() for p in plain]


def test_break_keeps_the_host_deflate(lib, tmp_path):
    case = "c3_break_mask"
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case))
    assert made == [] and SAID not in err
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(case, "expected.out.fq.gz")


def test_the_written_file_goes_back_in(lib, tmp_path):
    """second pass: -i <the .gz this CLI wrote> (the project's own multi-member reader) gives what -i <its plain twin> gives"""
    case = "c3_full"
    inp = case_input(tmp_path, case)
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case))
    assert len(made) >= 3
    (tmp_path / "twin.fq").write_bytes(gzip.decompress((tmp_path / "out.fq.gz").read_bytes()))
    outs = []
    for sub, src in (("z", tmp_path / "out.fq.gz"), ("p", tmp_path / "twin.fq")):
        (tmp_path / sub).mkdir()
        run(lib, src, tmp_path / sub / "second.fq", flags_of(case))
        outs.append((tmp_path / sub / "second.fq").read_bytes())
        js = [l for l in open(tmp_path / sub / "o.json", "rb").read().split(b"\n") if not l.startswith(b'\t"command":')]
        outs.append(js)
    assert outs[0] == outs[2] and outs[1] == outs[3] and len(outs[0]) > 1000


def test_a_library_without_the_v9_symbols_still_serves(tmp_path):
    build.build_host()
    old = stub_build.build()
    case = "c1_qualfilter"
    err, made = run(old, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case))
    assert made == [] and SAID not in err
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == gold(case, "expected.out.fq.gz")
