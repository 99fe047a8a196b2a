"""bin/fastplong_amd --bgzf on a box without GPUs: against tests/stub_bgzfout/libfastplong_amd.so (the CPU stand-in plus the gzip
calls and fpl_set_gzip_framing, made of the host's formatter and zlib; its blocks hold 49 152 text bytes) and against plain
tests/stub (no such call: the host frames everything, in blocks of 65 280).  Pinned: every .gz the run writes is BGZF blocks plus
the EOF block and inflates, block by block, to the run's text; host-framed blocks lie in order between device-framed ones; a file
no read reached is exactly the 28 bytes; the file goes back in; --bgzf without a .gz output is an error; and without the flag
nothing is framed."""
import glob
import os
import subprocess

import pytest

from fastplong_amd import bgzf, build
from tests.bgzf_out_cases import HOST_PIECE, STRIPE, check_blocks
from tests.stub import build as stub_build
from tests.stub_bgzfout import build as stub_bgzf_build
from tests.test_cli_gz_stub import TEXT_CASES, case_input, flags_of, gold, run

SAID_DEV = b"output: BGZF blocks, deflated and framed on the device"
SAID_HOST = b"output: BGZF blocks, deflated and framed by the host"


@pytest.fixture(scope="module")
def lib():
    build.build_host()
    return stub_bgzf_build.build()


@pytest.fixture(scope="module")
def old_lib():
    build.build_host()
    return stub_build.build()


def n_device_blocks(err):
    return int(err.split(b"BGZF blocks framed on the device: ")[1].split()[0])


def isizes(blocks):
    return [int.from_bytes(b[-4:], "little") for b in blocks]


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("case", TEXT_CASES)
def test_device_framed_blocks_plus_eof(lib, tmp_path, case, gpus):
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), gpus=gpus, extra=["--bgzf"])
    assert SAID_DEV in err and len(made) >= 3 and all(l.split()[1] == "bgzf" for l in made)
    data = (tmp_path / "out.fq.gz").read_bytes()
    blocks = check_blocks(data, gold(case, "expected.out.fq.gz"), eof=True)
    assert sum(int(l.split()[3]) for l in made) == len(data) - len(bgzf.EOF)  # nothing but the stand-in's blocks and the EOF block
    assert n_device_blocks(err) == len(blocks) == sum(int(l.split()[4]) for l in made)


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("case", TEXT_CASES)
def test_a_library_without_the_call_leaves_the_framing_to_the_host(old_lib, tmp_path, case, gpus):
    err, made = run(old_lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), gpus=gpus, extra=["--bgzf"])
    assert SAID_HOST in err and made == [] and n_device_blocks(err) == 0
    check_blocks((tmp_path / "out.fq.gz").read_bytes(), gold(case, "expected.out.fq.gz"), eof=True)


def test_irregular_chunk_gives_host_blocks_between_device_blocks(lib, tmp_path):
    case = "c3_full"
    lines = gold(case, "in.fq.gz").split(b"\n")
    k = (len(lines) // 8) * 4
    inp = tmp_path / "in.fq"
    inp.write_bytes(b"\n".join(lines[:k]) + b"\n\n" + b"\n".join(lines[k:]))
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case), chunk=60000, extra=["--bgzf"])
    assert b" 0 handed back" not in err and b"handed back to the host's reader" in err
    data = (tmp_path / "out.fq.gz").read_bytes()
    blocks = check_blocks(data, gold(case, "expected.out.fq.gz"), eof=True)
    n_dev = n_device_blocks(err)
    assert len(made) >= 2 and 0 < n_dev < len(blocks) and n_dev == sum(int(l.split()[4]) for l in made)
    assert sum(int(l.split()[3]) for l in made) < len(data) - len(bgzf.EOF)  # (some blocks are the host's)
    assert STRIPE in isizes(blocks) and HOST_PIECE not in isizes(blocks[:1])  # the first chunk is regular: the stand-in's stripe


def test_failed_out_and_split_files_are_bgzf(lib, tmp_path):
    case = "c3_full"
    inp = case_input(tmp_path, case)
    err, made = run(lib, inp, tmp_path / "out.fq.gz", flags_of(case), extra=["--bgzf", "--failed_out", str(tmp_path / "x.fq.gz")])
    assert SAID_DEV in err and len(made) >= 3
    check_blocks((tmp_path / "out.fq.gz").read_bytes(), gold(case, "expected.out.fq.gz"), eof=True)
    check_blocks((tmp_path / "x.fq.gz").read_bytes(), gold(case, "expected.failed.fq.gz"), eof=True)
    # a plain --out beside a --failed_out .gz: the flag is accepted and frames the one .gz there is
    (tmp_path / "f").mkdir()
    run(lib, inp, tmp_path / "f" / "out.fq", flags_of(case), extra=["--bgzf", "--failed_out", str(tmp_path / "f" / "x.fq.gz")])
    check_blocks((tmp_path / "f" / "x.fq.gz").read_bytes(), gold(case, "expected.failed.fq.gz"), eof=True)
    assert (tmp_path / "f" / "out.fq").read_bytes() == gold(case, "expected.out.fq.gz")
    for sub, name, extra in (("a", "out.fq.gz", ["--bgzf"]), ("b", "out.fq", [])):
        (tmp_path / sub).mkdir()
        err, made = run(lib, inp, tmp_path / sub / name, flags_of(case), extra=["--split", "3"] + extra)
        assert made == []  # --split* keeps the host's deflate, now host-framed
    zipped = sorted(glob.glob(str(tmp_path / "a" / "*out.fq.gz")))
    plain = sorted(glob.glob(str(tmp_path / "b" / "*out.fq")))
    assert len(zipped) == len(plain) == 3
    for z, p in zip(zipped, plain):
        check_blocks(open(z, "rb").read(), open(p, "rb").read(), eof=True)


@pytest.mark.parametrize("which", ["new", "old"])
def test_no_read_passes_gives_the_28_bytes(lib, old_lib, tmp_path, which):
    case = "c1_qualfilter"
    run(lib if which == "new" else old_lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case),
        extra=["--bgzf", "--length_required", "100000000"])
    assert (tmp_path / "out.fq.gz").read_bytes() == bgzf.EOF and len(bgzf.EOF) == 28


def test_the_written_file_goes_back_in(lib, tmp_path):
    case = "c3_full"
    run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case), extra=["--bgzf"])
    (tmp_path / "twin.fq").write_bytes(gold(case, "expected.out.fq.gz"))
    outs = []
    for sub, src in (("z", tmp_path / "out.fq.gz"), ("p", tmp_path / "twin.fq")):
        (tmp_path / sub).mkdir()
        run(lib, src, tmp_path / sub / "second.fq", flags_of(case))
        outs.append((tmp_path / sub / "second.fq").read_bytes())
        outs.append([l for l in open(tmp_path / sub / "o.json", "rb").read().split(b"\n") if not l.startswith(b'\t"command":')])
        outs.append(open(tmp_path / sub / "o.html", "rb").read().count(b"<"))
    assert outs[:3] == outs[3:] and len(outs[0]) > 1000


def test_bgzf_without_a_gz_output_is_an_error(lib, tmp_path):
    case = "c1_qualfilter"
    e = dict(os.environ, FPL_STUB_DEVICES="1")
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    inp = case_input(tmp_path, case)
    for outs in (["-o", str(tmp_path / "out.fq")], ["-o", str(tmp_path / "out.fq"), "--failed_out", str(tmp_path / "x.fq")], []):
        p = subprocess.run([build.CLI, "-i", str(inp), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html"), "--bgzf"] + outs + flags_of(case),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=e)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --bgzf needs an output whose name ends in .gz")


def test_without_the_flag_nothing_is_framed(lib, tmp_path):
    case = "c3_full"
    err, made = run(lib, case_input(tmp_path, case), tmp_path / "out.fq.gz", flags_of(case))
    data = (tmp_path / "out.fq.gz").read_bytes()
    assert data[:3] == b"\x1f\x8b\x08" and not data[3] & 4 and b"BGZF" not in err  # no FEXTRA: a plain member
    assert len(made) >= 3 and all(l.split()[1] == "gz" for l in made) and not data.endswith(bgzf.EOF)
