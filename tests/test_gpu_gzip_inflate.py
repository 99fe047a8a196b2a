"""-m gpu: one long deflate stream inflated on the device (fpl_inflate_gzip through engine.Inflater; csrc/gzip_inflate.h), against
zlib.  The streams, the caller's window loop and the rules are tests/gzip_cases.py, the same the emulator runs under the
sanitizers (tests/test_gzip_inflate_emu.py).  What only a device shows: waves that really share a program counter, stores and
loads of one wave and of one workgroup to the same bytes (docs/kernels.md "k_gzip_decode", "k_gzip_windows"), and the library's
buffers growing between calls."""
import os
import re
import subprocess
import zlib

import pytest

from fastplong_amd import abi, build, synth
from tests import gzip_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inflater():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    inf = engine.Inflater(0)
    yield inf
    inf.close()


def caller(inf):
    def batch_call(jobs):
        res = []
        for j in jobs:
            rc, r, data = inf.inflate_gzip(j["comp"], j.get("start_bit", 0), j.get("dict") or b"", j["out_cap"], j.get("chunk_bytes", 0))
            res.append(dict(rc=rc, status=int(r["status"]), out_bytes=int(r["out_bytes"]), end_bit=int(r["end_bit"]), crc32=int(r["crc32"]),
                            final=int(r["final_block"]), chunks=int(r["chunks"]), data=data))
        return res

    return batch_call


def test_zlib_writes_these(inflater):
    runs = gc.run_members(gc.zlib_cases(), caller(inflater))
    gc.check_zlib_list(runs)
    for r in runs:
        if len(r.case.data) > 70000 and "run" not in r.case.name:
            assert len(r.windows) >= 3, (r.case.name, len(r.windows))
        if r.case.name.startswith(("level", "spliced", "far_matches", "sync_flush")):
            assert max(w["chunks"] for w in r.windows) >= 2, r.case.name


def test_must_not_be_believed(inflater):
    runs = gc.run_members(gc.doubt_cases(), caller(inflater))
    gc.check_doubt_list(runs)
    gc.check_doubt_record(runs)  # every window's status and end are the emulator's (tests/golden/gzip_window_results.json)
    by = {r.case.name: r for r in runs}
    for ch in gc.CHUNKS:
        r = by["right_dict/c%d" % ch]
        assert r.final and r.refused == 0 and r.out == r.case.data
        e = by["embedded_stream/c%d" % ch]
        assert e.refused or (e.final and e.out == e.case.data)
        assert not by["out_cap_short/c%d" % ch].final
    assert all(not r.final for r in runs if r.case.name.startswith("cut/"))


def test_hand_made_and_refused_streams_of_the_bgzf_tests(inflater):
    """each as one window: the recorded results, and what holds by rule where this decoder and k_bgzf_inflate differ"""
    res = caller(inflater)(gc.stream_jobs())
    gc.check_stream_record(res)
    gc.check_stream_rules(res)


def test_eight_megabytes_at_the_default_sizes(inflater):
    (r,) = gc.run_members([gc.big_case()], caller(inflater))
    gc.check_zlib_list([r])
    assert sum(w["chunks"] for w in r.windows) > 20


def test_arguments_are_refused_before_anything_runs(inflater):
    comp = gc.raw(b"hello hello hello")
    for kw in (dict(chunk_bytes=63), dict(chunk_bytes=(1 << 24) + 1), dict(start_bit=8 * len(comp)), dict(zdict=b"x" * 32769)):
        rc, _, _ = inflater.inflate_gzip(comp, out_cap=100, **kw)
        assert rc == abi.FPL_ERR_ARG, kw
    assert inflater.inflate_gzip(b"", out_cap=100)[0] == abi.FPL_ERR_ARG
    rc, r, data = inflater.inflate_gzip(comp, out_cap=100)
    assert rc == 0 and r["status"] == 0 and r["final_block"] == 1 and data == b"hello hello hello" and r["crc32"] == zlib.crc32(data)
    assert r["end_bit"] + 7 >> 3 == len(comp)


def test_whole_run_with_device_inflate(inflater, tmp_path):
    """bin/fastplong_amd on a one-member .fastq.gz (level 6, 2000 reads): the same outputs and reports with and without the flag"""
    from tests.test_cli_bamgz_stub import reports

    build.build_all()
    seq, qual, off = synth.ont_like(2000, seed=21, median_len=1500)
    fq = tmp_path / "in.fastq.gz"
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    fq.write_bytes(c.compress(synth.to_fastq(seq, qual, off)) + c.flush())

    def cli(d, extra=()):
        d.mkdir(exist_ok=True)
        cmd = [build.CLI, "-i", str(fq), "-o", str(d / "out.fq"), "--failed_out", str(d / "failed.fq"), "-j", str(d / "out.json"), "-h",
               str(d / "out.html"), "-V", "--chunk_mb", "1"] + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stderr

    err0 = cli(tmp_path / "host")
    err1 = cli(tmp_path / "dev", ["--device_inflate"])
    assert b"inflated on the device" not in err0
    m = re.search(rb"input: gzip member inflated on the device: (\d+) windows \((\d+) refused, inflated by the host\)", err1)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, err1.decode()[-2000:]
    for f in ("out.fq", "failed.fq"):
        assert (tmp_path / "dev" / f).read_bytes() == (tmp_path / "host" / f).read_bytes()
    assert len((tmp_path / "dev" / "out.fq").read_bytes()) > 100000
    assert reports(tmp_path / "dev") == reports(tmp_path / "host")
