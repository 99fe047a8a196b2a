"""bin/fastplong_amd --keep_tags on a box without GPUs, against tests/stub_bam/libfastplong_amd.so (the CPU stand-in with the BAM
entry points; it has neither fpl_set_bam_tags nor fpl_set_gzip_records, so the host writes every record).  The expected files come
from the plain-Python rule of tests/bam_tag_cases.py applied to what the SAME run writes as FASTQ text: every output read is
found again by its name, and whether it is changed follows from its name, its length and its input record's flag."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from fastplong_amd import build
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.bgzf_out_cases import split_blocks
from tests.stub_bam import build as stub_bam_build
from tests.test_cli_gz_stub import flags_of, gold

CASE = "c3_full"
BREAK = ["--break", "--break_window_size", "40", "--break_mean_quality", "12"]
MASK = ["--mask", "--mask_window_size", "15", "--mask_mean_quality", "14"]
NAME = re.compile(rb"^@(?:r\d+-)?(?:split-by-adapter-(?:left|right)-)?(q\d+)(?: failed_\w+)?$")


@pytest.fixture(scope="module")
def env():
    build.build_host()
    lib = stub_bam_build.build()
    e = dict(os.environ, FPL_STUB_DEVICES="1")
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    return e


@pytest.fixture(scope="module")
def tagged(tmp_path_factory):
    """the golden reads as a tagged BAM: every region of the case list that is not huge, in turn; every third record stored
    reversed, a skipped record with tags every fifth; the header carries two @RG lines among others"""
    keys = [k for k in sorted(tc.REGIONS) if len(tc.REGIONS[k]) < 3000]
    recs = []
    for i, (_, _, codes, qual) in enumerate(bamio.fastq_to_records(gold(CASE, "in.fq.gz"))):
        name = b"q%d" % i
        n, f, c, q = bamio.reverse_record(name, codes, qual) if i % 3 == 1 else (name, 0x4, codes, qual)
        recs.append((n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.REGIONS[keys[i % len(keys)]], n_cigar=2 if i % 7 == 3 else 0)))
        if i % 5 == 2:
            recs.append((b"s%d" % i, 0x100, codes[:40], qual[:40], bamio.encode_record(b"s%d" % i, 0x100, codes[:40], qual[:40], tags=tc.P1 + tc.K1)))
    # one read that passes whole under every set of flags used here is not given: the golden reads decide
    p = tmp_path_factory.mktemp("tagged") / "tagged.bam"
    p.write_bytes(tc.input_bam(recs, header_text=tc.RG_HEADER, block=7000))
    return p, {r[0]: r for r in recs}


def cli(env, args, chunk=None, ok=True):
    e = dict(env)
    if chunk:
        e["FPLH_CHUNK_BYTES"] = str(chunk)
    p = subprocess.run([build.CLI] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    assert (p.returncode == 0) == ok, p.stderr.decode()[-3000:]
    return p


def reports(d):
    return ["-j", d / "o.json", "-h", d / "o.html"]


def model(text, by_name, fragment_mode):
    """the tagged records of a run's FASTQ text -> (record bytes, [kept every field, lost positional, tag bytes])"""
    out, stats = [], tc.Stats()
    for line, seq, qual in bc.fastq_records(text):
        name, flag, codes, _, enc = by_name[NAME.match(line).group(1)]
        changed = fragment_mode or bool(flag & 0x10) or len(seq) != len(codes) or b"split-by-adapter-" in line
        region = tc.aux_region(enc)
        t = tc.pick(region, changed)
        out.append(tc.with_tags(bc.record(line, seq, qual), t))
        stats.note(region, changed, t)
    return b"".join(out), stats.v


def read_bam(path, header_raw):
    """-> the record bytes behind the header; the header's blocks hold nothing else"""
    blocks = split_blocks(path.read_bytes(), eof=True)
    raw, k = b"", 0
    while len(raw) < len(header_raw):
        raw += gzip.decompress(blocks[k])
        k += 1
    assert raw == header_raw
    return b"".join(gzip.decompress(b) for b in blocks[k:])


@pytest.mark.parametrize("what,extra,chunk", [("plain", [], None), ("chunks", [], 20000), ("whole", [], 20000), ("break", BREAK, 20000), ("mask", MASK, None),
                                              ("break_mask", BREAK + MASK, 20000)])
def test_out_and_failed_out_equal_the_model(env, tagged, tmp_path, what, extra, chunk):
    bam, by_name = tagged
    flags = ["-A"] if what == "whole" else flags_of(CASE) + extra  # (-A: nothing is trimmed, so reads pass whole and unchanged)
    for sub in ("fq", "tags", "only_out", "old"):
        (tmp_path / sub).mkdir()
    d = tmp_path / "fq"
    cli(env, ["-i", bam, "-o", d / "out.fq", "--failed_out", d / "failed.fq", *reports(d), *flags], chunk)
    text, failed = (d / "out.fq").read_bytes(), (d / "failed.fq").read_bytes()
    assert len(text) > 10000 and len(failed) > 1000
    want_out, so = model(text, by_name, bool(extra))
    want_failed, sf = model(failed, by_name, bool(extra))
    hdr = tc.header_raw(tc.RG_HEADER)
    assert hdr.count(b"@RG\t") == 2 and len(hdr) > len(bc.HEADER_RAW)  # (the @CO line, with "@RG\t" inside it, is not one)
    d = tmp_path / "tags"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "-V", *reports(d), *flags], chunk)
    assert read_bam(d / "out.bam", hdr) == want_out and read_bam(d / "f.bam", hdr) == want_failed
    assert so[0] > 0 and so[1] > 0 and (extra or sf[0] + sf[1] > 0) and so[3] == 0
    if what == "whole":  # unchanged records keep their positional fields
        assert want_out.count(tc.P1) >= 1 and want_out.count(tc.P4) >= 1
    line = "BAM tags: %d records kept every field, %d lost positional fields (MM, ML, MN, B arrays), %d bytes" % (
        so[0] + sf[0], so[1] + sf[1], so[2] + sf[2])
    assert line.encode() in p.stderr
    if chunk:
        assert int(p.stderr.split(b"host pipeline: ")[1].split()[0]) >= 4  # records straddle batches
    # without --failed_out: the same --out
    d = tmp_path / "only_out"
    cli(env, ["-i", bam, "-o", d / "out.bam", "--keep_tags", *reports(d), *flags], chunk)
    assert read_bam(d / "out.bam", hdr) == want_out
    # without the flag: the bytes of a run that never heard of tags -- the fixed header, records that end at their qualities
    d = tmp_path / "old"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "-V", *reports(d), *flags], chunk)
    assert read_bam(d / "out.bam", bc.HEADER_RAW) == bc.records(text) and read_bam(d / "f.bam", bc.HEADER_RAW) == bc.records(failed)
    assert b"BAM tags" not in p.stderr
    # the reports do not depend on the flag
    js = lambda x: [l for l in (tmp_path / x / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    assert js("tags") == js("old") == js("fq")


def test_fastq_out_beside_a_bam_failed_out(env, tagged, tmp_path):
    bam, by_name = tagged
    flags = flags_of(CASE)
    cli(env, ["-i", bam, "-o", tmp_path / "out.fq", "--failed_out", tmp_path / "f.bam", "--keep_tags", *reports(tmp_path), *flags], 20000)
    (tmp_path / "r").mkdir()
    cli(env, ["-i", bam, "-o", tmp_path / "r" / "out.fq", "--failed_out", tmp_path / "r" / "f.fq", *reports(tmp_path / "r"), *flags], 20000)
    assert (tmp_path / "out.fq").read_bytes() == (tmp_path / "r" / "out.fq").read_bytes()
    assert read_bam(tmp_path / "f.bam", tc.header_raw(tc.RG_HEADER)) == model((tmp_path / "r" / "f.fq").read_bytes(), by_name, False)[0]


def test_the_output_goes_back_in_and_the_tags_survive(env, tagged, tmp_path):
    bam, _ = tagged
    cli(env, ["-i", bam, "-o", tmp_path / "out.bam", "--keep_tags", *reports(tmp_path), "-A"], 20000)
    off = ["-A", "-Q", "-L", "-n", "100", "--n_base_limit", "1000000"]  # every filter and every trim off
    cli(env, ["-i", tmp_path / "out.bam", "-o", tmp_path / "again.bam", "--keep_tags", *reports(tmp_path), *off], 15000)
    a, b = gzip.decompress((tmp_path / "out.bam").read_bytes()), gzip.decompress((tmp_path / "again.bam").read_bytes())
    assert a == b and a.count(b"@RG\t") == 2 and b"MMZC+m" not in a.split(b"\0\0\0\0", 1)[0]
    # ... and a third of the records did keep their fields whole, positional ones included
    assert a.count(tc.P1) >= 1 and a.count(tc.P4) >= 1 and a.count(tc.K2) > 5


def test_error_cases_of_the_flag(env, tagged, tmp_path):
    bam, _ = tagged
    fq = tmp_path / "in.fq"
    fq.write_bytes(gold(CASE, "in.fq.gz"))
    rp = reports(tmp_path)
    for args, word in [(["-i", fq, "-o", tmp_path / "x.bam", "--keep_tags"], b"BAM input"),
                       (["-i", bam, "-o", tmp_path / "x.fq", "--keep_tags"], b".bam"),
                       (["-i", bam, "-o", tmp_path / "x.fq.gz", "--failed_out", tmp_path / "y.fq", "--keep_tags"], b".bam"),
                       (["-i", bam, "-o", tmp_path / "x.bam", "--stdout", "--keep_tags"], b".bam"),
                       (["-i", bam, "--keep_tags"], b".bam")]:
        p = cli(env, args + rp + ["-A"], ok=False)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: ") and b"--keep_tags" in p.stderr and word in p.stderr
    # a record whose fields do not parse ends the run under the flag, and only under it
    rng = np.random.default_rng(4)
    recs = [(b"g%d" % i, 4, rng.integers(1, 16, 200, dtype=np.uint8).tobytes(), bytes([30] * 200)) for i in range(30)]
    recs = [(n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.MALFORMED["z_without_nul"][0] if i == 17 else tc.K1)) for i, (n, f, c, q) in enumerate(recs)]
    bad = tmp_path / "bad.bam"
    bad.write_bytes(tc.input_bam(recs))
    p = cli(env, ["-i", bad, "-o", tmp_path / "o.bam", "--keep_tags", "-A"] + rp, ok=False)
    assert b"ERROR: BAM record 17 (g17): the auxiliary fields do not parse" in p.stderr
    cli(env, ["-i", bad, "-o", tmp_path / "o.bam", "-A", "-Q", "-L", "-n", "100"] + rp)
    assert len(bamio.parse((tmp_path / "o.bam").read_bytes())) == 30


def test_a_header_past_one_block(env, tmp_path):
    rng = np.random.default_rng(5)
    text = b"@HD\tVN:1.6\n" + b"".join(b"@RG\tID:g%d\tDS:%s\n" % (k, b"d" * 60) for k in range(1200))
    recs = [(b"h%d" % i, 4, rng.integers(1, 16, 300, dtype=np.uint8).tobytes(), bytes([30] * 300)) for i in range(10)]
    recs = [(n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.K2 + tc.P2)) for n, f, c, q in recs]
    inp = tmp_path / "in.bam"
    inp.write_bytes(tc.input_bam(recs, header_text=text))
    cli(env, ["-i", inp, "-o", tmp_path / "o.bam", "--keep_tags", "-A", "-Q", "-L", *reports(tmp_path)])
    hdr = tc.header_raw(text)
    assert len(hdr) > 65280
    raw = read_bam(tmp_path / "o.bam", hdr)
    assert raw == b"".join(tc.with_tags(bc.record(b"@" + n, bytes(bamio.CODES[x] for x in c), bytes(v + 33 for v in q)), tc.K2 + tc.P2)
                           for n, f, c, q, _ in recs)
