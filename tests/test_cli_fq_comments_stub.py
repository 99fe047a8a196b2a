"""bin/fastplong_amd --reindex_comments on a box without GPUs, against tests/stub_bam/libfastplong_amd.so (the CPU stand-in; it has
no device form of the flag, so the host rewrites every name line) and tests/stub_gz (the stand-in whose text batches come back
deflated: under the flag the host must write them all the same).

(a) the error texts, and that without the flag the bytes are today's.
(b) the equivalence that makes the BAM side the oracle: a BAM without flag 0x10 and its twin as FASTQ with every field as a comment
    (the project's own --comment_tags '*' -A -Q -L) give, under the same flags, the same --out and --failed_out text and the same
    JSON -- the one through --comment_tags, the other through --reindex_comments.  For the .gz forms the INFLATED text is compared:
    members and blocks end where batches and formatter slices end, and those fall on different reads for BAM chunks and text chunks.
(c) the expected files and the -V line from the plain-Python model (tests/fq_comment_cases.py) applied to what the SAME run writes
    without the flag, as in tests/test_cli_bam_comments_stub.py."""
import gzip
import os
import re

import numpy as np
import pytest

from fastplong_amd import build
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc
from tests import bamio
from tests import fq_comment_cases as fc
from tests.bgzf_out_cases import split_blocks
from tests.stub_gz import build as stub_gz_build
from tests.test_cli_bam_tags_stub import BREAK, CASE, cli, env, reports  # noqa: F401 (env: a fixture)
from tests.test_cli_gz_stub import flags_of, gold

V_LINE = "FASTQ comments re-indexed: %d reads, %d not re-indexable and dropped, %d positions kept, %d cut away, %d reads left as they are (not tags)"
LINE = re.compile(rb"^@((?:r\d+-)?(?:split-by-adapter-(?:left|right)-)?)([^\t ]+)")


@pytest.fixture(scope="module")
def pair(env, tmp_path_factory):
    """the golden reads as a BAM with generated modification calls and no record reversed (tests/test_cli_bam_mods_stub.py's recipe:
    5mC / 5hmC at every CpG, 6mA at every fourth A, a sparse N group, every eleventh record with an ML one value short, some with a
    move table), and its twin as FASTQ with comments -> (bam, twin.fq, {name: (name line, bases, qualities)} of the twin)"""
    rng = np.random.default_rng(8)
    recs = []
    for i, (_, _, c, q) in enumerate(bamio.fastq_to_records(gold(CASE, "in.fq.gz"))):
        name = b"q%d" % i
        occ = mc.occurrences(c, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(c) and c[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(c, b"A", 4, 3)), (b"N+n", mc.every(c, b"N", 211, 50))]
        tags = mc.fields_of(c, spec, rng, between=tc.P4 if i % 4 == 1 else tc.K1)
        if i % 11 == 7:
            tags = tc.K1 + mc.mm_field(spec) + mc.ml_field([1] * (sum(len(d) * mc.k_of(h) for h, d in spec) - 1))
        recs.append((name, 0x4, c, q, bamio.encode_record(name, 0x4, c, q, tags=tags)))
    d = tmp_path_factory.mktemp("pair")
    (d / "in.bam").write_bytes(tc.input_bam(recs, header_text=tc.RG_HEADER, block=7000))
    cli(env, ["-i", d / "in.bam", "--comment_tags", "*", "-A", "-Q", "-L", "-n", "100", "-o", d / "twin.fq", *reports(d)], 20000)
    lines = (d / "twin.fq").read_bytes().split(b"\n")
    assert len(lines) == 4 * len(recs) + 1 and all(b"\tMM:Z:" in l and b"\tML:B:C" in l for l in lines[:-1:4])
    return d / "in.bam", d / "twin.fq", {l.split(b"\t")[0][1:]: (l, s, q) for l, s, q in zip(lines[0::4], lines[1::4], lines[3::4])}


def model(text, by_name, fragment_mode=False):
    """a run's FASTQ text as the same run writes it under --reindex_comments -> (text, the five counts, [(s, changed, kept)] of the reads)"""
    out, st, seen = [], [0] * 5, []
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    for k in range(0, len(lines) - 1, 4):
        fmt, seq, plus, qual = lines[k:k + 4]
        prefix, name = LINE.match(fmt).groups()
        line, bases, in_qual = by_name[name]
        tail = fmt[1 + len(prefix) + len(line) - 1:]
        assert fmt == b"@" + prefix + line[1:] + tail and (tail == b"" or tail.startswith(b" failed_"))
        changed = fragment_mode or len(seq) != len(bases) or b"split-by-adapter-" in prefix
        s = 0
        if changed and seq and not fragment_mode:  # (where re-indexing can apply, the piece's place matters)
            at = [j for j in range(len(bases) - len(seq) + 1) if bases[j:j + len(seq)] == seq and in_qual[j:j + len(seq)] == qual]
            assert len(at) == 1, fmt
            s = at[0]
        before = st[2]
        new = fc.line_of(line, bases, s, len(seq), changed, prefix, tail[1:] if tail else None, fragment_mode, st)
        seen.append((s, changed, st[2] - before))
        out.append(b"\n".join((new, seq, plus, qual)) + b"\n")
    return b"".join(out), st, seen


def v_line(p):
    return [l for l in p.stderr.split(b"\n") if l.startswith(b"FASTQ comments re-indexed:")]


def js(d):
    return [l for l in (d / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]


@pytest.fixture(scope="module")
def base(env, pair, tmp_path_factory):
    """the twin's run without the flag, once: --out and --failed_out as plain text, several batches"""
    d = tmp_path_factory.mktemp("base")
    p = cli(env, ["-i", pair[1], "-o", d / "out.fq", "--failed_out", d / "failed.fq", "-V", *reports(d), *flags_of(CASE)], 20000)
    assert not v_line(p)
    return (d / "out.fq").read_bytes(), (d / "failed.fq").read_bytes(), js(d)


@pytest.mark.parametrize("form", ["fq", "gz", "bgzf"])
def test_the_twin_under_the_flag_equals_the_bam_under_comment_tags_and_the_model(env, pair, base, tmp_path, form):
    bam, twin, by_name = pair
    ext = "fq" if form == "fq" else "fq.gz"
    extra = ["--bgzf"] if form == "bgzf" else []
    text = {}
    for sub, args in (("a", ["-i", bam, "--comment_tags", "*"]), ("b", ["-i", twin, "--reindex_comments"])):
        d = tmp_path / sub
        d.mkdir()
        p = cli(env, [*args, "-o", d / ("out." + ext), "--failed_out", d / ("failed." + ext), "-V", *extra, *reports(d), *flags_of(CASE)], 20000)
        raw = [(d / (f + "." + ext)).read_bytes() for f in ("out", "failed")]
        if form == "bgzf":
            assert len(split_blocks(raw[0], eof=True)) >= 4
        text[sub] = raw if form == "fq" else [gzip.decompress(r) for r in raw]
        assert int(p.stderr.split(b"host pipeline: ")[1].split()[0]) >= 4  # (several batches)
    assert text["a"][0] == text["b"][0] and text["a"][1] == text["b"][1]
    assert js(tmp_path / "a") == js(tmp_path / "b") == base[2]
    # (c) the model, on what the same run writes without the flag; and the run holds what the test is about
    want_out, so, seen_out = model(base[0], by_name)
    want_failed, sf, seen_failed = model(base[1], by_name)
    assert text["b"][0] == want_out and text["b"][1] == want_failed
    total = [x + y for x, y in zip(so, sf)]
    assert v_line(p) == [(V_LINE % tuple(total)).encode()]
    assert all(x > 0 for x in total[:4]) and total[4] == 0 and sf[0] > 0
    assert sum(1 for s, ch, kept in seen_out if s > 0 and kept > 0) > 20  # front-trimmed reads that carry calls
    halves = [l for l in want_out.split(b"\n")[::4] if l.startswith(b"@split-by-adapter-") and b"\tMM:Z:C+mh?," in l]
    assert len(halves) > 5 and any(b"-right-" in l for l in halves) and any(b"-left-" in l for l in halves)
    assert want_out != base[0] and re.search(rb"^@q\d+ failed_\w+\tRG:Z:", want_failed, re.M)


def test_without_the_flag_the_bytes_are_today_s(env, pair, base):
    """the twin's run without the flag is the formatter's: every name line is the input's, a prefix behind its '@' or a failure
    word behind it"""
    _, _, by_name = pair
    for text in base[:2]:
        for fmt in text.split(b"\n")[:-1:4]:
            prefix, name = LINE.match(fmt).groups()
            line = by_name[name][0]
            assert fmt.startswith(b"@" + prefix + line[1:]) and re.fullmatch(rb"(?: failed_\w+)?", fmt[len(prefix) + len(line):])


def test_stdout_and_split_files_equal_the_model(env, pair, base, tmp_path):
    bam, twin, by_name = pair
    p = cli(env, ["-i", twin, "--stdout", "--reindex_comments", *reports(tmp_path), *flags_of(CASE)], 20000)
    assert p.stdout == model(base[0], by_name)[0]
    for gz in (False, True):
        name = "o.fq.gz" if gz else "o.fq"
        files = {}
        for sub, extra in (("base", []), ("fixed", ["--reindex_comments", "-V"])):
            d = tmp_path / (sub + str(gz))
            d.mkdir()
            p = cli(env, ["-i", twin, "-o", d / name, "--split", "3", *extra, *reports(d), *flags_of(CASE)], 20000)
            files[sub] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith(name)}
        assert len(files["base"]) == 3 and sorted(files["base"]) == sorted(files["fixed"])
        total = [0] * 5
        for f, raw in files["base"].items():
            want, st, _ = model(gzip.decompress(raw) if gz else raw, by_name)
            got = files["fixed"][f]
            assert (gzip.decompress(got) if gz else got) == want
            total = [a + b for a, b in zip(total, st)]
        assert total[0] > 50 and v_line(p) == [(V_LINE % tuple(total)).encode()]


def test_a_break_run_re_indexes_nothing(env, pair, tmp_path):
    bam, twin, by_name = pair
    flags = flags_of(CASE) + BREAK
    for sub in ("base", "fixed"):
        (tmp_path / sub).mkdir()
    cli(env, ["-i", twin, "-o", tmp_path / "base" / "out.fq", "--failed_out", tmp_path / "base" / "f.fq", *reports(tmp_path / "base"), *flags], 20000)
    d = tmp_path / "fixed"
    p = cli(env, ["-i", twin, "-o", d / "out.fq", "--failed_out", d / "f.fq", "--reindex_comments", "-V", *reports(d), *flags], 20000)
    want_out, so, _ = model((tmp_path / "base" / "out.fq").read_bytes(), by_name, True)
    want_failed, sf, _ = model((tmp_path / "base" / "f.fq").read_bytes(), by_name, True)
    assert (d / "out.fq").read_bytes() == want_out and (d / "f.fq").read_bytes() == want_failed
    assert b"\tMM:Z:" not in want_out and b"\tML:B:" not in want_out and b"\tmv:B:" not in want_out and want_out.count(b"\tRG:Z:run7_grp") > 100
    assert so[0] == 0 and so[1] > 100 and v_line(p) == [(V_LINE % tuple(a + b for a, b in zip(so, sf))).encode()]


def test_the_case_list_through_the_cli(env, tmp_path):
    """every shape of the case list as the CLI's readers hand it on (CRLF line ends, the long line, lines that are not tags), with
    nothing trimmed by the run itself except a fixed front and tail: the model says what comes out"""
    reads, _, _ = fc.case_list()
    reads = [r for r in reads if len(r[1]) >= 20]
    (tmp_path / "in.fq").write_bytes(fc.fastq(reads, fc.CRLF))
    p = cli(env, ["-i", tmp_path / "in.fq", "-o", tmp_path / "out.fq", "--reindex_comments", "-A", "-Q", "-L", "-n", "100", "-f", "3", "-t", "2", "-V",
                  *reports(tmp_path)], 50000)
    st = [0] * 5
    want = b"".join(fc.line_of(l, s, 3, len(s) - 5, True, st=st) + b"\n" + s[3:-2] + b"\n+\n" + q[3:-2] + b"\n" for l, s, q in reads)
    assert (tmp_path / "out.fq").read_bytes() == want
    assert v_line(p) == [(V_LINE % tuple(st)).encode()] and st[0] > 400 and st[1] > 30 and st[4] > 10


def test_the_device_s_gzip_form_is_not_taken_under_the_flag(tmp_path):
    """tests/stub_gz deflates text batches itself and logs every member: under the flag it must make none, and the file must inflate
    to the host's text"""
    build.build_host()
    lib = stub_gz_build.build()
    reads, _, _ = fc.case_list()
    reads = [r for r in reads if 20 <= len(r[1]) < 2000]
    (tmp_path / "in.fq").write_bytes(fc.fastq(reads))
    log = tmp_path / "gzlog"
    e = dict(os.environ, FPL_STUB_DEVICES="1", FPL_STUB_GZ_LOG=str(log))
    e["LD_LIBRARY_PATH"] = os.path.dirname(lib) + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    common = ["-i", tmp_path / "in.fq", "-A", "-Q", "-L", "-n", "100", "-f", "3", "-V", *reports(tmp_path)]
    cli(e, [*common, "-o", tmp_path / "plain.fq.gz"], 30000)
    assert log.exists() and len(log.read_text().splitlines()) >= 3  # (the stand-in is in use: without the flag it deflates)
    log.unlink()
    cli(e, [*common, "-o", tmp_path / "fixed.fq.gz", "--reindex_comments", "--device_gzip"], 30000)
    assert not log.exists() or log.read_text() == ""
    want = b"".join(fc.line_of(l, s, 3, len(s) - 3, True) + b"\n" + s[3:] + b"\n+\n" + q[3:] + b"\n" for l, s, q in reads)
    assert gzip.decompress((tmp_path / "fixed.fq.gz").read_bytes()) == want


def test_error_texts(env, pair, tmp_path):
    bam, twin, _ = pair
    rp = reports(tmp_path)
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.fq", "--reindex_comments", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --reindex_comments needs FASTQ input") and b"--comment_tags" in p.stderr
    for args in (["-o", tmp_path / "x.bam"], ["-o", tmp_path / "x.bam", "--failed_out", tmp_path / "y.bam"], []):
        p = cli(env, ["-i", twin, *args, "--reindex_comments", "-A"] + rp, ok=False)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --reindex_comments needs a FASTQ output")
    for i in (bam, twin):
        p = cli(env, ["-i", i, "-o", tmp_path / "x.fq", "--reindex_comments", "--comment_tags", "*", "-A"] + rp, ok=False)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --reindex_comments and --comment_tags exclude each other")
    # a .bam --out beside a FASTQ --failed_out: the records' names are cut at the first tab as ever, the text follows the flag
    d = tmp_path / "mixed"
    d.mkdir()
    cli(env, ["-i", twin, "-o", d / "o.bam", "--failed_out", d / "f.fq", "--reindex_comments", *reports(d), *flags_of(CASE)], 20000)
    names = [r[1] for r in bamio.parse((d / "o.bam").read_bytes())]
    assert len(names) > 100 and all(b"\t" not in n for n in names) and b"\tMM:Z:" in (d / "f.fq").read_bytes()
