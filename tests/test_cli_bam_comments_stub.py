"""bin/fastplong_amd --comment_tags on a box without GPUs, against tests/stub_bam/libfastplong_amd.so (the CPU stand-in with the BAM
entry points; it has no fpl_set_bam_comments, so the host formats every batch).  As in tests/test_cli_bam_mods_stub.py the expected
files come from the plain-Python model (tests/bam_comment_cases.py) applied to what the SAME run writes without the flag: every
output read is found again by its name, its range in its read by looking its bases and qualities up there."""
import gzip
import os

import pytest

from tests import bam_comment_cases as cc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.bgzf_out_cases import split_blocks
from tests.test_cli_bam_mods_stub import model as mod_model, modded  # noqa: F401 (modded: a fixture)
from tests.test_cli_bam_tags_stub import BREAK, CASE, NAME, cli, env, read_bam, reports  # noqa: F401 (env: a fixture)
from tests.test_cli_gz_stub import flags_of

V_LINE = "FASTQ comments: %d records, %d fields, %d bytes, %d fields left out (control bytes)"


def model(text, by_name, sel, fragment_mode=False):
    """a run's FASTQ text as the same run writes it under --comment_tags -> (text, the four counts)"""
    out, st = [], [0] * 4
    lines = text.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    for k in range(0, len(lines) - 1, 4):
        line, seq, plus, qual = lines[k:k + 4]
        name, flag, codes, in_qual, enc = by_name[NAME.match(line).group(1)]
        region = tc.aux_region(enc)
        changed = fragment_mode or bool(flag & 0x10) or len(seq) != len(codes) or b"split-by-adapter-" in line
        s = 0
        if changed and seq and not flag & 0x10 and not fragment_mode:  # (where re-indexing can apply, the piece's place matters)
            full, full_q = bytes(bamio.CODES[x] for x in codes), bytes(v + 33 for v in in_qual)
            at = [j for j in range(len(full) - len(seq) + 1) if full[j:j + len(seq)] == seq and full_q[j:j + len(seq)] == qual]
            assert len(at) == 1, line
            s = at[0]
        c, n, left = cc.comment(cc.tag_bytes_of(region, codes, flag, s, len(seq), changed, fragment_mode), sel)
        cc.note(st, c, n, left)
        out.append(b"\n".join((line + c, seq, plus, qual)) + b"\n")
    return b"".join(out), st


def v_line(p):
    return [l for l in p.stderr.split(b"\n") if l.startswith(b"FASTQ comments:")]


def js(d):
    return [l for l in (d / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]


@pytest.fixture(scope="module")
def base(env, modded, tmp_path_factory):
    """the run without the flag, once: --out and --failed_out as plain text, several batches"""
    bam, by_name = modded
    d = tmp_path_factory.mktemp("base")
    p = cli(env, ["-i", bam, "-o", d / "out.fq", "--failed_out", d / "failed.fq", "-V", *reports(d), *flags_of(CASE)], 20000)
    assert int(p.stderr.split(b"host pipeline: ")[1].split()[0]) >= 4 and not v_line(p)
    return (d / "out.fq").read_bytes(), (d / "failed.fq").read_bytes(), js(d)


@pytest.mark.parametrize("form,sel", [("fq", "*"), ("gz", "MM,ML"), ("bgzf", "*"), ("fq", "qs,MN,RG"), ("gz", "Zq")])
def test_out_and_failed_out_equal_the_model(env, modded, base, tmp_path, form, sel):
    bam, by_name = modded
    text, failed, base_js = base
    want_sel = "*" if sel == "*" else [t.encode() for t in sel.split(",")]
    want_out, so = model(text, by_name, want_sel)
    want_failed, sf = model(failed, by_name, want_sel)
    ext = "fq" if form == "fq" else "fq.gz"
    extra = ["--bgzf"] if form == "bgzf" else []
    p = cli(env, ["-i", bam, "-o", tmp_path / ("out." + ext), "--failed_out", tmp_path / ("failed." + ext), "--comment_tags", sel, "-V",
                  *extra, *reports(tmp_path), *flags_of(CASE)], 20000)
    raw_out, raw_failed = (tmp_path / ("out." + ext)).read_bytes(), (tmp_path / ("failed." + ext)).read_bytes()
    if form == "bgzf":
        assert len(split_blocks(raw_out, eof=True)) >= 4
    got_out, got_failed = (raw_out, raw_failed) if form == "fq" else (gzip.decompress(raw_out), gzip.decompress(raw_failed))
    assert got_out == want_out and got_failed == want_failed
    assert v_line(p) == [(V_LINE % tuple(a + b for a, b in zip(so, sf))).encode()]
    assert js(tmp_path) == base_js
    if sel == "*":  # split, trimmed and failed reads carry re-indexed fields, reversed ones have lost theirs
        assert so[0] > 100 and sf[0] > 5 and want_out.count(b"\tMM:Z:") > 50 and want_failed.count(b"\tML:B:C") > 0
        assert any(b"split-by-adapter-right-" in l and b"\tMM:Z:" in l for l in want_out.split(b"\n"))
        assert want_out.count(b"\tmv:B:c,5,1,0,1,1,0") > 0 and want_out.count(b"\tqs:f:17.25") > 50
    if sel == "Zq":
        assert got_out == text and so == sf == [0] * 4


@pytest.mark.parametrize("gz", [False, True])
def test_split_files_equal_the_model(env, modded, tmp_path, gz):
    bam, by_name = modded
    name = "o.fq.gz" if gz else "o.fq"
    files = {}
    for sub, extra in (("base", []), ("notes", ["--comment_tags", "*", "-V"])):
        d = tmp_path / sub
        d.mkdir()
        p = cli(env, ["-i", bam, "-o", d / name, "--split", "3", *extra, *reports(d), *flags_of(CASE)], 20000)
        files[sub] = {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.endswith(name)}
    assert len(files["base"]) == 3 and sorted(files["base"]) == sorted(files["notes"])
    total = [0] * 4
    for f, raw in files["base"].items():
        want, st = model(gzip.decompress(raw) if gz else raw, by_name, "*")
        got = files["notes"][f]
        assert (gzip.decompress(got) if gz else got) == want
        total = [a + b for a, b in zip(total, st)]
    assert total[0] > 100 and v_line(p) == [(V_LINE % tuple(total)).encode()]
    assert js(tmp_path / "base") == js(tmp_path / "notes")


def test_stdout(env, modded, base, tmp_path):
    bam, by_name = modded
    p = cli(env, ["-i", bam, "--stdout", "--comment_tags", "MM,ML,MN", *reports(tmp_path), *flags_of(CASE)], 20000)
    assert p.stdout == model(base[0], by_name, [b"MM", b"ML", b"MN"])[0]


def test_a_break_run_re_indexes_nothing(env, modded, tmp_path):
    bam, by_name = modded
    flags = flags_of(CASE) + BREAK
    for sub in ("base", "notes"):
        (tmp_path / sub).mkdir()
    cli(env, ["-i", bam, "-o", tmp_path / "base" / "out.fq", "--failed_out", tmp_path / "base" / "f.fq", *reports(tmp_path / "base"), *flags], 20000)
    d = tmp_path / "notes"
    p = cli(env, ["-i", bam, "-o", d / "out.fq", "--failed_out", d / "f.fq", "--comment_tags", "*", "-V", *reports(d), *flags], 20000)
    want_out, so = model((tmp_path / "base" / "out.fq").read_bytes(), by_name, "*", True)
    want_failed, sf = model((tmp_path / "base" / "f.fq").read_bytes(), by_name, "*", True)
    assert (d / "out.fq").read_bytes() == want_out and (d / "f.fq").read_bytes() == want_failed
    assert b"\tMM:Z:" not in want_out and b"\tML:B:" not in want_out and b"\tmv:B:" not in want_out and want_out.count(b"\tRG:Z:run7_grp") > 100
    assert v_line(p) == [(V_LINE % tuple(a + b for a, b in zip(so, sf))).encode()]


def test_a_bam_failed_out_beside_a_fastq_out_each_by_its_own_rule(env, modded, base, tmp_path):
    bam, by_name = modded
    text, failed, _ = base
    p = cli(env, ["-i", bam, "-o", tmp_path / "out.fq.gz", "--failed_out", tmp_path / "f.bam", "--keep_tags", "--keep_mods", "--comment_tags", "MM,ML", "-V",
                  *reports(tmp_path), *flags_of(CASE)], 20000)
    want, so = model(text, by_name, [b"MM", b"ML"])
    assert gzip.decompress((tmp_path / "out.fq.gz").read_bytes()) == want
    assert read_bam(tmp_path / "f.bam", tc.header_raw(tc.RG_HEADER)) == mod_model(failed, by_name)[0]
    assert v_line(p) == [(V_LINE % tuple(so)).encode()] and b"BAM modifications: " in p.stderr


def test_error_texts(env, modded, tmp_path):
    bam, _ = modded
    fq = tmp_path / "in.fq"
    fq.write_bytes(b"@r\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    rp = reports(tmp_path)
    p = cli(env, ["-i", fq, "-o", tmp_path / "x.fq", "--comment_tags", "*", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --comment_tags needs BAM input")
    for args in (["-o", tmp_path / "x.bam"], ["-o", tmp_path / "x.bam", "--failed_out", tmp_path / "y.bam", "--keep_tags"], []):
        p = cli(env, ["-i", bam, *args, "--comment_tags", "*", "-A"] + rp, ok=False)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --comment_tags needs a FASTQ output")
    for bad in ("", "M", "MM,", "MM;ML", "mm,9x", ",".join("a%d" % (k % 10) + "" for k in range(10)) + "," + ",".join(t.decode() for t in cc.TAGS_32[:23])):
        p = cli(env, ["-i", bam, "-o", tmp_path / "x.fq", "--comment_tags", bad, "-A"] + rp, ok=False)
        assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --comment_tags takes * or a list"), bad
    # a record whose fields do not parse ends the run under the flag, as under --keep_tags, and only under it
    recs = [(b"g%d" % i, 4, bytes([1, 2, 4, 8] * 50), bytes([30] * 200)) for i in range(30)]
    recs = [(n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.MALFORMED["z_without_nul"][0] if i == 17 else tc.K1)) for i, (n, f, c, q) in enumerate(recs)]
    (tmp_path / "bad.bam").write_bytes(tc.input_bam(recs))
    p = cli(env, ["-i", tmp_path / "bad.bam", "-o", tmp_path / "o.fq", "--comment_tags", "*", "-A"] + rp, ok=False)
    assert b"ERROR: BAM record 17 (g17): the auxiliary fields do not parse" in p.stderr
    cli(env, ["-i", tmp_path / "bad.bam", "-o", tmp_path / "o.fq", "-A", "-Q", "-L", "-n", "100"] + rp)
    # --keep_tags and --keep_mods keep their error texts beside the flag
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.fq", "--keep_tags", "--comment_tags", "*", "-A"] + rp, ok=False)
    assert p.stderr.startswith(b"ERROR: --keep_tags needs an output whose name ends in .bam")
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.bam", "--failed_out", tmp_path / "y.fq", "--keep_mods", "--comment_tags", "*", "-A"] + rp, ok=False)
    assert p.stderr.startswith(b"ERROR: --keep_mods needs --keep_tags")
