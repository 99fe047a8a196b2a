"""bin/fastplong_amd --keep_mods on a box without GPUs, against tests/stub_bam/libfastplong_amd.so (the CPU stand-in with the BAM
entry points; it has none of fpl_set_gzip_records, fpl_set_bam_tags, fpl_set_bam_mods, so the host writes every record).  As in
tests/test_cli_bam_tags_stub.py the expected files come from the plain-Python rule (tests/bam_mod_cases.py) applied to what the
SAME run writes as FASTQ text: every output read is found again by its name, its range in its read by looking its bases and qualities up there."""
import numpy as np
import pytest

from tests import bam_mod_cases as mc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.test_cli_bam_tags_stub import BREAK, CASE, NAME, cli, env, model as tag_model, read_bam, reports  # noqa: F401 (env: a fixture)
from tests.test_cli_gz_stub import flags_of, gold


@pytest.fixture(scope="module")
def modded(tmp_path_factory):
    """the golden reads as a BAM with generated modification calls: 5mC / 5hmC at every CpG, 6mA at every fourth A, a sparse N group;
    every ninth record stored reversed (never re-indexable), every eleventh with an ML one value short, some with a move table"""
    rng = np.random.default_rng(8)
    recs = []
    for i, (_, _, codes, qual) in enumerate(bamio.fastq_to_records(gold(CASE, "in.fq.gz"))):
        name = b"q%d" % i
        n, f, c, q = bamio.reverse_record(name, codes, qual) if i % 9 == 4 else (name, 0x4, codes, qual)
        occ = mc.occurrences(c, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(c) and c[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(c, b"A", 4, 3)),
                (b"N+n", mc.every(c, b"N", 211, 50))]
        tags = mc.fields_of(c, spec, rng, between=tc.P4 if i % 4 == 1 else tc.K1)
        if i % 11 == 7:
            tags = tc.K1 + mc.mm_field(spec) + mc.ml_field([1] * (sum(len(d) * mc.k_of(h) for h, d in spec) - 1))
        recs.append((n, f, c, q, bamio.encode_record(n, f, c, q, tags=tags)))
    p = tmp_path_factory.mktemp("modded") / "modded.bam"
    p.write_bytes(tc.input_bam(recs, header_text=tc.RG_HEADER, block=7000))
    return p, {r[0]: r for r in recs}


def model(text, by_name):
    """the records of a run's FASTQ text under --keep_mods -> (record bytes, tag stats[:3], mod stats, re-indexed records)"""
    out, st, ms, done = [], [0, 0, 0], [0, 0, 0, 0], []
    for line, seq, qual in bc.fastq_records(text):
        name, flag, codes, in_qual, enc = by_name[NAME.match(line).group(1)]
        region = tc.aux_region(enc)
        changed = bool(flag & 0x10) or len(seq) != len(codes) or b"split-by-adapter-" in line
        if changed:
            s = 0
            if seq and not flag & 0x10:  # (an empty piece keeps no position wherever it lies)
                full, full_q = bytes(bamio.CODES[x] for x in codes), bytes(v + 33 for v in in_qual)
                at = [k for k in range(len(full) - len(seq) + 1) if full[k:k + len(seq)] == seq and full_q[k:k + len(seq)] == qual]
                assert len(at) == 1, line  # (the piece, bases and qualities, lies in its read exactly once)
                s = at[0]
            t, re_indexed, kept, cut, lost = mc.rewrite(region, codes, flag, s, len(seq))
            if re_indexed:
                ms[0], ms[2], ms[3] = ms[0] + 1, ms[2] + kept, ms[3] + cut
                done.append((region, codes, s, len(seq), t))
            else:
                ms[1] += 1
        else:
            t, lost = tc.pick(region, False), False
        out.append(tc.with_tags(bc.record(line, seq, qual), t))
        st[1 if lost else 0] += 1
        st[2] += len(t)
    return b"".join(out), st, ms, done


def test_error_texts(env, modded, tmp_path):
    bam, _ = modded
    rp = reports(tmp_path)
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.bam", "--keep_mods", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --keep_mods needs --keep_tags")
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.fq", "--keep_mods", "--keep_tags", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --keep_tags needs an output whose name ends in .bam")


@pytest.mark.parametrize("chunk", [None, 20000])
def test_out_and_failed_out_equal_the_model(env, modded, tmp_path, chunk):
    bam, by_name = modded
    flags = flags_of(CASE)
    for sub in ("fq", "mods", "tags"):
        (tmp_path / sub).mkdir()
    d = tmp_path / "fq"
    cli(env, ["-i", bam, "-o", d / "out.fq", "--failed_out", d / "failed.fq", *reports(d), *flags], chunk)
    text, failed = (d / "out.fq").read_bytes(), (d / "failed.fq").read_bytes()
    want_out, so, mo, done = model(text, by_name)
    want_failed, sf, mf, done_f = model(failed, by_name)
    hdr = tc.header_raw(tc.RG_HEADER)
    d = tmp_path / "mods"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "--keep_mods", "-V", *reports(d), *flags], chunk)
    assert read_bam(d / "out.bam", hdr) == want_out and read_bam(d / "f.bam", hdr) == want_failed
    # split reads, trimmed reads and failed reads were re-indexed, positions were kept and cut, and every cause of "not" was met
    assert mo[0] > 50 and mo[1] > 10 and mo[2] > 1000 and mo[3] > 100 and mf[0] > 0 and text.count(b"split-by-adapter-right-") > 5
    for region, codes, s, n, t in done + done_f:
        mc.check_semantics(region, codes, s, n, t)
    line = "BAM modifications: %d records re-indexed, %d not re-indexable and dropped, %d positions kept, %d cut away" % tuple(
        a + b for a, b in zip(mo, mf))
    assert line.encode() in p.stderr
    line = "BAM tags: %d records kept every field, %d lost positional fields (MM, ML, MN, B arrays), %d bytes" % tuple(a + b for a, b in zip(so, sf))
    assert line.encode() in p.stderr
    # --keep_tags alone on the same input: the bytes it has always written, and no word of modifications
    d = tmp_path / "tags"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "-V", *reports(d), *flags], chunk)
    old_out, old_failed = tag_model(text, by_name, False)[0], tag_model(failed, by_name, False)[0]
    assert read_bam(d / "out.bam", hdr) == old_out != want_out and read_bam(d / "f.bam", hdr) == old_failed
    assert b"BAM modifications" not in p.stderr
    js = lambda x: [l for l in (tmp_path / x / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    assert js("tags") == js("mods") == js("fq")


def test_a_break_run_re_indexes_nothing(env, modded, tmp_path):
    bam, by_name = modded
    flags = flags_of(CASE) + BREAK
    for sub in ("mods", "tags"):
        (tmp_path / sub).mkdir()
    d = tmp_path / "mods"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--keep_tags", "--keep_mods", "-V", *reports(d), *flags], 20000)
    cli(env, ["-i", bam, "-o", tmp_path / "tags" / "out.bam", "--keep_tags", *reports(tmp_path / "tags"), *flags], 20000)
    assert (d / "out.bam").read_bytes() == (tmp_path / "tags" / "out.bam").read_bytes()
    n = len(bamio.parse((d / "out.bam").read_bytes()))
    assert n > 100 and b"BAM modifications: 0 records re-indexed, %d not re-indexable and dropped, 0 positions kept, 0 cut away" % n in p.stderr
