"""bin/fastplong_amd --keep_moves on a box without GPUs, against tests/stub_bam/libfastplong_amd.so (the CPU stand-in with the BAM
entry points; it has none of fpl_set_gzip_records, fpl_set_bam_tags, fpl_set_bam_moves, so the host writes every record).  As in
tests/test_cli_bam_mods_stub.py the expected files come from the plain-Python rule (tests/bam_move_cases.py) applied to what the
SAME run writes as FASTQ text: every output read is found again by its name, its range in its read by looking its bases and
qualities up there."""
import numpy as np
import pytest

from tests import bam_mod_cases as mc
from tests import bam_move_cases as vc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.test_cli_bam_tags_stub import BREAK, CASE, NAME, cli, env, model as tag_model, read_bam, reports  # noqa: F401 (env: a fixture)
from tests.test_cli_gz_stub import flags_of, gold


@pytest.fixture(scope="module")
def moved(tmp_path_factory):
    """the golden reads as a basecaller's BAM: a generated move table of stride 6 with 1 to 4 entries a base, ts and ns; every third
    record with modification calls beside it; every ninth stored reversed (never re-indexable), every eleventh with a move of 2,
    every thirteenth with a ts:C that a trim widens"""
    rng = np.random.default_rng(9)
    recs = []
    for i, (_, _, codes, qual) in enumerate(bamio.fastq_to_records(gold(CASE, "in.fq.gz"))):
        name = b"q%d" % i
        n, f, c, q = bamio.reverse_record(name, codes, qual) if i % 9 == 4 else (name, 0x4, codes, qual)
        m = int(rng.integers(1, 5, len(c)).sum()) + 3
        mv = vc.table(len(c), m, rng, lead=3)
        if i % 11 == 7:
            mv[int(np.flatnonzero(mv == 0)[0])] = 2
        tags = vc.fields_of(mv, ts=(b"C", 250) if i % 13 == 5 else (b"i", 10 + i), order=("mt", "tm")[i % 2], pad=i % 16)
        if i % 3 == 0:
            tags += mc.fields_of(c, [(b"C+m?", mc.every(c, b"C", 3)), (b"A+a.", mc.every(c, b"A", 4, 3))], rng)
        recs.append((n, f, c, q, bamio.encode_record(n, f, c, q, tags=tags)))
    p = tmp_path_factory.mktemp("moved") / "moved.bam"
    p.write_bytes(tc.input_bam(recs, header_text=tc.RG_HEADER, block=7000))
    return p, {r[0]: r for r in recs}


def model(text, by_name, mods=False):
    """the records of a run's FASTQ text under --keep_moves -> (record bytes, tag stats[:3], move stats, re-indexed records)"""
    out, st, vs, done = [], [0, 0, 0], [0, 0, 0, 0], []
    for line, seq, qual in bc.fastq_records(text):
        name, flag, codes, in_qual, enc = by_name[NAME.match(line).group(1)]
        region = tc.aux_region(enc)
        changed = bool(flag & 0x10) or len(seq) != len(codes) or b"split-by-adapter-" in line
        if changed:
            s = 0
            if seq and not flag & 0x10:  # (an empty piece keeps no entry wherever it lies)
                full, full_q = bytes(bamio.CODES[x] for x in codes), bytes(v + 33 for v in in_qual)
                at = [k for k in range(len(full) - len(seq) + 1) if full[k:k + len(seq)] == seq and full_q[k:k + len(seq)] == qual]
                assert len(at) == 1, line  # (the piece, bases and qualities, lies in its read exactly once)
                s = at[0]
            t, lost, _, vv = vc.tags_of(region, codes, flag, s, len(seq), mods, True)
            if vv[0]:
                vs[0], vs[2], vs[3] = vs[0] + 1, vs[2] + vv[1], vs[3] + vv[2]
                done.append((region, s, len(seq), t))
            else:
                vs[1] += 1
        else:
            t, lost = tc.pick(region, False), False
        out.append(tc.with_tags(bc.record(line, seq, qual), t))
        st[1 if lost else 0] += 1
        st[2] += len(t)
    return b"".join(out), st, vs, done


def test_error_texts(env, moved, tmp_path):
    bam, _ = moved
    rp = reports(tmp_path)
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.bam", "--keep_moves", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --keep_moves needs --keep_tags")
    p = cli(env, ["-i", bam, "-o", tmp_path / "x.fq", "--keep_moves", "--keep_tags", "-A"] + rp, ok=False)
    assert p.returncode == 255 and p.stderr.startswith(b"ERROR: --keep_tags needs an output whose name ends in .bam")


@pytest.mark.parametrize("chunk", [None, 20000])
def test_out_and_failed_out_equal_the_model(env, moved, tmp_path, chunk):
    bam, by_name = moved
    flags = flags_of(CASE)
    for sub in ("fq", "moves", "both", "tags"):
        (tmp_path / sub).mkdir()
    d = tmp_path / "fq"
    cli(env, ["-i", bam, "-o", d / "out.fq", "--failed_out", d / "failed.fq", *reports(d), *flags], chunk)
    text, failed = (d / "out.fq").read_bytes(), (d / "failed.fq").read_bytes()
    want_out, so, vo, done = model(text, by_name)
    want_failed, sf, vf, done_f = model(failed, by_name)
    hdr = tc.header_raw(tc.RG_HEADER)
    d = tmp_path / "moves"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "--keep_moves", "-V", *reports(d), *flags], chunk)
    assert read_bam(d / "out.bam", hdr) == want_out and read_bam(d / "f.bam", hdr) == want_failed
    # split reads, trimmed reads and failed reads were re-indexed, entries were kept and cut, and records were refused
    assert vo[0] > 50 and vo[1] > 10 and vo[2] > 1000 and vo[3] > 100 and vf[0] > 0 and text.count(b"split-by-adapter-right-") > 5
    for region, s, n, t in done + done_f:
        vc.check_semantics(region, s, n, t)
    line = "BAM move tables: %d records re-indexed, %d not re-indexable and dropped, %d entries kept, %d cut away" % tuple(
        a + b for a, b in zip(vo, vf))
    assert line.encode() in p.stderr and b"BAM modifications" not in p.stderr
    line = "BAM tags: %d records kept every field, %d lost positional fields (MM, ML, MN, B arrays), %d bytes" % tuple(a + b for a, b in zip(so, sf))
    assert line.encode() in p.stderr
    # with --keep_mods beside it a record that carries both keeps every field: the tag line says so
    d = tmp_path / "both"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "--keep_moves", "--keep_mods", "-V", *reports(d), *flags],
            chunk)
    both_out, bo, bvo, _ = model(text, by_name, mods=True)
    both_failed, bf, bvf, _ = model(failed, by_name, mods=True)
    assert read_bam(d / "out.bam", hdr) == both_out != want_out and read_bam(d / "f.bam", hdr) == both_failed
    assert (bvo, bvf) == (vo, vf) and line.encode() not in p.stderr and bo[0] > so[0] and b"BAM modifications: " in p.stderr
    line = "BAM tags: %d records kept every field, %d lost positional fields (MM, ML, MN, B arrays), %d bytes" % tuple(a + b for a, b in zip(bo, bf))
    assert line.encode() in p.stderr
    # --keep_tags alone on the same input: the bytes it has always written, and no word of move tables
    d = tmp_path / "tags"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--failed_out", d / "f.bam", "--keep_tags", "-V", *reports(d), *flags], chunk)
    old_out, old_failed = tag_model(text, by_name, False)[0], tag_model(failed, by_name, False)[0]
    assert read_bam(d / "out.bam", hdr) == old_out != want_out and read_bam(d / "f.bam", hdr) == old_failed
    assert b"BAM move tables" not in p.stderr
    js = lambda x: [l for l in (tmp_path / x / "o.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]  # noqa: E731
    assert js("tags") == js("moves") == js("both") == js("fq")


def test_a_break_run_re_indexes_nothing(env, moved, tmp_path):
    bam, by_name = moved
    flags = flags_of(CASE) + BREAK
    for sub in ("moves", "tags"):
        (tmp_path / sub).mkdir()
    d = tmp_path / "moves"
    p = cli(env, ["-i", bam, "-o", d / "out.bam", "--keep_tags", "--keep_moves", "-V", *reports(d), *flags], 20000)
    cli(env, ["-i", bam, "-o", tmp_path / "tags" / "out.bam", "--keep_tags", *reports(tmp_path / "tags"), *flags], 20000)
    assert (d / "out.bam").read_bytes() == (tmp_path / "tags" / "out.bam").read_bytes()
    n = len(bamio.parse((d / "out.bam").read_bytes()))
    assert n > 100 and b"BAM move tables: 0 records re-indexed, %d not re-indexable and dropped, 0 entries kept, 0 cut away" % n in p.stderr
