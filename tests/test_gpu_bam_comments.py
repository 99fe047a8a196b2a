"""-m gpu: a BAM batch's auxiliary fields as comments behind the names of the FASTQ text the device composes (fpl_set_bam_comments;
csrc/bam_comments.h: k_bam_comment_tags, k_bam_comment_len, k_gz_layout_bam_comments, k_gz_compose_bam_comments) through
Engine.submit_bam in member and BGZF framing, Engine.submit_bgzf and the CLI on the real library.

The per-read records are the device's own, with the C3 options; what the output must hold for them is the model's answer
(tests/bam_comment_cases.py), and it must be the host form's (tests/test_host_bam_comments.py), byte for byte.  bam_comment_stats() is
the model's; with the switch off, or on and off again before the submission, the bytes are today's; a batch of BAM records
(FPL_GZIP_BAM) ignores the switch."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bam_comment_cases as cc
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc
from tests import bamio, hostio
from tests.bgzf_out_cases import STRIPE, check_blocks
from tests.test_bam_tags_emu import stream
from tests.test_gpu_bam_out import C3, engine_mod, new_engine, pinned  # noqa: F401
from tests.test_host_bam_comments import L, host_form  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the case list and reads with adapters that carry generated calls (C+mh? at CpGs, A+a. at every fourth A, a sparse N+n group),
    so that the device's own results hold split and front-trimmed reads; the input file and its twin arrays for the host's hook"""
    recs, _ = cc.case_list()
    rng = np.random.default_rng(12)
    seq, qual, off = synth.ont_like(160, seed=8, median_len=700, p_middle=0.3)
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        name = b"ont%d" % i
        occ = mc.occurrences(codes, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(codes) and codes[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(codes, b"A", 4, 3)),
                (b"N+n", mc.every(codes, b"N", 97, 11))]
        tags = mc.fields_of(codes, spec, rng, between=tc.P4 if i % 4 == 1 else tc.K1)
        recs.append((name, 0, codes, q, bamio.encode_record(name, 0, codes, q, tags=tags)))
    file = tc.input_bam(recs, header_text=tc.RG_HEADER)
    p = tmp_path_factory.mktemp("gpu_comments") / "in.bam"
    p.write_bytes(file)
    tseq, tqual, _, _ = bamio.twin_csr(file)
    return recs, file, p, np.ascontiguousarray(tseq), np.ascontiguousarray(tqual)


def submit_bam(engine_mod, case, sel, bgzf_framing=False, records=False, toggle=False):  # noqa: F811
    """-> (the batch's bytes, the device's records, bam_comment_stats())"""
    raw, starts, off = stream(case[0])
    eng = new_engine(engine_mod, C3, records, C=65536)
    if bgzf_framing:
        eng.set_gzip_framing(True)
    assert eng.bam_comment_stats() == (0, 0, 0, 0)
    eng.set_bam_comments(sel)
    if toggle:  # (on, then off again before the submission: the next submission decides)
        eng.set_bam_comments(None)
    res = np.zeros(len(starts), abi.RESULT_DTYPE)
    eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
    data = eng.wait()
    stats = eng.bam_comment_stats()
    eng.close()
    return data, res, stats


def check_text(data, want, bgzf_framing, label):
    if bgzf_framing:
        blocks = check_blocks(data, want, piece=STRIPE)  # (every block inflates on its own, to its stripe)
        assert len(blocks) == -(-len(want) // STRIPE) and all(len(b) <= 65536 for b in blocks)
    else:
        got = gzip.decompress(data)
        assert got == want, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
    print("%s: text %d, output %d" % (label, len(want), len(data)))


@pytest.mark.parametrize("name,bgzf_framing", [("all", False), ("all", True), ("mods", True), ("32", False)])
def test_submit_bam_equals_the_model_and_the_host_form(engine_mod, L, case, name, bgzf_framing):  # noqa: F811
    sel = cc.SELECTIONS[name]
    data, res, stats = submit_bam(engine_mod, case, sel, bgzf_framing)
    recs = case[0]
    want = cc.expected(recs, res, sel)
    # the device's own results hold a split read and a front-trimmed read that carry modifications
    ont = np.array([b"ont" in r[0] for r in recs if not r[1] & 0x900])
    assert ((res["n_frag"] == 2) & ont).any() and ((res["n_frag"] == 1) & (res["code"][:, 0] == 0) & (res["frag_start"][:, 0] > 0) & ont).any()
    check_text(data, want[0], bgzf_framing, "submit_bam %s" % name)
    assert list(stats) == want[2] and want[2][0] > 200 and want[2][1] > want[2][0]
    host = host_form(L, (recs, res, case[2], case[3], case[4]), sel, 3)
    assert host[0] == want[0] and host[2] == want[2]
    if name == "all":
        assert any(b"split-by-adapter-right-ont" in l and b"\tMM:Z:C+mh?," in l and b"\tML:B:C," in l for l in want[0].split(b"\n"))
        assert max(len(l) for l in want[0].split(b"\n")) > STRIPE + 16384 and want[2][3] >= 1


def test_submit_bgzf_equals_the_model(engine_mod, case):  # noqa: F811
    recs, file = case[0], case[1]
    eng = new_engine(engine_mod, C3, False, C=65536)
    eng.set_bam_comments(["MM", "ML", "MN", "qs", "RG"])
    desc, _ = bgzf.blocks(file)
    h, res, names, seq, qual, data = eng.submit_bgzf(pinned(eng, file), desc, skip=bgzf.header_len(file), gzip=True).wait()
    stats = eng.bam_comment_stats()
    eng.close()
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == len([r for r in recs if not r[1] & 0x900])
    want = cc.expected(recs, res, [b"MM", b"ML", b"MN", b"qs", b"RG"])
    check_text(data, want[0], False, "submit_bgzf")
    assert list(stats) == want[2] and want[2][0] > 200


def test_switch_off_gives_today_s_bytes_and_a_batch_of_bam_records_ignores_it(engine_mod, case):  # noqa: F811
    none = submit_bam(engine_mod, case, None)
    off_again = submit_bam(engine_mod, case, "*", toggle=True)
    nothing = submit_bam(engine_mod, case, cc.SELECTIONS["nothing"])
    assert none[0] == off_again[0] == nothing[0] and none[1].tobytes() == off_again[1].tobytes()
    assert none[2] == off_again[2] == nothing[2] == (0, 0, 0, 0)
    assert gzip.decompress(none[0]) == cc.expected(case[0], none[1], None)[0]  # today's form: the formatter's text
    records = submit_bam(engine_mod, case, None, records=True)
    with_switch = submit_bam(engine_mod, case, "*", records=True)
    assert records[0] == with_switch[0] and with_switch[2] == (0, 0, 0, 0) and records[0] != none[0]


def test_a_selection_that_is_none_is_refused(engine_mod):  # noqa: F811
    eng = new_engine(engine_mod, C3, False)
    too_many = ["a%c" % (65 + k) for k in range(26)] + ["b%d" % k for k in range(7)]  # 33 well-formed tags
    for bad in (["M_"], ["9M"], ["MM", "M\t"], too_many):
        with pytest.raises(engine_mod.FplError):
            eng.set_bam_comments(bad)
    eng.set_bam_comments(too_many[:32])
    eng.close()


def test_cli_device_form_equals_host_form(engine_mod, tmp_path, case):  # noqa: F811
    build.build_all()
    small = [r for r in case[0] if len(r[4]) < 20000 and not r[0].startswith((b"bad.", b"cut_behind_mm"))]
    (tmp_path / "in.bam").write_bytes(tc.input_bam(small, header_text=tc.RG_HEADER))
    flags = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]
    got = {}
    for name, extra in (("dev", ["--device_gzip"]), ("host", [])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([build.CLI, "-i", str(tmp_path / "in.bam"), "-o", str(d / "out.fastq.gz"), "--comment_tags", "*", "-V", "-j",
                            str(d / "o.json"), "-h", str(d / "o.html")] + flags + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, FPLH_CHUNK_BYTES="60000"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        n_dev = int(p.stderr.split(b"device gzip: ")[1].split()[0]) if b"device gzip: " in p.stderr else 0
        lines = [l for l in p.stderr.split(b"\n") if l.startswith(b"FASTQ comments: ")]
        assert len(lines) == 1 and (n_dev > 0) == bool(extra)
        got[name] = (gzip.decompress((d / "out.fastq.gz").read_bytes()), lines)
    assert got["dev"] == got["host"]
    n, fields, nbytes, left = (int(x) for x in got["dev"][1][0].split(b":")[1].replace(b",", b" ").split() if x.isdigit())
    assert n > 200 and fields > n and nbytes > 100000 and left >= 1 and got["dev"][0].count(b"\tMM:Z:") > 100
