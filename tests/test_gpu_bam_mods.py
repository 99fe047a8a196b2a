"""-m gpu: MM / ML / MN re-indexed in the trimmed and split BAM records the device composes (fpl_set_bam_mods; csrc/bam_mods.h:
k_bam_tags_mods, k_bam_mods_plan, k_bamout_compose_bam_mods) through Engine.submit_bam, Engine.submit_bgzf and the CLI on the real
library.

The per-read records are the device's own, with the C3 options; what the output must hold for them is the byte rule's answer
(tests/bam_mod_cases.py), it must satisfy the decoder's property, and it must be the host form's (tests/test_host_bam_mods.py),
byte for byte.  bam_mod_stats() and bam_tag_stats() are the model's; with the switch off, or with set_bam_mods alone, the bytes
are those of the tagged form and of the untagged form."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bam_mod_cases as mc
from tests import bam_tag_cases as tc
from tests import bamio, hostio
from tests.test_bam_tags_emu import stream
from tests.test_gpu_bam_out import C3, engine_mod, hostlib, inflater, new_engine, pinned  # noqa: F401
from tests.test_gpu_bam_tags import check_tagged
from tests.test_host_bam_mods import L, host_form  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recs():
    """the case list and reads with adapters that carry generated calls: C+mh? at CpGs, A+a. at every fourth A, a sparse N+n group"""
    out, _, _ = mc.case_list()
    rng = np.random.default_rng(12)
    seq, qual, off = synth.ont_like(160, seed=8, median_len=700, p_middle=0.3)
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        name = b"ont%d" % i
        occ = mc.occurrences(codes, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(codes) and codes[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(codes, b"A", 4, 3)),
                (b"N+n", mc.every(codes, b"N", 97, 11))]
        tags = mc.fields_of(codes, spec, rng, between=tc.P4 if i % 4 == 1 else tc.K1)
        out.append((name, 0, codes, q, bamio.encode_record(name, 0, codes, q, tags=tags)))
    return out


def carries(rec):
    return b"ont" in rec[0]


def test_submit_bam_equals_host_form_and_model(engine_mod, L, inflater, tmp_path, recs):  # noqa: F811
    raw, starts, off = stream(recs)
    eng = new_engine(engine_mod, C3, True, C=65536)
    eng.set_bam_tags(True)
    eng.set_bam_mods(True)
    assert eng.bam_mod_stats() == (0, 0, 0, 0)
    res = np.zeros(len(starts), abi.RESULT_DTYPE)
    eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
    data = eng.wait()
    mod_stats, stats = eng.bam_mod_stats(), eng.bam_tag_stats()
    eng.close()
    want = mc.expected(recs, res)
    # the device's own results hold a split read and a front-trimmed read that carry modifications
    ont = np.array([carries(r) for r in recs])
    assert ((res["n_frag"] == 2) & ont).any() and ((res["n_frag"] == 1) & (res["code"][:, 0] == 0) & (res["frag_start"][:, 0] > 0) & ont).any()
    assert want[4][0] > 100 and want[4][1] > 10 and want[4][2] > 1000 and want[4][3] > 100
    for name, region, codes, s, n, t in want[6]:
        mc.check_semantics(region, codes, s, n, t)
    check_tagged(inflater, data, want[0], "submit_bam mods")
    assert list(mod_stats) == want[4] and list(stats) == want[2]
    host = host_form(L, tmp_path, recs, res, 3)
    assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4]


def test_submit_bgzf_equals_the_model(engine_mod, inflater, recs):  # noqa: F811
    file = tc.input_bam(recs, header_text=tc.RG_HEADER)
    eng = new_engine(engine_mod, C3, True, C=65536)
    eng.set_bam_tags(True)
    eng.set_bam_mods(True)
    desc, _ = bgzf.blocks(file)
    h, res, names, seq, qual, data = eng.submit_bgzf(pinned(eng, file), desc, skip=bgzf.header_len(file), gzip=True).wait()
    mod_stats, stats = eng.bam_mod_stats(), eng.bam_tag_stats()
    eng.close()
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == len(recs)
    want = mc.expected(recs, res)
    check_tagged(inflater, data, want[0], "submit_bgzf mods")
    assert list(mod_stats) == want[4] and list(stats) == want[2] and want[4][0] > 100
    for name, region, codes, s, n, t in want[6]:
        mc.check_semantics(region, codes, s, n, t)


def test_switch_off_gives_the_tagged_form_and_mods_alone_the_untagged(engine_mod, recs):  # noqa: F811
    raw, starts, off = stream(recs)
    outs = {}
    for key, tags, mods in (("none", False, False), ("mods_alone", False, True), ("tags", True, False), ("off_again", True, None), ("both", True, True)):
        eng = new_engine(engine_mod, C3, True, C=65536)
        eng.set_bam_tags(tags)
        if mods is None:  # (on, then off again before the submission: the next submission decides)
            eng.set_bam_mods(True)
            eng.set_bam_mods(False)
        else:
            eng.set_bam_mods(mods)
        res = np.zeros(len(starts), abi.RESULT_DTYPE)
        eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
        outs[key] = (eng.wait(), res.tobytes(), eng.bam_tag_stats(), eng.bam_mod_stats())
        eng.close()
    assert outs["none"] == outs["mods_alone"] and outs["none"][2:] == ((0, 0, 0, 0), (0, 0, 0, 0))
    assert outs["tags"] == outs["off_again"] and outs["tags"][3] == (0, 0, 0, 0) and outs["tags"][0] != outs["none"][0]
    assert outs["both"][0] != outs["tags"][0] and outs["both"][1] == outs["tags"][1]
    res = np.frombuffer(outs["tags"][1], abi.RESULT_DTYPE)
    want = tc.expected(recs, res)  # today's tagged form
    assert gzip.decompress(outs["tags"][0]) == want[0] and list(outs["tags"][2]) == want[2]


def test_cli_device_form_equals_host_form(engine_mod, tmp_path, recs):  # noqa: F811
    build.build_all()
    small = [r for r in recs if len(r[4]) < 20000]
    (tmp_path / "mods.bam").write_bytes(tc.input_bam(small, header_text=tc.RG_HEADER))
    flags = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]
    got = {}
    for name, extra in (("dev", ["--device_gzip"]), ("host", [])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([build.CLI, "-i", str(tmp_path / "mods.bam"), "-o", str(d / "out.bam"), "--keep_tags", "--keep_mods", "-V", "-j",
                            str(d / "o.json"), "-h", str(d / "o.html")] + flags + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, FPLH_CHUNK_BYTES="60000"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        n_dev = int(p.stderr.split(b"BAM records: BGZF blocks framed on the device: ")[1].split()[0])
        lines = [l for l in p.stderr.split(b"\n") if l.startswith(b"BAM tags: ") or l.startswith(b"BAM modifications: ")]
        assert len(lines) == 2 and (n_dev > 0) == bool(extra)
        got[name] = (gzip.decompress((d / "out.bam").read_bytes()), lines)
    assert got["dev"] == got["host"]
    done, dropped, kept, cut = (int(x) for x in re.findall(rb"\d+", got["dev"][1][1]))
    assert done > 50 and dropped > 5 and kept > 1000 and cut > 100
