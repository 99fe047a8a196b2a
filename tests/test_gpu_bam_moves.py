"""-m gpu: the move table mv and ts re-indexed in the trimmed and split BAM records the device composes (fpl_set_bam_moves;
csrc/bam_moves.h: k_bam_tags_moves, k_bam_moves_plan, k_bamout_compose_bam_moves) through Engine.submit_bam, Engine.submit_bgzf and
the CLI on the real library.

The per-read records are the device's own, with the C3 options; what the output must hold for them is the byte rule's answer
(tests/bam_move_cases.py), it must satisfy the decoder's property, and it must be the host form's (tests/test_host_bam_moves.py),
byte for byte.  bam_move_stats(), bam_mod_stats() and bam_tag_stats() are the model's; with the switch off, or with set_bam_moves
alone, the bytes are those of the forms before it; with set_bam_mods beside it each switch decides its own fields."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bam_mod_cases as mc
from tests import bam_move_cases as vc
from tests import bam_tag_cases as tc
from tests import bamio, hostio
from tests.test_bam_tags_emu import stream
from tests.test_gpu_bam_out import C3, engine_mod, hostlib, inflater, new_engine, pinned  # noqa: F401
from tests.test_gpu_bam_tags import check_tagged
from tests.test_host_bam_moves import L, host_form  # noqa: F401

pytestmark = pytest.mark.gpu


def make_recs():
    """the case list and reads with adapters that carry generated tables -- stride 6, 1 to 4 entries a base -- with ts and ns; a
    quarter of them carry modification calls beside the table, every eighth a move of 2"""
    out, _, _ = vc.case_list()
    rng = np.random.default_rng(14)
    seq, qual, off = synth.ont_like(160, seed=8, median_len=700, p_middle=0.3)
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        name = b"ont%d" % i
        mv = vc.table(len(codes), int(rng.integers(1, 5, len(codes)).sum()) + 2, rng, lead=2)
        if i % 8 == 5:
            mv[int(np.flatnonzero(mv == 0)[0])] = 2
        tags = vc.fields_of(mv, ts=((b"i", 10 + i), (b"S", 65000), (b"C", 250))[i % 3], order=("mt", "tm")[i % 2], pad=i % 16)
        if i % 4 == 2:
            occ = mc.occurrences(codes, b"C")
            cpg = [k for k, p in enumerate(occ) if p + 1 < len(codes) and codes[p + 1] == 4]
            tags += mc.fields_of(codes, [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(codes, b"A", 4, 3))], rng)
        out.append((name, 0, codes, q, bamio.encode_record(name, 0, codes, q, tags=tags)))
    return out


@pytest.fixture(scope="module")
def recs():
    return make_recs()


def not_hollow(recs, res, want):
    """the results hold a split read and a front-trimmed read that carry a table, and the model on them re-indexes, refuses, keeps
    and cuts (the counts: what the CPU oracle's records of the same reads give, with room)"""
    ont = np.array([b"ont" in r[0] for r in recs])
    assert ((res["n_frag"] == 2) & ont).any() and ((res["n_frag"] == 1) & (res["code"][:, 0] == 0) & (res["frag_start"][:, 0] > 0) & ont).any()
    assert want[6][0] > 150 and want[6][1] > 20 and want[6][2] > 100000 and want[6][3] > 10000, want[6]


def test_submit_bam_equals_host_form_and_model(engine_mod, L, inflater, tmp_path, recs):  # noqa: F811
    raw, starts, off = stream(recs)
    eng = new_engine(engine_mod, C3, True, C=65536)
    eng.set_bam_tags(True)
    eng.set_bam_moves(True)
    assert eng.bam_move_stats() == (0, 0, 0, 0)
    res = np.zeros(len(starts), abi.RESULT_DTYPE)
    eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
    data = eng.wait()
    move_stats, mod_stats, stats = eng.bam_move_stats(), eng.bam_mod_stats(), eng.bam_tag_stats()
    eng.close()
    want = vc.expected(recs, res)
    not_hollow(recs, res, want)
    for name, region, s, n, t in want[8]:
        vc.check_semantics(region, s, n, t)
    check_tagged(inflater, data, want[0], "submit_bam moves")
    assert list(move_stats) == want[6] and list(stats) == want[2] and mod_stats == (0, 0, 0, 0)
    host = host_form(L, tmp_path, recs, res, 3)
    assert host[0] == want[0] and host[2] == want[2] and host[6] == want[6]


def test_submit_bgzf_equals_the_model(engine_mod, inflater, recs):  # noqa: F811
    file = tc.input_bam(recs, header_text=tc.RG_HEADER)
    eng = new_engine(engine_mod, C3, True, C=65536)
    eng.set_bam_tags(True)
    eng.set_bam_moves(True)
    desc, _ = bgzf.blocks(file)
    h, res, names, seq, qual, data = eng.submit_bgzf(pinned(eng, file), desc, skip=bgzf.header_len(file), gzip=True).wait()
    move_stats, stats = eng.bam_move_stats(), eng.bam_tag_stats()
    eng.close()
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == len(recs)
    want = vc.expected(recs, res)
    check_tagged(inflater, data, want[0], "submit_bgzf moves")
    assert list(move_stats) == want[6] and list(stats) == want[2] and want[6][0] > 150
    for name, region, s, n, t in want[8]:
        vc.check_semantics(region, s, n, t)


def test_the_switches(engine_mod, L, inflater, tmp_path, recs):  # noqa: F811
    """switch off, and set_bam_moves without set_bam_tags: the bytes of the forms before it; both switches on: the combination"""
    raw, starts, off = stream(recs)
    outs = {}
    for key, tags, mods, moves in (("none", False, False, False), ("moves_alone", False, False, True), ("tags", True, False, False),
                                   ("off_again", True, False, None), ("mods", True, True, False), ("moves", True, False, True), ("both", True, True, True)):
        eng = new_engine(engine_mod, C3, True, C=65536)
        eng.set_bam_tags(tags)
        eng.set_bam_mods(mods)
        if moves is None:  # (on, then off again before the submission: the next submission decides)
            eng.set_bam_moves(True)
            eng.set_bam_moves(False)
        else:
            eng.set_bam_moves(moves)
        res = np.zeros(len(starts), abi.RESULT_DTYPE)
        eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
        outs[key] = (eng.wait(), res.tobytes(), eng.bam_tag_stats(), eng.bam_mod_stats(), eng.bam_move_stats())
        eng.close()
    zero = (0, 0, 0, 0)
    assert outs["none"] == outs["moves_alone"] and outs["none"][2:] == (zero, zero, zero)
    assert outs["tags"] == outs["off_again"] and outs["tags"][3:] == (zero, zero) and outs["tags"][0] != outs["none"][0]
    assert len({outs[k][0] for k in ("tags", "mods", "moves", "both")}) == 4 and len({outs[k][1] for k in outs}) == 1
    res = np.frombuffer(outs["tags"][1], abi.RESULT_DTYPE)
    want = tc.expected(recs, res)  # today's tagged form
    assert gzip.decompress(outs["tags"][0]) == want[0] and list(outs["tags"][2]) == want[2]
    want = mc.expected(recs, res)  # today's --keep_mods
    assert gzip.decompress(outs["mods"][0]) == want[0] and list(outs["mods"][2]) == want[2] and list(outs["mods"][3]) == want[4]
    assert outs["mods"][4] == zero
    want = vc.expected(recs, res, mods=True)
    check_tagged(inflater, outs["both"][0], want[0], "both switches")
    assert [list(x) for x in outs["both"][2:]] == [want[2], want[4], want[6]] and want[4][0] > 20
    host = host_form(L, tmp_path, recs, res, 3, mods=True)
    assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4] and host[6] == want[6]
    # a read with both kinds of fields keeps every field only under both switches
    assert want[2][0] > outs["moves"][2][0] and want[2][0] > outs["mods"][2][0]


def test_cli_device_form_equals_host_form(engine_mod, tmp_path, recs):  # noqa: F811
    build.build_all()
    small = [r for r in recs if len(r[4]) < 20000]
    (tmp_path / "moves.bam").write_bytes(tc.input_bam(small, header_text=tc.RG_HEADER))
    flags = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]
    got = {}
    for name, extra in (("dev", ["--device_gzip"]), ("host", [])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([build.CLI, "-i", str(tmp_path / "moves.bam"), "-o", str(d / "out.bam"), "--keep_tags", "--keep_moves", "--keep_mods", "-V",
                            "-j", str(d / "o.json"), "-h", str(d / "o.html")] + flags + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=120, env=dict(os.environ, FPLH_CHUNK_BYTES="60000"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        n_dev = int(p.stderr.split(b"BAM records: BGZF blocks framed on the device: ")[1].split()[0])
        lines = [l for l in p.stderr.split(b"\n") if l.startswith((b"BAM tags: ", b"BAM modifications: ", b"BAM move tables: "))]
        assert len(lines) == 3 and (n_dev > 0) == bool(extra)
        got[name] = (gzip.decompress((d / "out.bam").read_bytes()), lines)
    assert got["dev"] == got["host"]
    done, dropped, kept, cut = (int(x) for x in re.findall(rb"\d+", got["dev"][1][2]))
    assert done > 150 and dropped > 20 and kept > 100000 and cut > 10000
