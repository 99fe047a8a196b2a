"""-m gpu: device output for --break / --mask runs (fpl_set_fragment_output): the fragment list ordered on the device
(csrc/frag_index.h), gzip members and BGZF blocks of text and BAM batches composed from it (k_gz_layout_frag / k_gz_compose_frag
and their BAM forms), the CSR form (fpl_emit_batch_device: k_emit_count_frag, k_emit_fill_frag, k_emit_mask), through Engine and
the CLI on the real library.

The expected bytes always come from the host formatter: the same batch goes through the CSR path of a second engine,
fpl_get_fragments gives its list, and fplh_format_batch_fragments writes the text for it.  The device's member is inflated with
zlib, gzip and libdeflate.  Every test asserts on the fetched list that the case it is named for occurred."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, build, synth
from tests import bamio
from tests import frag_cases as fc
from tests.gzcheck import inflate_all

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def hostlib():
    return fc.load_hostlib()


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


def make(engine_mod, okw, frag_out=True, C=8192):
    eng = engine_mod.Engine(abi.FplOptions.default(**okw), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=C)
    if frag_out:
        eng.set_fragment_output(True)
    return eng


def csr_lists(engine_mod, okw, reads):
    """the batch through fpl_process_batch_async on an engine without the switch -> records, sorted fragments, regions"""
    eng = make(engine_mod, okw, frag_out=False)
    seq, qual, off = fc.csr_of(reads)
    res = np.zeros(len(reads), abi.RESULT_DTYPE)
    if len(reads):
        eng.submit_host(seq, qual, off, res)
        eng.wait()
    frags, regs = eng.fragments()
    frags, regs = frags.copy(), regs.copy()
    eng.close()
    return res, frags, regs


def text_member(engine_mod, okw, reads, bgzf=False):
    """-> (the batch's gzip bytes, records, fragments as fetched behind the wait)"""
    eng = make(engine_mod, okw)
    if bgzf:
        eng.set_gzip_framing(True)
    text = fc.text_of(reads)
    buf = eng.pinned_array(max(len(text), 1))
    buf[:len(text)] = np.frombuffer(text, np.uint8)
    eng.submit_text(buf[:len(text)], gzip=True)
    info, res, lines, member = eng.wait_text()
    assert info["status"] == 0 and info["n_reads"] == len(reads)
    frags, regs = eng.fragments()
    out = member, res, frags.copy(), regs.copy(), eng.gzip_batches()
    eng.close()
    return out


def bam_of(reads, reverse=1):
    """the reads as BAM records (record `reverse` with flag 0x10) -> raw record stream, starts, records"""
    recs = []
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(fc.text_of(reads))):
        recs.append(bamio.reverse_record(name, codes, q) if i == reverse else (name, 0, codes, q))
    parts, starts, pos = [], [], 0
    for r in recs:
        b = bamio.encode_record(*r)
        starts.append(pos)
        parts.append(b)
        pos += len(b)
    return b"".join(parts), np.array(starts, np.uint64), recs


def bam_member(engine_mod, okw, reads):
    raw, starts, recs = bam_of(reads)
    twin = [tuple(bamio.twin_record(*r).split(b"\n")[:4]) for r in recs]
    eng = make(engine_mod, okw)
    off = fc.csr_of(twin)[2]
    res = np.zeros(len(recs), abi.RESULT_DTYPE)
    bam = eng.pinned_array(max(len(raw), 1))
    bam[:len(raw)] = np.frombuffer(raw, np.uint8)
    eng.submit_bam(bam[:len(raw)], starts, off, res=res, gzip=True)
    member = eng.wait()
    frags, regs = eng.fragments()
    out = member, res, frags.copy(), regs.copy(), twin
    eng.close()
    return out


def check_text(engine_mod, hostlib, tmp_path, okw, reads, bgzf=False):
    res0, frags0, regs0 = csr_lists(engine_mod, okw, reads)
    want = fc.host_format(hostlib, tmp_path, fc.text_of(reads), res0, frags0, regs0)
    member, res, frags, regs, n_gz = text_member(engine_mod, okw, reads, bgzf)
    assert res.tobytes() == res0.tobytes() and fc.normal(frags, regs) == fc.normal(frags0, regs0)
    if not want:
        assert member == b"" and n_gz == 0
    elif bgzf:
        fc.inflate_stripes(member, want)
    else:
        assert n_gz == 1 and inflate_all(member, len(want)) == want
    return res0, frags0, regs0, want


def assert_names(frags, want):
    ok = frags[frags["code"] == 0]
    assert ok["break_no"].max() >= 10 and b"@r9-" in want and b"@r10-" in want
    assert ((ok["kind"] == 1) & (ok["break_no"] > 0)).any() and ((ok["kind"] == 2) & (ok["break_no"] > 0)).any()
    assert b"@r1-\n" in want and b" " in want.split(b"\n")[0]


def assert_masks(frags, regs, want):
    ok = frags[(frags["code"] == 0) & (frags["region_count"] > 0)]
    assert len(ok) >= 3 and (frags["break_no"] > 0).any()
    assert any(int(regs[f["region_first"]]["start"]) == int(f["start"]) for f in ok)  # a masked stretch at output offset 0
    last = [regs[int(f["region_first"]) + int(f["region_count"]) - 1] for f in ok]
    assert any(int(g["start"] + g["len"]) == int(f["start"] + f["len"]) for f, g in zip(ok, last))
    assert any(f["region_count"] >= 2 and int(regs[f["region_first"]]["start"] + regs[f["region_first"]]["len"]) ==
               int(regs[int(f["region_first"]) + 1]["start"]) for f in ok)
    whole = frags[frags["read"] == 3]
    assert len(whole) == 1 and whole[0]["code"] != 0 and int(regs[whole[0]["region_first"]]["len"]) == int(whole[0]["len"])
    assert b"@whole" not in want


def test_refusals_turn_into_output(engine_mod, hostlib, tmp_path):
    import torch

    reads = fc.masks_case()
    text = fc.text_of(reads)
    seq, qual, off = fc.csr_of(reads)
    for on in (True, False):
        eng = make(engine_mod, fc.BREAK_MASK, frag_out=on)
        buf = eng.pinned_array(len(text))
        buf[:] = np.frombuffer(text, np.uint8)
        st, qt = torch.from_numpy(seq.copy()).cuda(), torch.from_numpy(qual.copy()).cuda()
        ot = torch.from_numpy(off.astype(np.int64)).cuda()
        if on:
            eng.submit_text(buf, gzip=True)
            assert len(eng.wait_text()[3]) > 0
            assert eng.L.fpl_set_bam_gzip(eng.h, 1) == 0
            rt = eng.process_device(st, qt, ot, 8192)
            info = eng.emit_info(eng.emit_device(st, qt, ot, rt)[5])
            assert info["status"] == 0 and info["n_out"] > 0
            # the forms that stay with the host are refused while the switch is on
            assert eng.L.fpl_set_gzip_records(eng.h, abi.FPL_GZIP_BAM) == abi.FPL_ERR_STATE
            assert eng.L.fpl_set_bam_tags(eng.h, 1) == abi.FPL_ERR_STATE
            assert eng.L.fpl_set_bam_comments(eng.h, b"MM", 1) == abi.FPL_ERR_STATE
        else:
            with pytest.raises(engine_mod.FplError, match="invalid state"):
                eng.submit_text(buf, gzip=True)
            assert eng.L.fpl_set_bam_gzip(eng.h, 1) == abi.FPL_ERR_STATE
            rt = eng.process_device(st, qt, ot, 8192)
            with pytest.raises(engine_mod.FplError, match="invalid state"):
                eng.emit_device(st, qt, ot, rt)
        eng.close()
    # a context without the two options: the call succeeds and changes nothing
    eng = make(engine_mod, {}, frag_out=True)
    rt = eng.process_device(st, qt, ot, 8192)
    info = eng.emit_info(eng.emit_device(st, qt, ot, rt)[5])
    res = eng.results_to_numpy(rt, len(reads))
    passing = int(sum(int(r["code"][f]) == 0 for r in res if not r["dropped"] for f in range(int(r["n_frag"]))))
    assert info["status"] == 0 and info["n_out"] == passing > 0 and not hasattr(eng, "emit_break_no")
    eng.close()


def test_names(engine_mod, hostlib, tmp_path):
    res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, fc.BREAK_ONLY, fc.names_case())
    assert_names(frags, want)
    assert b"@r9-nine\n" in want and b"@r10-ten\n" in want and b"@r1-split-by-adapter-left-adapter in the middle\n" in want


def test_masks(engine_mod, hostlib, tmp_path):
    res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, fc.BREAK_MASK, fc.masks_case())
    assert_masks(frags, regs, want)


@pytest.mark.parametrize("lengths", [(1021,), (1022,), (1023,), (1024,), (1025,), (1021, 1022, 1023, 1024, 1025)])
def test_forced_cuts(engine_mod, hostlib, tmp_path, lengths):
    res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, fc.MASK_ONLY, fc.forced_case(lengths))
    assert len(frags) == len(lengths) and (frags["code"] == 0).all() and sorted(frags["len"].tolist()) == sorted(lengths)


def test_scans_and_stripes(engine_mod, hostlib, tmp_path):
    res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, fc.BREAK_ONLY, fc.scan_case(1100))
    assert len(frags) > 1024 and (frags["break_no"] > 0).all()
    res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, fc.BREAK_MASK, fc.stripes_case(), bgzf=True)
    assert len(want) > 3 * 49152 and (frags["region_count"] > 0).any()


def emit(engine_mod, okw, reads, res_in=None):
    """process_device + emit_device -> info, the output tensors as numpy, fragments, regions"""
    import torch

    seq, qual, off = fc.csr_of(reads)
    eng = make(engine_mod, okw)
    st = torch.from_numpy(np.append(seq, np.uint8(0))).cuda()[:len(seq)]
    qt = torch.from_numpy(np.append(qual, np.uint8(0))).cuda()[:len(seq)]
    ot = torch.from_numpy(off.astype(np.int64)).cuda()
    rt = eng.process_device(st, qt, ot, 8192)
    if res_in is not None:
        rt = torch.from_numpy(res_in.view(np.uint8).copy()).cuda()
    so, qo, oo, src, kind, info_t = eng.emit_device(st, qt, ot, rt)
    info = eng.emit_info(info_t)
    out = dict(info=info, off=oo.cpu().numpy(), src=src.cpu().numpy(), kind=kind.cpu().numpy(),
               break_no=eng.emit_break_no.cpu().numpy().view(np.uint16), seq=so.cpu().numpy().tobytes(), qual=qo.cpu().numpy().tobytes())
    frags, regs = eng.fragments()
    out["res"] = eng.results_to_numpy(rt, len(reads)).copy() if len(reads) else np.zeros(0, abi.RESULT_DTYPE)
    out["frags"], out["regs"] = frags.copy(), regs.copy()
    eng.close()
    return out


def check_csr(engine_mod, okw, reads, res_in=None):
    r = emit(engine_mod, okw, reads, res_in)
    off, src, kind, brk, seq, qual = fc.csr_slices(reads, r["res"], r["frags"], r["regs"])
    n = r["info"]["n_out"]
    assert r["info"]["status"] == 0 and n == len(src) and r["info"]["n_bytes"] == len(seq) and int(r["off"][0]) == 0
    assert r["off"][:n + 1].tolist() == off and r["src"][:n].tolist() == src and r["kind"][:n].tolist() == kind
    assert r["break_no"][:n].tolist() == brk
    assert r["seq"][:len(seq)] == seq and r["qual"][:len(seq)] == qual
    return r


def test_nothing(engine_mod, hostlib, tmp_path):
    for okw, reads in ((fc.BREAK_MASK, []), (fc.MASK_ONLY, fc.all_fail_case())):
        res, frags, regs, want = check_text(engine_mod, hostlib, tmp_path, okw, reads)
        assert want == b"" and (len(reads) == 0 or ((frags["code"] != 0).all() and len(frags) == len(reads)))
        r = check_csr(engine_mod, okw, reads)
        assert r["info"]["n_out"] == 0 and int(r["off"][0]) == 0
    # every read dropped: the caller's records say so
    reads = fc.masks_case()
    dropped = np.zeros(len(reads), abi.RESULT_DTYPE)
    dropped["dropped"] = 1
    r = check_csr(engine_mod, fc.BREAK_MASK, reads, res_in=dropped)
    assert r["info"]["n_out"] == 0 and int(r["off"][0]) == 0 and (r["frags"]["code"] == 0).any()


@pytest.mark.parametrize("case", ["names", "masks"])
def test_both_sources(engine_mod, hostlib, tmp_path, case):
    reads, okw = (fc.names_case(), fc.BREAK_ONLY) if case == "names" else (fc.masks_case(), fc.BREAK_MASK)
    member, res, frags, regs, twin = bam_member(engine_mod, okw, reads)
    res0, frags0, regs0 = csr_lists(engine_mod, okw, twin)
    assert res.tobytes() == res0.tobytes() and fc.normal(frags, regs) == fc.normal(frags0, regs0)
    want = fc.host_format(hostlib, tmp_path, fc.text_of(twin), res0, frags0, regs0)
    assert inflate_all(member, len(want)) == want
    if case == "names":
        assert_names(frags, want)
    else:
        assert_masks(frags, regs, want)


@pytest.mark.parametrize("case", ["names", "masks"])
def test_csr(engine_mod, case):
    reads, okw = (fc.names_case(), fc.BREAK_ONLY) if case == "names" else (fc.masks_case(), fc.BREAK_MASK)
    r = check_csr(engine_mod, okw, reads)
    ok = r["frags"][r["frags"]["code"] == 0]
    if case == "names":
        assert r["break_no"][:r["info"]["n_out"]].max() >= 10 and set(r["kind"][:r["info"]["n_out"]].tolist()) == {0, 1, 2}
    else:
        assert (ok["region_count"] > 0).any() and b"N" * 30 in r["seq"]


@pytest.mark.parametrize("how", ["chunks", "whole"])
def test_cli_device_gzip_reproduces_golden(tmp_path, how):
    """the golden --break / --mask case with -o out.fq.gz --device_gzip: cut into chunks the device parses them and deflates the
    fragments' text; the same run without the flag stays with the host, as before"""
    build.build_all()
    case = "c3_break_mask"
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    inp = tmp_path / "in.fq"
    inp.write_bytes(gzip.open(os.path.join(GOLD, case, "in.fq.gz")).read())
    env = dict(os.environ)
    if how == "chunks":
        env["FPLH_CHUNK_BYTES"] = "30000"
    said, parsed = b"gzip members deflated on the device", b"device parse:"
    for flag in (["--device_gzip"], []):
        out = tmp_path / ("out%d.fq.gz" % len(flag))
        cmd = [build.CLI, "-i", str(inp), "-o", str(out), "-j", str(tmp_path / "out.json"), "-h", str(tmp_path / "out.html"),
               "--reader_threads", "3", "-V"] + list(meta["flags"]) + flag
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert gzip.decompress(out.read_bytes()) == gzip.open(os.path.join(GOLD, case, "expected.out.fq.gz")).read()
        got = [l for l in (tmp_path / "out.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
        assert got == gzip.open(os.path.join(GOLD, case, "expected.json.gz")).read().split(b"\n")
        if flag and how == "chunks":
            assert said in p.stderr and parsed in p.stderr, p.stderr[-1500:]
        if not flag:
            assert said not in p.stderr and parsed not in p.stderr
