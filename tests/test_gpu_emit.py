"""-m gpu: fpl_emit_batch_device through Engine.emit_device (csrc/emit.h): the passing, trimmed reads of a resident batch as a CSR
batch in device memory.  The hand-made cases of tests/emit_cases.py (the ones tests/test_emit_emu.py runs on the emulator) against
the numpy gather over the records, then batches that went through the pipeline: against the gather over the ORACLE's records,
against the host formatter's --out text, and as the input of a second context with nothing but the 32-byte info read back in
between.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from fastplong_amd import abi, synth
from tests import emit_cases as ec
from tests import hostio, parity
from tests.gzcheck import host_format, load_hostlib

pytestmark = pytest.mark.gpu

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
# fastplong_amd/csrc/emit.h: EM_LAYOUT_READS, EM_SCAN_BLOCKS, EM_TILE (tests/test_emit_emu.py reads them from the emulator build)
LAYOUT_READS, SCAN_BLOCKS, TILE = 256, 1024, 32768


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


@pytest.fixture(scope="module")
def eng(engine_mod):
    e = engine_mod.Engine(abi.FplOptions.default(), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=512)
    yield e
    e.close()


@pytest.fixture(scope="module")
def run(eng):
    """the backend of tests/emit_cases.py: Engine.emit_device over views of pattern-filled tensors"""
    import torch

    def dev(a, dtype=None):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        return t if dtype is None else t.view(dtype)

    def go(seq, qual, off, res, cap_bytes, cap_reads, shift, src=True, kind=True):
        st = dev(seq) if len(seq) else torch.zeros(1, dtype=torch.uint8, device="cuda")
        qt = dev(qual) if len(qual) else torch.zeros(1, dtype=torch.uint8, device="cuda")
        ot = dev(off.astype(np.int64), torch.int64)
        rt = dev(res) if len(res) else torch.zeros(36, dtype=torch.uint8, device="cuda")
        nb, nr = cap_bytes + ec.GUARD, cap_reads + ec.GUARD
        # (torch's blocks are 256-byte aligned: the arrays start `shift` bytes behind a 16-byte boundary)
        gs = torch.full((nb + 32,), ec.PAT, dtype=torch.uint8, device="cuda")[16 + shift:16 + shift + nb]
        gq = torch.full((nb + 32,), ec.PAT, dtype=torch.uint8, device="cuda")[shift:shift + nb]
        assert gs.data_ptr() % 16 == shift and gq.data_ptr() % 16 == shift
        goff = torch.full((nr + 1,), ec.PAT64, dtype=torch.int64, device="cuda")
        gsrc = torch.full((nr,), ec.PAT32 - 2 ** 32, dtype=torch.int32, device="cuda")
        gkind = torch.full((nr,), ec.PAT, dtype=torch.uint8, device="cuda")
        out = eng.emit_device(st, qt, ot, rt, seq_out=gs[:cap_bytes], qual_out=gq[:cap_bytes], off_out=goff[:cap_reads + 1],
                              src=gsrc[:cap_reads] if src else None, kind=gkind[:cap_reads] if kind else None)
        info = eng.emit_info(out[5])
        return (0, info, gs.cpu().numpy(), gq.cpu().numpy(), goff.cpu().numpy().view(np.uint64), gsrc.cpu().numpy().view(np.uint32),
                gkind.cpu().numpy())

    return go


def test_lengths_at_every_source_and_destination_alignment(run):
    seq, qual, off, res = ec.case_lengths_and_alignments(TILE)
    info, want = ec.check(run, seq, qual, off, res)
    s, d = ec.alignments(off, res, want)
    assert s == set(range(16)) and d == set(range(16)), (s, d)
    assert info["max_len"] == TILE + 1


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_output_arrays_at_any_address(run, shift):
    seq, qual, off, res = ec.case_tiles(TILE)
    ec.check(run, seq, qual, off, res, shift=shift)


def test_tiles_of_many_reads_and_a_read_over_many_tiles(run):
    seq, qual, off, res = ec.case_tiles(TILE)
    info, want = ec.check(run, seq, qual, off, res)
    woff = want[2]
    last = np.searchsorted(woff, TILE - 1, "right") - 1
    assert (np.diff(woff)[:last + 1] > 0).sum() == 5
    assert ((woff[1:] - 1) // TILE - woff[:-1] // TILE)[np.diff(woff) > 0].max() >= 3
    ec.check(run, seq, qual, off, res, spare_bytes=1000, spare_reads=5)


def test_an_output_shorter_than_sixteen_bytes(run):
    seq, qual, off, res = ec.case_tiny()
    info, _ = ec.check(run, seq, qual, off, res)
    assert info["n_bytes"] == 7 and info["n_out"] == 3


def test_record_kinds(run):
    seq, qual, off, res = ec.case_record_kinds()
    info, want = ec.check(run, seq, qual, off, res)
    assert info["n_out"] == 2 * (1 + 2 + 1 + 1 + 2)
    assert set(want[4].tolist()) == {0, 1, 2}


def test_every_read_fails_and_no_reads(run):
    seq, qual, off, res = ec.case_all_fail()
    info, _ = ec.check(run, seq, qual, off, res)
    assert info["n_out"] == 0 and info["n_bytes"] == 0
    z = np.zeros(0, np.uint8)
    rc, info, gs, gq, goff, gsrc, gkind = run(z, z, np.zeros(1, np.uint64), ec.records(0), 0, 0, 0)
    assert info == dict(n_bytes=0, n_out=0, max_len=0, status=0)
    assert goff[0] == 0 and (goff[1:] == np.uint64(ec.PAT64)).all() and (gs == ec.PAT).all()


def test_more_reads_than_a_layout_block_and_more_blocks_than_a_scan_step(run):
    seq, qual, off, res = ec.case_random(3 * LAYOUT_READS + 17, seed=31)
    ec.check(run, seq, qual, off, res)
    n = LAYOUT_READS * SCAN_BLOCKS + 2 * LAYOUT_READS + 5
    seq, qual, off, res = ec.case_random(n, seed=32)
    info, _ = ec.check(run, seq, qual, off, res, shift=3)
    assert info["n_out"] > n // 2


def test_a_window_past_its_read_is_refused(run):
    seq, qual, off, res = ec.case_random(700, seed=33)
    want = ec.reference(seq, qual, off, res)
    n_bytes, n_out = len(want[0]), len(want[3])
    lens = np.diff(off.astype(np.int64))
    i = int(np.nonzero((res["dropped"] == 0) & (res["n_frag"] == 2) & (res["code"][:, 1] == ec.PASS))[0][-1])
    bad = res.copy()
    bad["frag_start"][i, 1] = lens[i] - bad["frag_len"][i, 1] + 1  # one byte past the read's end
    assert ec.reference(seq, qual, off, bad) is None
    ec.check_refused(run, seq, qual, off, bad, n_bytes, n_out, status=1)
    ec.check_refused(run, seq, qual, off, bad, n_bytes + 100, n_out + 100, status=1)
    bad["code"][i, 1] = 16  # in a fragment that is not put out it is nobody's business
    ec.check(run, seq, qual, off, bad)
    bad = res.copy()
    bad["frag_start"][i, 1], bad["frag_len"][i, 1] = 0xFFFFFFFF, 2
    ec.check_refused(run, seq, qual, off, bad, n_bytes + 2, n_out, status=1)


def test_capacities_one_short_are_refused_and_exact_ones_pass(run):
    seq, qual, off, res = ec.case_random(700, seed=34)
    want = ec.reference(seq, qual, off, res)
    n_bytes, n_out = len(want[0]), len(want[3])
    ec.check_refused(run, seq, qual, off, res, n_bytes - 1, n_out, status=2)
    ec.check_refused(run, seq, qual, off, res, n_bytes, n_out - 1, status=2)
    ec.check(run, seq, qual, off, res)


def test_default_outputs_are_sized_to_suffice(eng):
    """emit_device without output tensors: seq_t.numel() bytes and 2 n reads, which always suffice"""
    import torch

    seq, qual, off, res = ec.case_random(900, seed=35)
    ws, wq, woff, wsrc, wkind = ec.reference(seq, qual, off, res)
    st, qt = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    ot = torch.from_numpy(off.astype(np.int64)).cuda()
    rt = torch.from_numpy(res.view(np.uint8).copy()).cuda()
    so, qo, oo, src, kind, info_t = eng.emit_device(st, qt, ot, rt)
    info = eng.emit_info(info_t)
    assert so.numel() == st.numel() and oo.numel() == 2 * 900 + 1
    assert info == dict(n_bytes=len(ws), n_out=len(wsrc), max_len=int(np.diff(woff).max()), status=0)
    assert np.array_equal(so[:len(ws)].cpu().numpy(), ws) and np.array_equal(qo[:len(ws)].cpu().numpy(), wq)
    assert np.array_equal(oo[:len(wsrc) + 1].cpu().numpy(), woff)
    assert np.array_equal(src[:len(wsrc)].cpu().numpy().view(np.uint32), wsrc) and np.array_equal(kind[:len(wsrc)].cpu().numpy(), wkind)


def test_state_and_argument_errors(engine_mod, eng):
    import torch

    seq, qual, off, res = ec.case_tiny()
    st, qt = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    ot = torch.from_numpy(off.astype(np.int64)).cuda()
    rt = torch.from_numpy(res.view(np.uint8).copy()).cuda()
    masked = engine_mod.Engine(abi.FplOptions.default(mask_enabled=1), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=512)
    with pytest.raises(engine_mod.FplError, match="invalid state.*break_enabled / mask_enabled"):
        masked.emit_device(st, qt, ot, rt)
    masked.close()
    # NULL outputs with reads to put out, a NULL info, a NULL context: FPL_ERR_ARG from the C call itself
    so, qo, oo, src, kind, info_t = eng.emit_device(st, qt, ot, rt)
    L, n, s0 = eng.L, len(off) - 1, C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ctx=eng.h, seq_out=so.data_ptr(), qual_out=qo.data_ptr(), off_out=oo.data_ptr(), info=info_t.data_ptr(), n_reads=n):
        return L.fpl_emit_batch_device(ctx, st.data_ptr(), qt.data_ptr(), ot.data_ptr(), n_reads, rt.data_ptr(), seq_out, qual_out,
                                       so.numel(), off_out, oo.numel() - 1, None, None, info, s0)
    assert call() == abi.FPL_OK
    assert call(seq_out=None) == abi.FPL_ERR_ARG and call(qual_out=None) == abi.FPL_ERR_ARG and call(off_out=None) == abi.FPL_ERR_ARG
    assert call(info=None) == abi.FPL_ERR_ARG and call(ctx=None) == abi.FPL_ERR_ARG
    assert call(seq_out=None, qual_out=None, off_out=None, n_reads=0) == abi.FPL_OK  # nothing to put out: only the info is needed
    assert eng.emit_info(info_t) == dict(n_bytes=0, n_out=0, max_len=0, status=0)


# ---- batches that went through the pipeline ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def piped(orc, engine_mod):
    """3 000 adversarial and 2 000 ONT-like reads as one batch: process_device, then emit_device on the same stream with no
    synchronize between; the oracle's records for the same batch"""
    import torch

    a = synth.adversarial(3000, seed=41)
    b = synth.ont_like(2000, seed=42, median_len=3000, max_len=40000, p_middle=0.1)
    seq, qual = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    off = np.concatenate([a[2], b[2][1:] + a[2][-1]]).astype(np.uint64)
    n = len(off) - 1
    max_len = int(np.diff(off.astype(np.int64)).max())
    opt = abi.FplOptions.default(**C3)
    e = engine_mod.Engine(opt, synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=max_len)
    st, qt = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    ot = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    rt = e.process_device(st, qt, ot, max_len)
    out = e.emit_device(st, qt, ot, rt)
    info = e.emit_info(out[5])
    got_res = e.results_to_numpy(rt, n)
    e.close()
    want_res, _ = orc.process_batch(orc.Config(opt, synth.START_ADAPTER, synth.END_ADAPTER), seq, qual, off, max_cycles=max_len)
    return dict(seq=seq, qual=qual, off=off, got_res=got_res, want_res=want_res, info=info,
                out=[t.cpu().numpy() for t in out[:5]])


def test_emitted_batch_is_the_gather_over_the_oracle_records(piped):
    p = piped
    parity.assert_results_equal(p["got_res"], p["want_res"], p["seq"], p["off"])
    ws, wq, woff, wsrc, wkind = ec.reference(p["seq"], p["qual"], p["off"], p["want_res"])
    so, qo, oo, src, kind = p["out"]
    assert p["info"] == dict(n_bytes=len(ws), n_out=len(wsrc), max_len=int(np.diff(woff).max()), status=0)
    assert set(wkind.tolist()) == {0, 1, 2} and 0 < len(ws) < len(p["seq"])  # splits and trims happened
    assert np.array_equal(so[:len(ws)], ws) and np.array_equal(qo[:len(ws)], wq)
    assert np.array_equal(oo[:len(wsrc) + 1], woff)
    assert np.array_equal(src[:len(wsrc)].view(np.uint32), wsrc) and np.array_equal(kind[:len(wsrc)], wkind)


def test_emitted_reads_are_the_formatter_s_lines(piped, tmp_path):
    """bases and quality lines of fplh_format_batch's --out text for the same batch and records, one for one"""
    p = piped
    text, _, _ = hostio.make_fastq(p["seq"], p["qual"], p["off"], strand_names=True)
    lines = host_format(load_hostlib(), tmp_path, text, p["got_res"]).split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    so, qo, oo, src, kind = p["out"]
    n_out = p["info"]["n_out"]
    assert len(lines) // 4 == n_out
    assert b"".join(lines[1::4]) == so[:p["info"]["n_bytes"]].tobytes() and b"".join(lines[3::4]) == qo[:p["info"]["n_bytes"]].tobytes()
    assert np.array_equal(np.array([len(x) for x in lines[1::4]], np.int64), np.diff(oo[:n_out + 1]))
    assert np.array_equal(np.array([len(x) for x in lines[3::4]], np.int64), np.diff(oo[:n_out + 1]))


def test_statistics_close_over_the_emitted_batch_with_no_host_in_between(engine_mod, monkeypatch):
    """property (2) of tests/test_gpu_parity.py::test_large_batch_properties with the fragment batch made by emit_device: the
    post-filter Stats of a run == the pre-filter Stats of a run over exactly the emitted reads with trimming and filters off.
    Between the two contexts only the 32 bytes of the info come to the host."""
    import torch

    monkeypatch.setenv("FPL_STATS_SORT_MIN", "1")
    opt = abi.FplOptions.default(**C3)
    seq_t, qual_t, off_t, max_len = synth.device_batch(20000, seed=9, median_len=8000)
    eng1 = engine_mod.Engine(opt, synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=max_len)
    monkeypatch.delenv("FPL_STATS_SORT_MIN")  # (the library reads it when a context is created)
    rt = eng1.process_device(seq_t, qual_t, off_t, max_len)
    fseq, fqual, foff, _, _, info_t = eng1.emit_device(seq_t, qual_t, off_t, rt)
    info = eng1.emit_info(info_t)  # the 32 bytes
    assert info["status"] == 0 and 0 < info["n_out"] and info["n_bytes"] < seq_t.numel()
    C_ = eng1.max_cycles
    plain = abi.FplOptions.default(adapter_enabled=0, qual_filter=0, length_filter=0)
    eng2 = engine_mod.Engine(plain, "", "", device=0, max_cycles=C_)
    eng2.process_device(fseq[:info["n_bytes"]], fqual[:info["n_bytes"]], foff[:info["n_out"] + 1], info["max_len"])
    v = abi.CountersView(eng1.counters(), C_, 2)
    v2 = abi.CountersView(eng2.counters(), C_, 2)
    eng1.close()
    eng2.close()
    assert int(v.post.reads) == info["n_out"] and int(v.post.length_sum) == info["n_bytes"]
    for f in ("cyc", "base_qual_hist", "median_hist", "median_bases", "kmer", "reads", "length_sum"):
        assert np.array_equal(np.asarray(getattr(v.post, f)), np.asarray(getattr(v2.pre, f))), f


def test_offsets_beyond_four_gib(eng):
    """four reads of about 1 GiB over an input above 4 GiB, made on the device; the output's last offset exceeds 2^32"""
    import torch

    G = 1 << 30
    lens = [G + 5, G + 100, 3, G - 7, G + 11]
    need = 4 * sum(lens) + (2 << 30)  # bases, qualities, the two outputs, and room to compare
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("%.1f GiB of device memory free, the test needs %.1f" % (free / G, need / G))
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    seq_t = torch.empty(total, dtype=torch.uint8, device="cuda")
    qual_t = torch.empty(total, dtype=torch.uint8, device="cuda")
    for a in range(0, total, 1 << 28):
        b = min(total, a + (1 << 28))
        seq_t[a:b] = torch.randint(0, 256, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
        qual_t[a:b] = torch.randint(0, 256, (b - a,), generator=g, device="cuda", dtype=torch.uint8)
    res = ec.one_fragment(lens, [3, 0, 1, 2, 4], [lens[0] - 3, lens[1] - 50, 2, lens[3] - 2, lens[4] - 5])
    res["code"][2, 0] = abi.FPL_FAIL_LENGTH
    flens = [lens[0] - 3, lens[1] - 50, lens[3] - 2, lens[4] - 5]
    starts = [int(off[0]) + 3, int(off[1]), int(off[3]) + 2, int(off[4]) + 4]
    so, qo, oo, src, kind, info_t = eng.emit_device(seq_t, qual_t, torch.from_numpy(off).cuda(), torch.from_numpy(res.view(np.uint8).copy()).cuda())
    info = eng.emit_info(info_t)
    woff = np.concatenate([[0], np.cumsum(flens)])
    assert info == dict(n_bytes=int(woff[-1]), n_out=4, max_len=max(flens), status=0) and info["n_bytes"] > 2 ** 32
    assert oo[:5].cpu().tolist() == woff.tolist() and src[:4].cpu().tolist() == [0, 1, 3, 4]
    for j in range(4):
        a, b, s = int(woff[j]), int(woff[j + 1]), starts[j]
        assert torch.equal(so[a:b], seq_t[s:s + b - a]) and torch.equal(qo[a:b], qual_t[s:s + b - a]), j
