"""-m gpu: a BAM's BGZF blocks in, records out, everything between on the device (fpl_process_bgzf_bam_async / fpl_peek_bgzf_bam /
fpl_start_bgzf_bam / fpl_wait_bgzf_bam and the tail calls, through Engine.submit_bgzf; csrc/bgzf_inflate.h -> csrc/bam_walk.h ->
csrc/bam_decode.h -> the per-read kernels -> csrc/gz_emit.h).

The yardstick is the host path on the same file: fplh_bam_read_all (the host's inflate and walk) + Engine.submit_bam.  Records,
the whole counter buffer, the decoded arrays and the names must be byte-equal; that the host path equals the oracle is what the
existing BAM tests show.  Files are written here with zlib, in BGZF blocks of 300 bytes (records straddle blocks and submissions
all the time) and of 64 KiB; segments are 4 KiB where a test says so (FPL_BAM_SEG_BYTES, read when a context is made) so that a
file of a megabyte is cut into hundreds of them.  A refusal here is a status the library returns: nothing makes a kernel misbehave."""
import os

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, synth
from tests import bamio, hostio
from tests.test_host_bam import load_host, read_all

pytestmark = pytest.mark.gpu

OPTS = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
C = 8192


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


@pytest.fixture(scope="module")
def host():
    return load_host()


def make_records(seed, n=300):
    """reads of 0 .. 5000 bases, both strands, secondary / supplementary records mixed in"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 17, 5000, 333] + [int(x) for x in rng.integers(2, 5000, 40)]
    return bamio.random_records(rng, n, flags=(0, 0x10, 0x4, 0x14, 0, 0x10, 0x100, 0x800, 0x110), lengths=lens)


@pytest.fixture(scope="module")
def files(tmp_path_factory, host, engine_mod):
    """the two files, and for each the host path's outcome, computed once: tables of fplh_bam_read_all, and records, counters and
    decoded arrays of ONE submit_bam of all of them"""
    d = tmp_path_factory.mktemp("bam_resident")
    out = {}
    for name, block in (("b300", 300), ("b64k", 65280)):
        data, _, _ = bamio.bam_bytes(make_records(5), block=block, level=1)
        path = d / (name + ".bam")
        path.write_bytes(data)
        t = read_all(host, path)
        assert t["err"] == "" and t["n"] > 200
        out[name] = dict(data=data, t=t, ref=host_path(engine_mod, t))
    return out


def new_engine(engine_mod, seg=None, **opts):
    old = os.environ.get("FPL_BAM_SEG_BYTES")
    if seg:
        os.environ["FPL_BAM_SEG_BYTES"] = str(seg)
    try:
        return engine_mod.Engine(abi.FplOptions.default(**dict(OPTS, **opts)), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=C)
    finally:
        if seg:
            if old is None:
                del os.environ["FPL_BAM_SEG_BYTES"]
            else:
                os.environ["FPL_BAM_SEG_BYTES"] = old


def host_path(engine_mod, t, gzip=False, lo=0, hi=None, eng=None):
    """records lo .. hi of the host's tables through submit_bam -> dict(res, seq, qual, cnt, member)"""
    hi = t["n"] if hi is None else hi
    own = eng is None
    eng = new_engine(engine_mod) if own else eng
    n = hi - lo
    res = np.zeros(n, abi.RESULT_DTYPE)
    off = (t["off"][lo:hi + 1] - t["off"][lo]).astype(np.uint64)
    raw = eng.pinned_array(len(t["raw"]))
    raw[:] = np.frombuffer(t["raw"], np.uint8)
    so, qo = eng.pinned_array(int(off[-1]) + 1), eng.pinned_array(int(off[-1]) + 1)
    eng.submit_bam(raw, np.ascontiguousarray(t["rec"][lo:hi]), off, so, qo, res, gzip=gzip)
    member = eng.wait()
    r = dict(res=res, seq=so[:int(off[-1])].copy(), qual=qo[:int(off[-1])].copy(), member=member)
    if own:
        r["cnt"] = eng.counters()
        eng.close()
    return r


def payload(eng, data, begin=0, end=None):
    blk, offs = bgzf.blocks(data, begin, end)
    end = len(data) if end is None else end
    comp = eng.pinned_array(max(end - begin, 1))
    comp[:end - begin] = np.frombuffer(data, np.uint8, end - begin, begin)
    return comp[:end - begin], blk, offs


def assert_same(got, t, ref, lo=0, hi=None, arrays=True):
    """got: what BgzfBatch.wait returned (or several of them joined) against records lo .. hi of the host path"""
    h, res, names, seq, qual, _ = got
    hi = t["n"] if hi is None else hi
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == hi - lo
    assert res.tobytes() == ref["res"][lo:hi].tobytes()
    assert names == t["names"][lo:hi]
    a, b = int(t["off"][lo]), int(t["off"][hi])
    assert h["n_bases"] == b - a
    if arrays:
        assert seq.tobytes() == ref["seq"][a:b].tobytes() and qual.tobytes() == ref["qual"][a:b].tobytes()
    else:
        assert seq is None and qual is None


@pytest.mark.parametrize("name", ["b300", "b64k"])
def test_whole_file_in_one_submission(engine_mod, files, name):
    f = files[name]
    eng = new_engine(engine_mod, seg=4096)
    comp, blk, _ = payload(eng, f["data"])
    batch = eng.submit_bgzf(comp, blk, skip=bgzf.header_len(f["data"]))
    h = batch.peek()
    assert h["status"] == abi.FPL_BAMW_OK and h["segments"] > 200 and h["tail_bytes"] == 0
    assert h["records_seen"] > h["n_reads"] == f["t"]["n"]
    print("%s: %d segments, %d walked again" % (name, h["segments"], h["rewalked"]))
    got = batch.wait()
    assert_same(got, f["t"], f["ref"])
    assert np.array_equal(eng.counters(), f["ref"]["cnt"])
    assert eng.bam_tail() == b""
    eng.close()


@pytest.mark.parametrize("name,per", [("b300", 400), ("b64k", 1)])
def test_submissions_of_a_few_blocks_three_in_flight(engine_mod, files, name, per):
    """`per` blocks per submission, three submissions in flight all the time; records straddle the submissions (the tail)"""
    f = files[name]
    eng = new_engine(engine_mod)  # (the default segments of 64 KiB)
    _, offs = bgzf.blocks(f["data"])
    cuts = [offs[i] for i in range(0, len(offs), per)] + [len(f["data"])]
    assert len(cuts) > 4
    pending, res, names, seqs, quals, tails = [], [], [], [], [], 0
    skip = bgzf.header_len(f["data"])
    assert skip < int(bgzf.blocks(f["data"], 0, cuts[1])[0]["isize"].sum())

    def collect():
        h, r, nm, s, q, _ = pending.pop(0).wait()
        assert h["status"] == abi.FPL_BAMW_OK, h
        res.append(r), names.extend(nm)
        if h["n_reads"]:
            seqs.append(s.copy()), quals.append(q.copy())
        return h["tail_bytes"]

    for k in range(len(cuts) - 1):
        comp, blk, _ = payload(eng, f["data"], cuts[k], cuts[k + 1])
        pending.append(eng.submit_bgzf(comp, blk, skip=skip if k == 0 else 0))
        if len(pending) == abi.FPL_MAX_IN_FLIGHT:
            assert eng.in_flight() == 3
            tails += collect() > 0
    while pending:
        last_tail = collect()
    assert last_tail == 0 and tails > 0
    t, ref = f["t"], f["ref"]
    assert np.concatenate(res).tobytes() == ref["res"].tobytes() and names == t["names"]
    assert np.concatenate(seqs).tobytes() == ref["seq"].tobytes() and np.concatenate(quals).tobytes() == ref["qual"].tobytes()
    assert np.array_equal(eng.counters(), ref["cnt"])
    eng.close()


def test_null_arrays_and_gzip(engine_mod, files):
    f = files["b300"]
    eng = new_engine(engine_mod, seg=4096)
    comp, blk, _ = payload(eng, f["data"])
    got = eng.submit_bgzf(comp, blk, skip=bgzf.header_len(f["data"])).wait(want_reads=False)
    assert_same(got, f["t"], f["ref"], arrays=False)
    assert got[5] is None and np.array_equal(eng.counters(), f["ref"]["cnt"])
    eng.close()
    # the member of a gzip batch: what submit_bam(..., gzip=True) gives for the same reads
    want = host_path(engine_mod, f["t"], gzip=True)
    assert isinstance(want["member"], bytes) and len(want["member"]) > 1000
    eng = new_engine(engine_mod, seg=4096)
    comp, blk, _ = payload(eng, f["data"])  # (page-locked memory is its engine's: the first one's went with it)
    got = eng.submit_bgzf(comp, blk, skip=bgzf.header_len(f["data"]), gzip=True).wait(want_reads=False)
    assert_same(got, f["t"], f["ref"], arrays=False)
    import zlib
    assert zlib.decompress(got[5], 31) == zlib.decompress(want["member"], 31)
    assert eng.gzip_batches() == 1
    eng.close()


def test_a_refused_block_and_the_way_back_through_the_host_path(engine_mod, files, host, tmp_path):
    """a block in the middle whose trailer CRC is altered: BLOCK with its index, CHAIN behind it; then the recovery sequence"""
    f = files["b64k"]
    data = bytearray(f["data"])
    _, offs = bgzf.blocks(bytes(data))
    j = len(offs) // 2
    end_j = offs[j + 1]
    data[end_j - 8] ^= 0x55  # the CRC-32 of block j's trailer
    data = bytes(data)
    (tmp_path / "bad.bam").write_bytes(data)
    verdict = read_all(host, tmp_path / "bad.bam")["err"]
    assert "BGZF block at file offset %d has a bad CRC" % offs[j] in verdict  # the host's verdict is the one reported
    t, ref = f["t"], f["ref"]
    eng = new_engine(engine_mod)
    a = eng.submit_bgzf(*payload(eng, data, 0, offs[j - 1])[:2], skip=bgzf.header_len(data))
    b = eng.submit_bgzf(*payload(eng, data, offs[j - 1], offs[j + 2])[:2])  # blocks j - 1, j, j + 1
    c = eng.submit_bgzf(*payload(eng, data, offs[j + 2], offs[j + 3])[:2])
    with pytest.raises(engine_mod.FplError, match="invalid state"):
        eng.bam_tail()  # batches in flight
    ha = a.wait()
    hb, hc = b.wait()[0], c.wait()[0]
    assert ha[0]["status"] == abi.FPL_BAMW_OK
    assert hb["status"] == abi.FPL_BAMW_BLOCK and hb["bad_index"] == 1 and hb["n_reads"] == 0
    assert hc["status"] == abi.FPL_BAMW_CHAIN
    n0 = ha[0]["n_reads"]
    # recovery: the tail out, the refused stretch inflated and walked here, its whole records through submit_bam, the rest in
    tail = eng.bam_tail()
    assert len(tail) == ha[0]["tail_bytes"]
    stretch = tail + b"".join(bgzf.inflate_block(data, offs[k]) for k in (j - 1, j, j + 1))
    raw_pos = int(bgzf.blocks(data, 0, offs[j - 1])[0]["isize"].sum()) - len(tail)  # where the tail starts in the inflated stream
    assert n0 == int(np.searchsorted(t["rec"], raw_pos, side="left"))
    assert t["raw"][raw_pos:raw_pos + len(stretch)] == stretch  # (the block's bytes are intact: only its trailer was altered)
    n1 = int(np.searchsorted(t["rec"], raw_pos + len(stretch), side="left"))
    while n1 > n0 and (int(t["rec"][n1 - 1]) + 4 + int.from_bytes(t["raw"][int(t["rec"][n1 - 1]):int(t["rec"][n1 - 1]) + 4], "little") > raw_pos + len(stretch)):
        n1 -= 1
    assert n1 > n0
    mid = host_path(engine_mod, t, lo=n0, hi=n1, eng=eng)
    # the rest of the stretch: behind the last whole record, skipped ones included (the walk below is bamio's)
    p = int(t["rec"][n1 - 1])
    p += 4 + int.from_bytes(t["raw"][p:p + 4], "little")
    while p + 4 <= raw_pos + len(stretch) and p + 4 + int.from_bytes(t["raw"][p:p + 4], "little") <= raw_pos + len(stretch):
        p += 4 + int.from_bytes(t["raw"][p:p + 4], "little")  # (only skipped records can stand here)
    eng.set_bam_tail(t["raw"][p:raw_pos + len(stretch)])
    rest = eng.submit_bgzf(*payload(eng, data, offs[j + 2], len(data))[:2]).wait()
    assert rest[0]["status"] == abi.FPL_BAMW_OK and rest[0]["tail_bytes"] == 0
    res = np.concatenate([ha[1], mid["res"], rest[1]])
    assert res.tobytes() == ref["res"].tobytes() and ha[2] + t["names"][n0:n1] + rest[2] == t["names"]
    assert np.array_equal(eng.counters(), ref["cnt"])
    eng.close()


def tails_behind_blocks(data, raw):
    """for every block of the file: how many inflated bytes lie behind the last whole record once that block is in (the walk is
    bamio's: block_size after block_size from the end of the header)"""
    blk, _ = bgzf.blocks(data)
    p, ends, tails = bgzf.header_len(data), np.cumsum(blk["isize"].astype(np.int64)), []
    for e in (int(x) for x in ends):
        while p + 4 <= e and p + 4 + int.from_bytes(raw[p:p + 4], "little") <= e:
            p += 4 + int.from_bytes(raw[p:p + 4], "little")
        tails.append(e - p)
    return tails, [int(x) for x in ends]


def test_tail_room_then_the_same_result(engine_mod, files):
    f = files["b64k"]
    t, ref = f["t"], f["ref"]
    skip = bgzf.header_len(f["data"])
    _, offs = bgzf.blocks(f["data"])
    offs = list(offs) + [len(f["data"])]
    tails, ends = tails_behind_blocks(f["data"], t["raw"])
    # the file's first stretch with a tiny capacity: refused, the tail stays empty, and resume lets it in again WITH its skip
    eng = new_engine(engine_mod)
    eng.reserve_bam_tail(16)  # no record's cut-off part fits
    assert tails[1] > 16
    first = payload(eng, f["data"], 0, offs[2])
    h = eng.submit_bgzf(*first[:2], skip=skip).wait()[0]
    assert h["status"] == abi.FPL_BAMW_TAIL_ROOM and h["tail_bytes"] == tails[1] and h["n_reads"] == 0 and eng.bam_tail() == b""
    eng.reserve_bam_tail(1 << 20)
    eng.resume_bgzf()
    a = eng.submit_bgzf(*first[:2], skip=skip).wait()
    assert a[0]["status"] == abi.FPL_BAMW_OK and a[0]["tail_bytes"] == tails[1]
    b = eng.submit_bgzf(*payload(eng, f["data"], offs[2], len(f["data"]))[:2]).wait()
    assert np.concatenate([a[1], b[1]]).tobytes() == ref["res"].tobytes() and a[2] + b[2] == t["names"]
    assert np.array_equal(eng.counters(), ref["cnt"])
    eng.close()
    # a refusal in the middle of the file, a tail present: block i leaves a tail that fits exactly, block i + 1 a longer one
    i = next(k for k in range(len(tails) - 1) if tails[k + 1] > tails[k] > 0)
    eng = new_engine(engine_mod)
    eng.reserve_bam_tail(tails[i])
    a = eng.submit_bgzf(*payload(eng, f["data"], 0, offs[i + 1])[:2], skip=skip).wait()
    assert a[0]["status"] == abi.FPL_BAMW_OK and a[0]["tail_bytes"] == tails[i]
    kept = t["raw"][ends[i] - tails[i]:ends[i]]
    assert eng.bam_tail() == kept
    mid = payload(eng, f["data"], offs[i + 1], offs[i + 2])
    m = eng.submit_bgzf(*mid[:2])
    behind = eng.submit_bgzf(*payload(eng, f["data"], offs[i + 2], offs[i + 3])[:2])
    h, hb = m.wait()[0], behind.wait()[0]
    assert h["status"] == abi.FPL_BAMW_TAIL_ROOM and h["tail_bytes"] == tails[i + 1] and h["n_reads"] == 0
    assert hb["status"] == abi.FPL_BAMW_CHAIN
    assert eng.bam_tail() == kept  # the refusal left the tail exactly as it was
    n_a = a[0]["n_reads"]
    assert a[1].tobytes() == ref["res"][:n_a].tobytes()
    eng.reserve_bam_tail(tails[i + 1])  # (the old tail moves into the larger buffer)
    eng.resume_bgzf()
    assert eng.bam_tail() == kept
    assert eng.L.fpl_process_bgzf_bam_async(eng.h, mid[0].ctypes.data, len(mid[0]), mid[1].ctypes.data, len(mid[1]), 1) == abi.FPL_ERR_ARG  # skip, a tail present
    m = eng.submit_bgzf(*mid[:2]).wait()
    assert m[0]["status"] == abi.FPL_BAMW_OK and m[0]["tail_bytes"] == tails[i + 1]
    eng.reserve_bam_tail(1 << 20)
    rest = eng.submit_bgzf(*payload(eng, f["data"], offs[i + 2], len(f["data"]))[:2]).wait()
    assert rest[0]["status"] == abi.FPL_BAMW_OK and rest[0]["tail_bytes"] == 0
    assert np.concatenate([a[1], m[1], rest[1]]).tobytes() == ref["res"].tobytes() and a[2] + m[2] + rest[2] == t["names"]
    assert np.array_equal(eng.counters(), ref["cnt"])  # the refused stretches counted nothing
    eng.close()


def test_fifo_interleave_and_the_wrong_waits(engine_mod, files):
    f = files["b300"]
    seq, qual, off = synth.ont_like(200, seed=9, median_len=1500, max_len=8000)
    text = hostio.make_fastq(seq, qual, off)[0]
    eng = new_engine(engine_mod)
    r0 = np.zeros(len(off) - 1, abi.RESULT_DTYPE)
    eng.submit_host(seq, qual, off, r0)
    tbuf = eng.pinned_array(len(text))
    tbuf[:] = np.frombuffer(text, np.uint8)
    eng.submit_text(tbuf)
    comp, blk, _ = payload(eng, f["data"])
    batch = eng.submit_bgzf(comp, blk, skip=bgzf.header_len(f["data"]))
    assert eng.in_flight() == 3
    import ctypes as Cc
    win = np.zeros(1, np.dtype(abi.BAM_WINDOW_DTYPE))
    fr = abi.FplTextResult()
    assert eng.L.fpl_wait_bgzf_bam(eng.h, win.ctypes.data, None, None, None, None, None) == abi.FPL_ERR_STATE  # a CSR batch is the oldest
    eng.wait()
    assert eng.L.fpl_wait(eng.h) == abi.FPL_ERR_STATE  # a text batch
    info, r1, _ = eng.wait_text()
    assert info["n_reads"] == len(off) - 1 and r1.tobytes() == r0.tobytes()
    assert eng.L.fpl_wait(eng.h) == abi.FPL_ERR_STATE and eng.L.fpl_wait_text(eng.h, Cc.byref(fr), None, None) == abi.FPL_ERR_STATE
    gp, gl = Cc.c_void_p(), Cc.c_uint64(0)
    assert eng.L.fpl_wait_bam_gz(eng.h, Cc.byref(gp), Cc.byref(gl)) == abi.FPL_ERR_STATE and eng.in_flight() == 1
    eng._bam_gz_flags.clear()
    nb = int(f["t"]["off"][-1])
    so, qo = eng.pinned_array(nb + 5), eng.pinned_array(nb)  # the caller's own arrays: the reads land in them
    with pytest.raises(engine_mod.FplError, match="at least n_bases"):
        batch.wait(seq_out=so, qual_out=qo[:nb - 1])
    got = batch.wait(seq_out=so, qual_out=qo)
    assert_same(got, f["t"], f["ref"])
    assert np.shares_memory(got[3], so) and qo.tobytes() == f["ref"]["qual"].tobytes()
    assert eng.in_flight() == 0
    eng.close()


def test_argument_and_state_errors(engine_mod, files):
    f = files["b300"]
    eng = new_engine(engine_mod)
    comp, blk, _ = payload(eng, f["data"])
    L, ARG, STATE = eng.L, abi.FPL_ERR_ARG, abi.FPL_ERR_STATE

    def submit(b, skip=0, n=None):
        return L.fpl_process_bgzf_bam_async(eng.h, comp.ctypes.data, len(comp) if n is None else n, b.ctypes.data, len(b), skip)

    for field, bad in (("comp_off", len(comp)), ("comp_len", len(comp)), ("isize", 65537), ("out_off", 7)):
        b = blk.copy()
        b[field][3] = bad
        assert submit(b) == ARG
    assert submit(blk, n=int(blk["comp_off"][-1]) + 1) == ARG  # the last payload ends outside comp
    assert submit(blk, skip=int(blk["isize"].sum()) + 1) == ARG
    assert eng.in_flight() == 0
    assert submit(blk[:5], skip=bgzf.header_len(f["data"])) == 0
    assert L.fpl_bam_tail_set(eng.h, None, 0) == STATE and L.fpl_resume_bgzf_bam(eng.h) == STATE and L.fpl_reserve_bam_tail(eng.h, 1 << 24) == STATE
    win = np.zeros(1, np.dtype(abi.BAM_WINDOW_DTYPE))
    one = eng.pinned_array(16)
    assert L.fpl_start_bgzf_bam(eng.h, one.ctypes.data, None) == ARG
    assert L.fpl_wait_bgzf_bam(eng.h, win.ctypes.data, None, None, None, None, None) == 0 and win[0]["status"] == abi.FPL_BAMW_OK
    nxt = blk[5:9].copy()
    nxt["out_off"] -= nxt["out_off"][0]
    assert submit(nxt, skip=3) == ARG  # skip with a file under way
    assert L.fpl_peek_bgzf_bam(eng.h, win.ctypes.data) == STATE and L.fpl_start_bgzf_bam(eng.h, None, None) == STATE  # nothing pending
    eng.close()
    eng = new_engine(engine_mod, break_enabled=1)
    comp, blk, _ = payload(eng, f["data"])
    assert eng.L.fpl_process_bgzf_bam_async(eng.h, comp.ctypes.data, len(comp), blk.ctypes.data, len(blk), 0) == STATE
    eng.close()


def text_batch(eng, seed):
    """200 reads as CSR arrays and as FASTQ text in the engine's page-locked memory"""
    seq, qual, off = synth.ont_like(200, seed=seed, median_len=1500, max_len=8000)
    text = hostio.make_fastq(seq, qual, off)[0]
    buf = eng.pinned_array(len(text))
    buf[:] = np.frombuffer(text, np.uint8)
    return seq, qual, off, buf


def test_staged_kinds_interleaved(engine_mod, files):
    """text T1, a BGZF batch B, text T2 in flight together: each kind's peek / start / cancel finds the oldest pending slot of ITS
    kind, whatever stands in front of it, and the waits collect in the order of submission"""
    import ctypes as Cc
    f = files["b300"]
    t, L, STATE = f["t"], None, abi.FPL_ERR_STATE
    # what B and T2 alone give: the host path for B, the same reads as a CSR batch for T2, one context
    ref = new_engine(engine_mod)
    s2, q2, o2, _ = text_batch(ref, 22)
    host_path(engine_mod, t, eng=ref)
    want2 = np.zeros(len(o2) - 1, abi.RESULT_DTYPE)
    ref.submit_host(s2, q2, o2, want2)
    ref.wait()
    want_cnt = ref.counters()
    ref.close()

    eng = new_engine(engine_mod)
    L = eng.L
    _, _, o1, t1 = text_batch(eng, 21)
    _, _, _, t2 = text_batch(eng, 22)
    assert int(o1[-1]) != int(o2[-1])
    comp, blk, _ = payload(eng, f["data"])
    eng.submit_text(t1)
    batch = eng.submit_bgzf(comp, blk, skip=bgzf.header_len(f["data"]))
    eng.submit_text(t2)
    assert eng.in_flight() == abi.FPL_MAX_IN_FLIGHT == 3
    info = eng.peek_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] == 200 and info["n_bases"] == int(o1[-1])  # T1
    h = batch.peek()  # B, although T1 is older
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == t["n"] and not eng.counters().any()
    nb = int(t["off"][-1])
    so, qo = eng.pinned_array(nb + 1), eng.pinned_array(nb + 1)
    assert L.fpl_start_bgzf_bam(eng.h, so.ctypes.data, qo.ctypes.data) == 0  # B's kernels ahead of T1's wait
    eng.cancel_text()  # T1
    info = eng.peek_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] == 200 and info["n_bases"] == int(o2[-1])  # T2
    # a fourth submission, of any kind
    r4 = np.zeros(len(o2) - 1, abi.RESULT_DTYPE)
    raw = np.frombuffer(t["raw"], np.uint8)
    assert L.fpl_process_text_async(eng.h, t2.ctypes.data, len(t2)) == STATE
    assert L.fpl_process_bgzf_bam_async(eng.h, comp.ctypes.data, len(comp), blk.ctypes.data, len(blk), 0) == STATE
    assert L.fpl_process_batch_async(eng.h, s2.ctypes.data, q2.ctypes.data, o2.ctypes.data, len(o2) - 1, r4.ctypes.data) == STATE
    assert L.fpl_process_bam_async(eng.h, raw.ctypes.data, len(raw), t["rec"].ctypes.data, t["off"].ctypes.data, 0, None, None, None) == STATE
    assert eng.in_flight() == 3
    # the waits, in the order of submission
    info, res, _ = eng.wait_text()
    assert info["status"] == abi.FPL_TEXT_CANCELLED and len(res) == 0
    got = batch.wait(want_reads=False)  # (started above, into so / qo)
    assert_same(got, t, f["ref"], arrays=False)
    assert so[:nb].tobytes() == f["ref"]["seq"].tobytes() and qo[:nb].tobytes() == f["ref"]["qual"].tobytes()
    info, res, _ = eng.wait_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] == 200 and res.tobytes() == want2.tobytes()
    assert np.array_equal(eng.counters(), want_cnt)  # B and T2, nothing of T1
    # nothing in flight: nothing pending for either kind
    assert eng.in_flight() == 0
    fr = abi.FplTextResult()
    win = np.zeros(1, np.dtype(abi.BAM_WINDOW_DTYPE))
    assert L.fpl_peek_text(eng.h, Cc.byref(fr)) == STATE and L.fpl_start_text(eng.h) == STATE and L.fpl_cancel_text(eng.h) == STATE
    assert L.fpl_peek_bgzf_bam(eng.h, win.ctypes.data) == STATE and L.fpl_start_bgzf_bam(eng.h, None, None) == STATE
    eng.close()


def test_check_order_of_the_submit_calls_with_break(engine_mod, files):
    """break_enabled: the staged kinds are refused outright, the CSR and BAM calls only while a batch is in flight; an argument
    error comes before either"""
    f = files["b300"]
    t = f["t"]
    eng = new_engine(engine_mod, break_enabled=1)
    L, ARG, STATE = eng.L, abi.FPL_ERR_ARG, abi.FPL_ERR_STATE
    seq, qual, off, tbuf = text_batch(eng, 23)
    n = len(off) - 1
    comp, blk, _ = payload(eng, f["data"])
    raw = np.frombuffer(t["raw"], np.uint8)
    nb = int(t["off"][-1])
    so, qo = eng.pinned_array(nb + 1), eng.pinned_array(nb + 1)
    rb = np.zeros(t["n"], abi.RESULT_DTYPE)
    r0, r1 = np.zeros(n, abi.RESULT_DTYPE), np.zeros(n, abi.RESULT_DTYPE)

    def csr(res):
        return L.fpl_process_batch_async(eng.h, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, n, res.ctypes.data if res is not None else None)

    def bam(res):
        return L.fpl_process_bam_async(eng.h, raw.ctypes.data, len(raw), t["rec"].ctypes.data, t["off"].ctypes.data, t["n"], so.ctypes.data,
                                       qo.ctypes.data, res.ctypes.data if res is not None else None)

    assert L.fpl_process_text_async(eng.h, tbuf.ctypes.data, len(tbuf)) == STATE
    assert L.fpl_process_bgzf_bam_async(eng.h, comp.ctypes.data, len(comp), blk.ctypes.data, len(blk), bgzf.header_len(f["data"])) == STATE
    assert csr(None) == ARG and bam(None) == ARG and eng.in_flight() == 0
    assert csr(r0) == 0 and eng.in_flight() == 1
    eng._bam_gz_flags.append(False)  # (what submit_host notes for wait())
    assert csr(r1) == STATE and bam(rb) == STATE  # one in flight: the fragment lists are its
    assert csr(None) == ARG and bam(None) == ARG and eng.in_flight() == 1
    assert L.fpl_set_bam_gzip(eng.h, 1) == STATE
    eng.wait()
    assert eng.in_flight() == 0 and csr(r1) == 0  # collected: the next one is let in
    eng._bam_gz_flags.append(False)
    eng.wait()
    assert r1.tobytes() == r0.tobytes()
    eng.close()
