"""-m gpu: a BGZF-compressed FASTQ's blocks in, records out, everything between on the device (fpl_process_bgzf_text_async /
fpl_peek_bgzf_text / fpl_start_bgzf_text / fpl_wait_bgzf_text and the tail calls, through Engine.submit_bgzf_text;
csrc/bgzf_inflate.h -> csrc/text_walk.h -> the per-read kernels -> csrc/gz_emit.h).

The yardstick is the path that exists without it: Engine.submit_text of the inflated text, whole, through a fresh context (that
this path equals the oracle is what tests/test_gpu_text.py shows).  Records, names, bases, qualities and the whole counter buffer
must be byte-equal.  Three seeded files of about 300 reads of 0 .. 20 000 bases, one of them with "\\r\\n", each written with zlib
in BGZF blocks of 65280 bytes and of 700 bytes -- block and submission cuts then fall on arbitrary bytes of a record.  A refusal
here is a status the library returns: nothing makes a kernel misbehave."""
import ctypes as Cc
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, synth
from tests import bamio, hostio

pytestmark = pytest.mark.gpu

C = 20480
OPTION_SETS = {
    "default": (dict(), "", ""),
    "trims": (dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1), synth.START_ADAPTER,
              synth.END_ADAPTER),
}
TAIL = 1 << 16  # the tail capacity of the contexts here: holds the longest record (40 KB), and keeps the slots small


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


def make_text(seed, crlf):
    seq, qual, off = synth.ont_like(300, seed=seed, median_len=1200, max_len=20000, p_middle=0.05)
    reads = [(seq[int(off[i]):int(off[i + 1])], qual[int(off[i]):int(off[i + 1])]) for i in range(300)]
    for i, ln in ((3, 0), (4, 1), (77, 17), (150, 16), (299, 15)):
        reads[i] = (reads[i][0][:ln], reads[i][1][:ln])
    s, q, _ = synth.ont_like(1, seed=seed + 100, median_len=20000, min_len=20000, max_len=20000)
    reads[200] = (s, q)
    seq, qual, off = synth.pack(reads)
    return hostio.make_fastq(seq, qual, off, crlf=crlf)[0]


@pytest.fixture(scope="module")
def files():
    out = {}
    for name, seed, crlf in (("a", 71, False), ("b", 72, True), ("c", 73, False)):
        text = make_text(seed, crlf)
        out[name] = dict(text=text, b64k=bamio.bgzf(text, block=65280, level=1), b700=bamio.bgzf(text, block=700, level=6))
    return out


def new_engine(engine_mod, opts="trims", tail=TAIL, **kw):
    o, start, end = OPTION_SETS[opts]
    eng = engine_mod.Engine(abi.FplOptions.default(**dict(o, **kw)), start, end, device=0, max_cycles=C)
    if tail:
        eng.reserve_bam_tail(tail)
    return eng


def pinned(eng, data):
    a = eng.pinned_array(max(len(data), 1))
    a[:len(data)] = np.frombuffer(data, np.uint8)
    return a[:len(data)]


_REF = {}


def reference(engine_mod, text, opts="trims", gzip=False):
    """the text whole through submit_text on a fresh context -> dict(res, cnt, names, seq, qual, member); computed once"""
    key = (hash(text), len(text), opts, gzip)
    if key not in _REF:
        eng = new_engine(engine_mod, opts, tail=0)
        eng.submit_text(pinned(eng, text), gzip=gzip)
        got = eng.wait_text()
        info, res, lines = got[:3]
        assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] > 0, info  # the reference must not be the one refusing
        strip = lambda l: l[:-1] if l.endswith(b"\r") else l
        ends = np.concatenate([lines.reshape(-1)[1:], [len(text)]]).reshape(-1, 4)
        four = [[strip(text[int(a):int(b) - 1]) for a, b in zip(ls, es)] for ls, es in zip(lines, ends)]
        _REF[key] = dict(res=res, cnt=eng.counters(), names=[f[0] for f in four], seq=b"".join(f[1] for f in four),
                         qual=b"".join(f[3] for f in four), member=got[3] if gzip else None, max_len=max(len(f[1]) for f in four))
        eng.close()
    return _REF[key]


def record_start(text, i):
    """where record i of regular text starts"""
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    return int(nl[4 * i - 1]) + 1 if i else 0


def payload(eng, data, begin=0, end=None):
    blk, offs = bgzf.blocks(data, begin, end)
    end = len(data) if end is None else end
    return pinned(eng, data[begin:end]), blk, offs


def run_windows(eng, data, per, gzip=False, want_reads=True):
    """the file in submissions of `per` blocks, three in flight -> (headers, records, names, bases, qualities, members)"""
    _, offs = bgzf.blocks(data)
    cuts = [offs[i] for i in range(0, len(offs), per)] + [len(data)]
    pending, hs, res, names, seqs, quals, members = [], [], [], [], [], [], []

    def collect():
        h, r, nm, s, q, m = pending.pop(0).wait(want_reads=want_reads)
        assert h["status"] == abi.FPL_TXTW_OK, h
        hs.append(h), res.append(r), names.extend(nm), members.append(m)
        if h["n_reads"] and want_reads:
            seqs.append(s.tobytes()), quals.append(q.tobytes())

    for k in range(len(cuts) - 1):
        comp, blk, _ = payload(eng, data, cuts[k], cuts[k + 1])
        pending.append(eng.submit_bgzf_text(comp, blk, gzip=gzip))
        if len(pending) == abi.FPL_MAX_IN_FLIGHT:
            assert eng.in_flight() == 3
            collect()
    while pending:
        collect()
    return hs, np.concatenate(res), names, b"".join(seqs), b"".join(quals), members


def assert_same(got, ref, arrays=True):
    _, res, names, seq, qual = got[:5]
    assert res.tobytes() == ref["res"].tobytes() and names == ref["names"]
    if arrays:
        assert bytes(seq) == ref["seq"] and bytes(qual) == ref["qual"]


@pytest.mark.parametrize("name", ["a", "b", "c"])
@pytest.mark.parametrize("form", ["b64k", "b700"])
def test_whole_file_in_one_submission(engine_mod, files, name, form):
    f = files[name]
    for opts in OPTION_SETS:
        ref = reference(engine_mod, f["text"], opts)
        eng = new_engine(engine_mod, opts)
        comp, blk, _ = payload(eng, f[form])
        assert len(blk) > (500 if form == "b700" else 5)
        batch = eng.submit_bgzf_text(comp, blk)
        h = batch.peek()
        assert h["status"] == abi.FPL_TXTW_OK and h["n_reads"] == 300 == h["records_seen"] and h["tail_bytes"] == 0 and h["n_lines"] == 1200, h
        assert h["n_bases"] == len(ref["seq"]) and h["max_read_len"] == ref["max_len"] > 20000 and h["name_bytes"] == sum(len(x) for x in ref["names"])
        assert not eng.counters().any()  # peeked at, not run
        got = batch.wait()
        assert got[0] == h
        assert_same((got[0], got[1], got[2], got[3].tobytes(), got[4].tobytes()), ref)
        assert np.array_equal(eng.counters(), ref["cnt"])
        assert eng.bam_tail() == b""
        eng.close()


@pytest.mark.parametrize("name,form,per", [("a", "b700", 1), ("b", "b700", 3), ("c", "b700", 17), ("b", "b64k", 1)])
def test_many_submissions_three_in_flight(engine_mod, files, name, form, per):
    f = files[name]
    ref = reference(engine_mod, f["text"])
    eng = new_engine(engine_mod)
    got = run_windows(eng, f[form], per)
    assert_same(got, ref)
    hs = got[0]
    assert hs[-1]["tail_bytes"] == 0 and hs[-1]["records_seen"] == 300 and sum(h["tail_bytes"] > 0 for h in hs) > 2
    if form == "b700" and per == 1:
        assert sum(h["n_reads"] == 0 for h in hs) > 50  # (a record of 40 KB spans many blocks of 700 bytes: zero reads, the tail grows)
    assert np.array_equal(eng.counters(), ref["cnt"])
    assert eng.bam_tail() == b""
    eng.close()


def test_a_file_without_a_final_line_break_leaves_its_last_record(engine_mod, files):
    text = files["a"]["text"]
    ref = reference(engine_mod, text)
    eng = new_engine(engine_mod)
    got = run_windows(eng, bamio.bgzf(text[:-1], block=700), 17)
    last = text[record_start(text, 299):-1]
    assert last.count(b"\n") == 3 and last.startswith(b"@read299 ") and eng.bam_tail() == last
    assert got[1].tobytes() == ref["res"][:299].tobytes() and got[2] == ref["names"][:299] and got[0][-1]["tail_bytes"] == len(last)
    # the caller's own reader takes it: one record through the CSR path
    _, s, _, q = last.split(b"\n")
    r = np.zeros(1, abi.RESULT_DTYPE)
    off = np.array([0, len(s)], np.uint64)
    eng.submit_host(pinned(eng, s), pinned(eng, q), off, r)
    eng.wait()
    assert r.tobytes() == ref["res"][299:].tobytes() and np.array_equal(eng.counters(), ref["cnt"])
    eng.set_bam_tail(b"")  # a new file
    eng.close()


def test_null_arrays_and_gzip(engine_mod, files):
    f = files["b"]
    ref = reference(engine_mod, f["text"], gzip=True)
    assert len(ref["member"]) > 1000
    eng = new_engine(engine_mod)
    hs, res, names, seq, qual, members = run_windows(eng, f["b700"], 17, gzip=True, want_reads=False)
    assert res.tobytes() == ref["res"].tobytes() and names == ref["names"] and seq == b"" and qual == b""
    assert b"".join(zlib.decompress(m, 31) for m in members if m) == zlib.decompress(ref["member"], 31)
    assert eng.gzip_batches() == sum(1 for m in members if m) > 10
    assert np.array_equal(eng.counters(), ref["cnt"])
    eng.close()


def host_parse(stretch):
    """the caller's own reader for a refused stretch of regular text: whole records as CSR arrays, and the rest"""
    lines = stretch.split(b"\n")
    rest = lines.pop()
    n = len(lines) // 4
    rest = b"\n".join(lines[4 * n:] + [rest])
    strip = lambda l: l[:-1] if l.endswith(b"\r") else l
    reads = [(np.frombuffer(strip(lines[4 * i + 1]), np.uint8), np.frombuffer(strip(lines[4 * i + 3]), np.uint8)) for i in range(n)]
    return synth.pack(reads), [strip(lines[4 * i]) for i in range(n)], rest


def test_a_refused_block_and_the_way_back_through_the_host_path(engine_mod, files):
    f = files["c"]
    ref = reference(engine_mod, f["text"])
    data = bytearray(f["b64k"])
    _, offs = bgzf.blocks(bytes(data))
    j = len(offs) // 2
    data[offs[j + 1] - 8] ^= 0x55  # the CRC-32 of block j's trailer
    data = bytes(data)
    eng = new_engine(engine_mod)
    a = eng.submit_bgzf_text(*payload(eng, data, 0, offs[j - 1])[:2])
    b = eng.submit_bgzf_text(*payload(eng, data, offs[j - 1], offs[j + 2])[:2])  # blocks j - 1, j, j + 1
    c = eng.submit_bgzf_text(*payload(eng, data, offs[j + 2], offs[j + 3])[:2])
    with pytest.raises(engine_mod.FplError, match="invalid state"):
        eng.bam_tail()  # batches in flight
    ga = a.wait()
    hb, hc = b.wait()[0], c.wait()[0]
    assert ga[0]["status"] == abi.FPL_TXTW_OK
    assert hb["status"] == abi.FPL_TXTW_BLOCK and hb["bad_index"] == 1 and hb["n_reads"] == 0 and hb["records_seen"] == ga[0]["records_seen"]
    assert hc["status"] == abi.FPL_TXTW_CHAIN and hc["n_reads"] == 0
    # recovery: the tail out, the refused stretch inflated and parsed here, its records through submit_host, the rest in
    tail = eng.bam_tail()
    assert len(tail) == ga[0]["tail_bytes"] > 0
    stretch = tail + b"".join(bgzf.inflate_block(data, offs[k]) for k in (j - 1, j, j + 1))
    (s, q, off), mid_names, rest = host_parse(stretch)
    mid = np.zeros(len(off) - 1, abi.RESULT_DTYPE)
    eng.submit_host(pinned(eng, s.tobytes()), pinned(eng, q.tobytes()), off, mid)
    eng.wait()
    eng.set_bam_tail(rest)
    gr = eng.submit_bgzf_text(*payload(eng, data, offs[j + 2], len(data))[:2]).wait()
    assert gr[0]["status"] == abi.FPL_TXTW_OK and gr[0]["tail_bytes"] == 0
    assert np.concatenate([ga[1], mid, gr[1]]).tobytes() == ref["res"].tobytes() and ga[2] + mid_names + gr[2] == ref["names"]
    assert np.array_equal(eng.counters(), ref["cnt"])
    eng.close()


def test_tail_room_then_the_same_result(engine_mod, files):
    """a tail capacity of 4096 and a submission that ends 10 000 bytes into the record of the 20 000-base read"""
    text = files["a"]["text"]
    ref = reference(engine_mod, text)
    cut1, cut2 = record_start(text, 190) + 5, record_start(text, 200) + 10000
    data = bamio.bgzf(text, cuts=[cut1, cut2], block=65280, level=1)
    blk, offs = bgzf.blocks(data)
    offs = list(offs) + [len(data)]
    ends = [int(x) for x in np.cumsum(blk["isize"].astype(np.int64))]
    i1, i2 = ends.index(cut1) + 1, ends.index(cut2) + 1  # the first block behind either cut
    eng = new_engine(engine_mod, tail=4096)
    a = eng.submit_bgzf_text(*payload(eng, data, 0, offs[i1])[:2]).wait()
    assert a[0]["status"] == abi.FPL_TXTW_OK and a[0]["tail_bytes"] == 5 and a[0]["n_reads"] == 190
    kept = eng.bam_tail()
    assert kept == text[cut1 - 5:cut1]
    mid = payload(eng, data, offs[i1], offs[i2])
    m = eng.submit_bgzf_text(*mid[:2])
    behind = eng.submit_bgzf_text(*payload(eng, data, offs[i2], offs[i2 + 1])[:2])
    h, hb = m.wait()[0], behind.wait()[0]
    assert h["status"] == abi.FPL_TXTW_TAIL_ROOM and h["tail_bytes"] == 10000 and h["n_reads"] == 0 and h["records_seen"] == 190, h
    assert hb["status"] == abi.FPL_TXTW_CHAIN
    assert eng.bam_tail() == kept  # the refusal left the tail exactly as it was
    eng.reserve_bam_tail(TAIL)  # (the old tail moves into the larger buffer)
    eng.resume_bgzf()
    assert eng.bam_tail() == kept
    m = eng.submit_bgzf_text(*mid[:2]).wait()
    assert m[0]["status"] == abi.FPL_TXTW_OK and m[0]["tail_bytes"] == 10000 and m[0]["n_reads"] == 10
    rest = eng.submit_bgzf_text(*payload(eng, data, offs[i2], len(data))[:2]).wait()
    assert rest[0]["status"] == abi.FPL_TXTW_OK and rest[0]["tail_bytes"] == 0 and rest[0]["records_seen"] == 300
    assert np.concatenate([a[1], m[1], rest[1]]).tobytes() == ref["res"].tobytes() and a[2] + m[2] + rest[2] == ref["names"]
    assert b"".join(x[3].tobytes() for x in (a, m, rest)) == ref["seq"] and b"".join(x[4].tobytes() for x in (a, m, rest)) == ref["qual"]
    assert np.array_equal(eng.counters(), ref["cnt"])  # the refused stretches counted nothing
    eng.close()


def test_irregular_and_strand(engine_mod, files):
    text = files["a"]["text"]
    lines = text.split(b"\n")
    blank = b"\n".join(lines[:400] + [b""] + lines[400:])  # in front of record 100
    named = b"\n".join(lines[:202] + [b"+" + lines[200][1:]] + lines[203:])  # record 50
    for bad, status, index in ((blank, abi.FPL_TXTW_IRREGULAR, 100), (named, abi.FPL_TXTW_STRAND, 50)):
        data = bamio.bgzf(bad, block=700)
        _, offs = bgzf.blocks(data)
        cut = offs[40]  # (28 000 bytes: behind record 5 at the least, in front of record 50)
        eng = new_engine(engine_mod)
        a = eng.submit_bgzf_text(*payload(eng, data, 0, cut)[:2])
        b = eng.submit_bgzf_text(*payload(eng, data, cut, len(data))[:2])
        ga, gb = a.wait(), b.wait()
        assert ga[0]["status"] == abi.FPL_TXTW_OK and 0 < ga[0]["n_reads"] < 50
        h = gb[0]
        assert h["status"] == status and h["bad_index"] == index and h["n_reads"] == 0 and len(gb[1]) == 0, h
        start = len(b"\n".join(lines[:4 * index])) + 1 - (28000 - ga[0]["tail_bytes"])
        assert h["bad_pos"] == start, (h, start)
        assert eng.bam_tail() == bad[28000 - ga[0]["tail_bytes"]:28000]  # as the first submission left it
        eng.close()


def test_fifo_interleave_wrong_waits_and_whose_tail_it_is(engine_mod, files):
    f = files["a"]
    ref = reference(engine_mod, f["text"])
    seq, qual, off = synth.ont_like(200, seed=9, median_len=1500, max_len=8000)
    text = hostio.make_fastq(seq, qual, off)[0]
    eng = new_engine(engine_mod)
    L, STATE = eng.L, abi.FPL_ERR_STATE
    r0 = np.zeros(len(off) - 1, abi.RESULT_DTYPE)
    eng.submit_host(seq, qual, off, r0)
    eng.submit_text(pinned(eng, text))
    comp, blk, _ = payload(eng, f["b700"])
    batch = eng.submit_bgzf_text(comp, blk)
    assert eng.in_flight() == 3
    # a BGZF BAM batch on ANOTHER context, while this one is in flight
    rng = np.random.default_rng(3)
    bam = bamio.bam_bytes(bamio.random_records(rng, 50, flags=(0, 0x10), lengths=[1, 17, 500, 2000]), block=300, level=1)[0]
    other = new_engine(engine_mod, tail=0)
    hb = other.submit_bgzf(*payload(other, bam)[:2], skip=bgzf.header_len(bam)).wait()[0]
    assert hb["status"] == abi.FPL_BAMW_OK and hb["n_reads"] == 50
    assert L.fpl_process_bgzf_text_async(other.h, comp.ctypes.data, len(comp), blk.ctypes.data, len(blk)) == STATE  # it holds a BAM's tail state
    other.set_bam_tail(b"")
    assert other.submit_bgzf_text(*payload(other, f["b64k"])[:2]).wait(want_reads=False)[0]["n_reads"] == 300  # fresh again: let in
    other.close()
    win = np.zeros(1, np.dtype(abi.TEXT_WINDOW_DTYPE))
    bwin = np.zeros(1, np.dtype(abi.BAM_WINDOW_DTYPE))
    fr = abi.FplTextResult()
    gp, gl = Cc.c_void_p(), Cc.c_uint64(0)
    assert L.fpl_wait_bgzf_text(eng.h, win.ctypes.data, None, None, None, None, None) == STATE  # a CSR batch is the oldest
    assert L.fpl_wait_text(eng.h, Cc.byref(fr), None, None) == STATE and eng.in_flight() == 3
    eng.wait()
    assert L.fpl_wait_bgzf_text(eng.h, win.ctypes.data, None, None, None, None, None) == STATE  # a text batch
    assert L.fpl_wait(eng.h) == STATE and eng.in_flight() == 2
    info, r1, _ = eng.wait_text()
    assert info["n_reads"] == len(off) - 1 and r1.tobytes() == r0.tobytes()
    # the BGZF text batch is the oldest: every other wait leaves it alone
    assert L.fpl_wait(eng.h) == STATE and L.fpl_wait_text(eng.h, Cc.byref(fr), None, None) == STATE
    assert L.fpl_wait_bam_gz(eng.h, Cc.byref(gp), Cc.byref(gl)) == STATE
    assert L.fpl_wait_bgzf_bam(eng.h, bwin.ctypes.data, None, None, None, None, None) == STATE
    assert L.fpl_peek_bgzf_bam(eng.h, bwin.ctypes.data) == STATE and eng.in_flight() == 1
    eng._bam_gz_flags.clear()
    # a BGZF BAM submission on a context that holds a text tail
    bcomp, bblk, _ = payload(eng, bam)
    assert L.fpl_process_bgzf_bam_async(eng.h, bcomp.ctypes.data, len(bcomp), bblk.ctypes.data, len(bblk), 0) == STATE and eng.in_flight() == 1
    nb = len(ref["seq"])
    so, qo = eng.pinned_array(nb + 5), eng.pinned_array(nb)  # the caller's own arrays: the reads land in them
    with pytest.raises(engine_mod.FplError, match="at least n_bases"):
        batch.wait(seq_out=so, qual_out=qo[:nb - 1])
    got = batch.wait(seq_out=so, qual_out=qo)
    assert got[0]["status"] == abi.FPL_TXTW_OK and got[1].tobytes() == ref["res"].tobytes() and got[2] == ref["names"]
    assert np.shares_memory(got[3], so) and so[:nb].tobytes() == ref["seq"] and qo.tobytes() == ref["qual"]
    assert eng.in_flight() == 0
    assert L.fpl_process_bgzf_bam_async(eng.h, bcomp.ctypes.data, len(bcomp), bblk.ctypes.data, len(bblk), 0) == STATE  # still the text's
    assert L.fpl_peek_bgzf_text(eng.h, win.ctypes.data) == STATE and L.fpl_start_bgzf_text(eng.h, None, None) == STATE  # nothing pending
    eng.close()


def test_argument_and_state_errors(engine_mod, files):
    f = files["a"]
    eng = new_engine(engine_mod)
    comp, blk, _ = payload(eng, f["b700"])
    L, ARG, STATE = eng.L, abi.FPL_ERR_ARG, abi.FPL_ERR_STATE

    def submit(b, n=None):
        return L.fpl_process_bgzf_text_async(eng.h, comp.ctypes.data, len(comp) if n is None else n, b.ctypes.data, len(b))

    for field, bad in (("comp_off", len(comp)), ("comp_len", len(comp)), ("isize", 65537), ("out_off", 7)):
        b = blk.copy()
        b[field][3] = bad
        assert submit(b) == ARG
    assert submit(blk, n=int(blk["comp_off"][-1]) + 1) == ARG  # the last payload ends outside comp
    big = np.zeros(70000, np.dtype(abi.BGZF_BLOCK_DTYPE))  # 70 000 blocks of 65536 bytes: a total beyond 32 bits
    big["isize"] = 65536
    big["out_off"] = np.arange(70000, dtype=np.uint64) * 65536
    assert submit(big) == ARG
    assert L.fpl_process_bgzf_text_async(eng.h, None, 10, blk.ctypes.data, len(blk)) == ARG
    assert eng.in_flight() == 0 and eng.bam_tail() == b""  # nothing was enqueued
    assert submit(blk[:5]) == 0
    assert L.fpl_bam_tail_set(eng.h, None, 0) == STATE and L.fpl_resume_bgzf_bam(eng.h) == STATE and L.fpl_reserve_bam_tail(eng.h, 1 << 24) == STATE
    win = np.zeros(1, np.dtype(abi.TEXT_WINDOW_DTYPE))
    one = eng.pinned_array(16)
    assert L.fpl_start_bgzf_text(eng.h, one.ctypes.data, None) == ARG and L.fpl_start_bgzf_text(eng.h, None, one.ctypes.data) == ARG
    gp = Cc.c_void_p()
    assert L.fpl_wait_bgzf_text(eng.h, win.ctypes.data, None, None, None, Cc.byref(gp), None) == ARG and eng.in_flight() == 1
    assert L.fpl_wait_bgzf_text(eng.h, win.ctypes.data, None, None, None, None, None) == 0 and win[0]["status"] == abi.FPL_TXTW_OK
    assert eng.in_flight() == 0
    eng.close()
    eng = new_engine(engine_mod, tail=0, break_enabled=1)
    comp, blk, _ = payload(eng, f["b700"])
    assert eng.L.fpl_process_bgzf_text_async(eng.h, comp.ctypes.data, len(comp), blk.ctypes.data, len(blk)) == STATE
    assert eng.in_flight() == 0
    eng.close()
