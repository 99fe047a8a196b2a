"""The device's BAM record walk (fastplong_amd/csrc/bam_walk.h: k_bam_place_tail, k_bam_find, k_bam_walk_seg, k_bam_chain,
k_bam_compact) on the emulator, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/emu_bamwalk): every buffer has exactly its promised size, so a run that ends clean also never left one.

What is expected never comes from the kernels: record starts, offsets, names and the index of a failing record are the host's own
walk (fplh_bam_read_all over a BAM file made of the same records), the tail and records_seen follow from where the generator put
the records, and `rewalked` is predicted EXACTLY by a pure-Python model of find + chain (tests/bam_walk_cases.py) -- 0 on the
plain streams, so the guessed path is what ran, at least 1 where a false candidate was planted.

Segments are 256 bytes, the tail capacity 1024: a position p of the stream [tail | data] is byte 1024 - len(tail) + p of the buffer."""
import re

import numpy as np
import pytest

from tests import bam_walk_cases as wc
from tests import bamio
from tests.emu_bamwalk import build as emu
from tests.test_host_bam import load_host, read_all

SEG, CAP = 256, 1024
OK, BLOCK, RECORD, TAIL_ROOM, TOO_MANY, CHAIN = range(6)


@pytest.fixture(scope="module")
def host():
    return load_host()


def host_tables(host, tmp_path, recs, name="x.bam"):
    """the host's walk over a file of these records -> (starts in the record stream, offsets, names, error text)"""
    hdr = bamio.header()
    path = tmp_path / name
    path.write_bytes(bamio.bgzf(hdr + b"".join(recs), block=300))
    t = read_all(host, path)
    return [int(r) - len(hdr) for r in t["rec"]], [int(o) for o in t["off"]], t["names"], t["err"]


def run_stream(host, tmp_path, recs, cuts, lead=b"", seg=SEG, cap=CAP, planted=False):
    """the records' stream (behind `lead`, bytes the first submission skips) cut at `cuts` into submissions, one context.  Every
    submission is checked against the generator's boundaries and the model; the accepted ones together against the host's walk.
    -> the submissions' results"""
    stream = b"".join(recs)
    bounds = np.cumsum([0] + [len(r) for r in recs])  # record boundaries in the stream
    h_rec, h_off, h_names, err = host_tables(host, tmp_path, recs)
    assert err == ""
    cuts = sorted(set(list(cuts) + [len(stream)]))
    ops, at = [emu.new(cap)], 0
    for k, c in enumerate(cuts):
        data = stream[at:c]
        ops.append(emu.submit(lead + data if k == 0 else data, skip=len(lead) if k == 0 else 0, seg_bytes=seg))
        ops.append(("tail_get",))
        at = c
    res = emu.run(ops)
    got_rec, got_names, got_off, seen, at, tail_start, rew_total = [], [], [0], 0, 0, 0, 0
    for k, c in enumerate(cuts):
        r, tail = res[2 * k], res[2 * k + 1]
        assert r["rc"] == 0 and r["status"] == OK, (k, r)
        data = stream[at:c]
        old_tail = stream[tail_start:at]
        rew, cand = wc.model(old_tail, lead + data if k == 0 else data, cap, seg, len(lead) if k == 0 else 0)
        assert r["rewalked"] == rew, (k, r["rewalked"], rew)
        assert list(r["cand"]) == cand
        assert r["segments"] == len(cand)
        rew_total += rew
        n_whole = int(np.searchsorted(bounds, c, side="right")) - 1  # records that end at or before c
        new_tail_start = int(bounds[n_whole])
        assert r["records_seen"] == n_whole - seen and r["tail_bytes"] == c - new_tail_start and tail == stream[new_tail_start:c]
        lo = cap - len(old_tail) + (len(lead) if k == 0 else 0)  # buffer position of stream byte tail_start
        got_rec += [int(x) - lo + tail_start for x in r["rec"]]
        got_off += [got_off[-1] + int(o) for o in r["off"][1:]]
        assert int(r["off"][0]) == 0 and int(r["off"][-1]) == r["n_bases"] and int(r["name_off"][-1]) == r["name_bytes"] == len(r["names"])
        got_names += [r["names"][int(r["name_off"][i]):int(r["name_off"][i + 1])] for i in range(r["n_reads"])]
        lens = np.diff(r["off"].astype(np.int64))
        assert r["max_read_len"] == (int(lens.max()) if len(lens) else 0)
        seen, at, tail_start = n_whole, c, new_tail_start
    assert got_rec == h_rec and got_off == h_off and got_names == h_names
    assert (rew_total >= 1) if planted else (rew_total == 0), rew_total
    return res[0::2]


def test_plain_streams_and_every_cut(host, tmp_path):
    rng = np.random.default_rng(1)
    recs = wc.records(rng, 30)
    n = len(b"".join(recs))
    run_stream(host, tmp_path, recs, [])
    run_stream(host, tmp_path, recs, [n // 3, 2 * n // 3])
    run_stream(host, tmp_path, recs, range(197, n, 397))  # records straddle the submissions
    run_stream(host, tmp_path, recs, [], lead=bamio.header())  # skip points at the first record
    run_stream(host, tmp_path, recs, [500], lead=bamio.header())


@pytest.mark.parametrize("d", [-3, -2, -1, 0, 1, 2, 3])
def test_a_record_start_at_and_around_a_segment_boundary(host, tmp_path, d):
    """record 3 starts d bytes from buffer position 1024 + 512 (the block_size field straddles the boundary for d = -3 .. -1)"""
    rng = np.random.default_rng(2)
    recs = [wc.pad_record(rng, 0, 200), wc.pad_record(rng, 1, 180), wc.pad_record(rng, 2, 132 + d)] + wc.records(rng, 8)
    assert sum(len(r) for r in recs[:3]) == 512 + d
    run_stream(host, tmp_path, recs, [])


def test_a_record_over_four_segments_and_skipped_records(host, tmp_path):
    rng = np.random.default_rng(3)
    sk = [wc.record(rng, 100 + i, 30, f) for i, f in enumerate((0x100, 0x800, 0x110, 0x900))]
    recs = [sk[0]] + wc.records(rng, 5) + [wc.record(rng, 50, 700), sk[1], sk[2]] + wc.records(rng, 5) + [wc.record(rng, 51, 0, name=b""), sk[3]]
    res = run_stream(host, tmp_path, recs, [])
    assert (res[0]["cand"] == wc.NO_CAND).sum() >= 4 + 2  # the tail room's empty segments, and the long record's middle ones
    assert res[0]["records_seen"] == res[0]["n_reads"] + 4
    run_stream(host, tmp_path, recs, [len(recs[0]) + 10, 900])


def test_a_planted_false_candidate_is_not_believed(host, tmp_path):
    """bytes inside a record's tags that pass k_bam_find's filter, 5 bytes into a segment; the record ends 20 bytes behind them, so
    the true start of the next record lies later in the same segment: that segment's guess is wrong and the chain walks it again"""
    rng = np.random.default_rng(4)
    head = wc.records(rng, 4)
    tags_at = CAP + sum(len(r) for r in head) + len(wc.record(rng, 60, 20))
    recs = head + [wc.record(rng, 60, 20, tags=wc.planted_tags(SEG + 5 + (-tags_at) % SEG, 20))] + wc.records(rng, 6)
    run_stream(host, tmp_path, recs, [], planted=True)
    run_stream(host, tmp_path, recs, [2 * SEG], planted=True)  # (a cut at a multiple of the segment size keeps the positions' phase)


def test_where_the_buffer_ends(host, tmp_path):
    rng = np.random.default_rng(5)
    recs = wc.records(rng, 12)
    s = int(np.cumsum([len(r) for r in recs])[5])  # start of record 6 (l_seq 500)
    assert len(recs[6]) > 500
    for cut in (s + 2, s + 20, s + 38, s + 70, s):  # inside block_size, the fixed fields, the name, the bases; at a record's end
        res = run_stream(host, tmp_path, recs, [cut])
        assert res[0]["tail_bytes"] == cut - s


def test_one_record_as_the_tail_across_three_submissions(host, tmp_path):
    rng = np.random.default_rng(6)
    recs = wc.records(rng, 3) + [wc.record(rng, 70, 400)] + wc.records(rng, 3)
    s = sum(len(r) for r in recs[:3])
    res = run_stream(host, tmp_path, recs, [s + 100, s + 250, s + 400])
    assert [r["n_reads"] for r in res[1:3]] == [0, 0] and res[1]["tail_bytes"] == 250 and res[2]["tail_bytes"] == 400


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", wc.DAMAGE)
def test_every_rule_refuses_with_the_hosts_index(host, tmp_path, kind, where):
    rng = np.random.default_rng(7)
    recs = wc.records(rng, 9)
    k = {"first": 0, "middle": 4, "last": 8}[where]
    recs[k] = wc.damaged(rng, k, kind)
    *_, err = host_tables(host, tmp_path, recs)
    m = re.match(r"BAM record (\d+)", err)
    assert m and int(m.group(1)) == k, err
    stream = b"".join(recs)
    bounds = np.cumsum([0] + [len(r) for r in recs])
    cut = 2 if k == 0 else int(bounds[k - 1]) + 10  # the first submission ends inside the record in front (or inside block_size)
    res = emu.run([emu.new(CAP), emu.submit(stream[:cut]), ("tail_get",), emu.submit(stream[cut:]), ("tail_get",), emu.submit(b""),
                   ("resume",), emu.submit(b"")])
    first, tail0, bad, tail1, behind, again = res
    assert first["status"] == OK and len(tail0) == cut - (0 if k == 0 else int(bounds[k - 1]))
    assert bad["status"] == RECORD and bad["bad_index"] == k and bad["bad_pos"] == int(bounds[k]) - (cut - len(tail0))
    assert bad["n_reads"] == 0 and bad["records_seen"] == 0 and tail1 == tail0  # nothing counted, the tail as it was
    assert behind["status"] == CHAIN
    assert again["status"] == OK and again["n_reads"] == 0  # resumed: the tail alone holds no whole record


def test_tail_room_and_the_way_on(host, tmp_path):
    rng = np.random.default_rng(8)
    recs = wc.records(rng, 7)
    stream = b"".join(recs)
    s = sum(len(r) for r in recs[:6])
    cut = s + 100  # 100 bytes of the last record: more than a tail capacity of 64
    res = emu.run([emu.new(64), emu.submit(stream[:cut], seg_bytes=64), ("tail_get",), emu.submit(b"", seg_bytes=64), ("reserve", 256),
                   ("resume",), emu.submit(stream[:cut], seg_bytes=64), ("tail_get",), emu.submit(stream[cut:], seg_bytes=64)])
    full, tail, behind, again, tail2, rest = res
    assert full["status"] == TAIL_ROOM and full["tail_bytes"] == 100 and tail == b"" and behind["status"] == CHAIN
    assert again["status"] == OK and again["n_reads"] == 6 and tail2 == stream[s:cut]
    assert rest["status"] == OK and rest["n_reads"] == 1 and rest["tail_bytes"] == 0
    h_rec, h_off, h_names, _ = host_tables(host, tmp_path, recs)
    assert [int(x) - 256 for x in again["rec"]] == h_rec[:6] and [int(o) for o in again["off"]] == h_off[:7]


def test_a_refused_block_too_many_records_and_refused_arguments():
    rng = np.random.default_rng(9)
    stream = b"".join(wc.records(rng, 6))
    res = emu.run([emu.new(CAP), emu.submit(stream, block_status=[0, 0, 3, 0, 1]), emu.submit(b""), ("tail_set", b""),
                   emu.submit(stream, rec_cap=5), ("tail_set", b""), emu.submit(stream, rec_cap=6), emu.submit(stream, skip=len(stream) + 1),
                   emu.submit(stream, seg_bytes=32)])
    assert res[0]["status"] == BLOCK and res[0]["bad_index"] == 2 and res[1]["status"] == CHAIN
    assert res[2]["status"] == TOO_MANY and res[3]["status"] == OK and res[3]["n_reads"] == 6
    assert res[4]["rc"] == -1 and res[5]["rc"] == -1
