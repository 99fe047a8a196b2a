"""BAM input on the MI355X: fpl_decode_bam bit-exact with bamio's twin (200 kb and 1.2 Mb reads, every code, both strands);
fpl_process_bam_async equal to fpl_process_batch_async on the twin's CSR -- records, fragments, the whole counter buffer --
on a small batch, on a batch of 150 000 reads (the batched trim and sorted statistics forms) and with three batches in
flight; and the CLI on a BAM twin of each golden case reproducing the twin's FASTQ run byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, build, engine, synth
from tests import bamio, parity

pytestmark = pytest.mark.gpu


def fast_bam(rng, n, lengths, flags=(0, 0x10)):
    """(raw record stream without header, record starts, records) built with numpy: many reads quickly"""
    parts, starts, recs, pos = [], [], [], 0
    for i in range(n):
        L = int(lengths[i % len(lengths)])
        codes = rng.integers(0, 16, L, dtype=np.uint8)
        if L % 2:
            pk = np.append(codes, 0)
        else:
            pk = codes
        packed = ((pk[0::2] << 4) | pk[1::2]).astype(np.uint8).tobytes()
        qual = rng.integers(0, 120, L, dtype=np.uint8).tobytes()
        flag = int(flags[i % len(flags)])
        name = b"q%d\0" % i
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, flag, L, -1, -1, 0) + name + packed + qual
        rec = struct.pack("<I", len(body)) + body
        starts.append(pos)
        parts.append(rec)
        pos += len(rec)
        recs.append((name[:-1], flag, codes.tobytes(), qual))
    return b"".join(parts), np.array(starts, np.uint64), recs


def twin_arrays(recs):
    seqs, quals = [], []
    for r in recs:
        t = bamio.twin_record(*r).split(b"\n")
        seqs.append(t[1])
        quals.append(t[3])
    off = np.zeros(len(recs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8), np.frombuffer(b"".join(quals), np.uint8), off


def test_decode_bam_long_reads_bit_exact():
    rng = np.random.default_rng(7)
    raw, starts, recs = fast_bam(rng, 8, [200_000, 1_200_000, 1, 0, 199_999, 17, 1_199_999, 64], flags=(0, 0x10, 0x10, 0))
    seq, qual, off = twin_arrays(recs)
    got_s, got_q = engine.decode_bam(0, np.frombuffer(raw, np.uint8), starts, off)
    assert got_s.tobytes() == seq.tobytes()
    assert got_q.tobytes() == qual.tobytes()
    # the small records of bamio's generator: all codes, qualities up to 254, lengths 0 / 1 / odd / even, CIGAR and tags
    recs = bamio.random_records(np.random.default_rng(3), 3000, max_len=500)
    data, st, raw = bamio.bam_bytes(recs, n_cigar=2, tags=b"XYZabc")
    keep = [i for i, r in enumerate(recs) if not (r[1] & 0x900)]
    seq, qual, off, _ = bamio.twin_csr(data)
    got_s, got_q = engine.decode_bam(0, np.frombuffer(raw, np.uint8), np.array([st[i] for i in keep], np.uint64), off)
    assert got_s.tobytes() == seq.tobytes() and got_q.tobytes() == qual.tobytes()


def _opt(**kw):
    return abi.FplOptions.default(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1, **kw)


def _pair(opt, batches, C):
    """the same batches through fpl_process_bam_async and fpl_process_batch_async on two contexts, all in flight at once"""
    a = engine.Engine(opt, synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=C)
    b = engine.Engine(opt, synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=C)
    keep, out = [], []
    for raw, starts, recs in batches:
        seq, qual, off = twin_arrays(recs)
        n = len(recs)
        ra = np.zeros(n, abi.RESULT_DTYPE)
        rb = np.zeros(n, abi.RESULT_DTYPE)
        so = a.pinned_array(int(off[-1]) + 1)
        qo = a.pinned_array(int(off[-1]) + 1)
        bam = a.pinned_array(len(raw))
        bam[:] = np.frombuffer(raw, np.uint8)
        a.submit_bam(bam, starts, off, so, qo, ra)
        b.submit_host(seq, qual, off, rb)
        keep.append((seq, qual, off, starts))
        out.append((ra, rb, so, qo, seq, qual, off))
    for _ in batches:
        a.wait()
        b.wait()
    return a, b, out


def test_process_bam_equals_csr_small_and_three_in_flight():
    rng = np.random.default_rng(11)
    batches = [fast_bam(rng, 700, rng.integers(0, 3000, 50)) for _ in range(3)]
    a, b, out = _pair(_opt(), batches, 4096)
    for ra, rb, so, qo, seq, qual, off in out:
        n = int(off[-1])
        assert so[:n].tobytes() == seq.tobytes() and qo[:n].tobytes() == qual.tobytes()
        assert ra.tobytes() == rb.tobytes()
    assert np.array_equal(a.counters(), b.counters())
    a.close()
    b.close()


def test_process_bam_fragments_equal_csr():
    rng = np.random.default_rng(12)
    batches = [fast_bam(rng, 400, rng.integers(0, 2500, 40))]
    a, b, out = _pair(_opt(break_enabled=1, break_window=40, break_quality=55, mask_enabled=1, mask_window=15, mask_quality=58),
                      batches, 4096)
    ra, rb = out[0][0], out[0][1]
    assert ra.tobytes() == rb.tobytes()
    fa, fb = a.fragments(), b.fragments()
    assert len(fa[0]) > 0
    parity.assert_fragments_equal(fa[0], fa[1], fb[0], fb[1])  # (the region list's layout may differ: compared per fragment)
    assert np.array_equal(a.counters(), b.counters())
    a.close()
    b.close()


def test_process_bam_equals_csr_150k_reads():
    rng = np.random.default_rng(13)
    batches = [fast_bam(rng, 150_000, rng.integers(20, 400, 97))]
    a, b, out = _pair(_opt(), batches, 512)
    ra, rb, so, qo, seq, qual, off = out[0]
    n = int(off[-1])
    assert so[:n].tobytes() == seq.tobytes() and qo[:n].tobytes() == qual.tobytes()
    assert ra.tobytes() == rb.tobytes()
    assert np.array_equal(a.counters(), b.counters())
    forms = a.batch_forms()
    assert forms["trim_batched"] >= 1 and forms["stats_sorted"] >= 1, forms  # k_trim_ends_batched and k_stats_sorted taken
    a.close()
    b.close()


def test_cli_bam_twin_of_golden_cases_on_the_library(tmp_path):
    from tests.test_cli_bam_stub import CASES, case_bam, flags_of, outputs
    build.build_host()
    for case in CASES:
        d = tmp_path / case
        d.mkdir()
        bam, twin = case_bam(d, case)
        res = {}
        for tag, inp in (("fq", twin), ("bam", bam)):
            o = d / tag
            o.mkdir()
            cmd = [build.CLI, "-i", str(inp), "-o", str(o / "out.fq"), "--failed_out", str(o / "failed.fq"), "-j", str(o / "out.json"),
                   "-h", str(o / "out.html")] + flags_of(case)
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                               env=dict(os.environ, FPLH_CHUNK_BYTES="30000"))
            assert p.returncode == 0, p.stderr.decode()[-3000:]
            res[tag] = outputs(o)
        assert res["bam"] == res["fq"], case
