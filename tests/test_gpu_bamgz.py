"""-m gpu: gzip members of BAM batches, composed and deflated on the device (fpl_set_bam_gzip / fpl_wait_bam_gz, ABI v10;
csrc/gz_emit.h: k_gz_layout_bam, k_gz_compose_bam) through Engine and the CLI on the real library.

The expected bytes never come from the code under test: a member is inflated with zlib, gzip and libdeflate (CRC-32 and ISIZE
checked by each) and compared with what the host's formatter (fplh_format_batch) writes for the batch's FASTQ twin
(tests/bamio.py) and the records the call returned; records and counters are compared with the same batch through
fpl_process_batch_async on the twin's CSR arrays; the CLI's .gz is compared with the plain --out of the run on the twin, and
with the reference program on the twin."""
import gzip
import json
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, build, synth
from tests import bamio, hostio, refbin
from tests.gzcheck import host_format, inflate_all, load_hostlib
from tests.test_gpu_bam import fast_bam, twin_arrays

pytestmark = pytest.mark.gpu

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
SAID = b"output: gzip members deflated on the device"


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


def twin_text(recs):
    return b"".join(bamio.twin_record(*r) for r in recs)


def submit(eng, raw, starts, off, gzip_on=True, arrays=False):
    """-> (records array, (seq_out, qual_out) or None); everything is kept alive by the engine / the caller"""
    n = len(off) - 1
    res = np.zeros(n, abi.RESULT_DTYPE)
    bam = eng.pinned_array(max(len(raw), 1))
    bam[:len(raw)] = np.frombuffer(raw, np.uint8)
    outs = None
    if arrays:
        outs = (eng.pinned_array(int(off[-1]) + 1), eng.pinned_array(int(off[-1]) + 1))
        eng.submit_bam(bam[:len(raw)], starts, off, outs[0], outs[1], res, gzip=gzip_on)
    else:
        eng.submit_bam(bam[:len(raw)], starts, off, res=res, gzip=gzip_on)
    return res, outs


def csr_reference(engine_mod, opts, start, end, fasta, C, batches):
    """records and counters of the same batches through fpl_process_batch_async on the twin's CSR arrays"""
    b = engine_mod.Engine(abi.FplOptions.default(**opts), start, end, fasta, device=0, max_cycles=C)
    out = []
    for seq, qual, off in batches:
        rb = np.zeros(len(off) - 1, abi.RESULT_DTYPE)
        b.submit_host(seq, qual, off, rb)
        b.wait()
        out.append(rb)
    cnt = b.counters()
    b.close()
    return out, cnt


def one_batch(engine_mod, hostlib, tmp_path, raw, starts, recs, opts=C3, C=4096, arrays=False, start=synth.START_ADAPTER,
              end=synth.END_ADAPTER, fasta=()):
    seq, qual, off = twin_arrays(recs)
    members = []
    for rep in range(2):  # two runs give identical bytes
        eng = engine_mod.Engine(abi.FplOptions.default(**opts), start, end, list(fasta), device=0, max_cycles=C)
        res, outs = submit(eng, raw, starts, off, arrays=arrays and rep == 0)
        member = eng.wait()
        assert isinstance(member, bytes)
        if outs is not None:  # with seq_out given the decoded arrays still come back right
            n = int(off[-1])
            assert outs[0][:n].tobytes() == seq.tobytes() and outs[1][:n].tobytes() == qual.tobytes()
        members.append((member, res.tobytes(), eng.counters(), eng.gzip_batches()))
        eng.close()
    assert members[0][0] == members[1][0] and members[0][1] == members[1][1]
    (rb,), cnt = csr_reference(engine_mod, opts, start, end, list(fasta), C, [(seq, qual, off)])
    assert res.tobytes() == rb.tobytes()
    assert np.array_equal(members[0][2], cnt)
    want = host_format(hostlib, tmp_path, twin_text(recs), res)
    member = members[0][0]
    if want:
        assert members[0][3] == 1
        assert inflate_all(member, len(want)) == want
    else:
        assert member == b"" and members[0][3] == 0
    return member, res, want


def test_small_batch_both_strands(engine_mod, hostlib, tmp_path):
    rng = np.random.default_rng(21)
    raw, starts, recs = fast_bam(rng, 700, rng.integers(0, 3000, 50))
    member, res, want = one_batch(engine_mod, hostlib, tmp_path, raw, starts, recs, arrays=True)
    assert len(want) > 100_000


def test_planted_adapters_give_both_prefixes(engine_mod, hostlib, tmp_path):
    """ONT-like reads with middle adapters, stored as BAM with every third record reverse-complemented: split reads in the member"""
    seq, qual, off = synth.ont_like(400, seed=31, median_len=2500, p_middle=0.3, max_len=20000)
    fq, _, _ = hostio.make_fastq(seq, qual, off)
    recs = []
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(fq)):
        recs.append(bamio.reverse_record(name, codes, q) if i % 3 == 1 else (name, 0, codes, q))
    _, st, raw = bamio.bam_bytes(recs, n_cigar=1, tags=b"RGZx\0")
    member, res, want = one_batch(engine_mod, hostlib, tmp_path, raw, np.array(st, np.uint64), recs, C=20000)
    assert b"@split-by-adapter-left-" in want and b"@split-by-adapter-right-" in want


def test_one_batch_of_150000_reads(engine_mod, hostlib, tmp_path):
    rng = np.random.default_rng(22)
    raw, starts, recs = fast_bam(rng, 150_000, rng.integers(20, 400, 97))
    seq, qual, off = twin_arrays(recs)
    eng = engine_mod.Engine(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=512)
    res, _ = submit(eng, raw, starts, off)
    member = eng.wait()
    forms = eng.batch_forms()
    assert forms["trim_batched"] >= 1 and forms["stats_sorted"] >= 1, forms
    cnt = eng.counters()
    assert eng.gzip_batches() == 1
    eng.close()
    (rb,), cb = csr_reference(engine_mod, C3, synth.START_ADAPTER, synth.END_ADAPTER, [], 512, [(seq, qual, off)])
    assert res.tobytes() == rb.tobytes() and np.array_equal(cnt, cb)
    want = host_format(hostlib, tmp_path, twin_text(recs), res)
    assert len(want) > 1_000_000 and inflate_all(member, len(want)) == want


def test_three_in_flight_gzip_bam_plain_bam_text_gzip_and_an_empty_output(engine_mod, hostlib, tmp_path):
    rng = np.random.default_rng(23)
    b0 = fast_bam(rng, 500, rng.integers(0, 3000, 41))
    b1 = fast_bam(rng, 300, rng.integers(0, 2000, 37))
    seq2, qual2, off2 = synth.ont_like(300, seed=24, median_len=2000, p_middle=0.2, max_len=20000)
    text2 = hostio.make_fastq(seq2, qual2, off2)[0]
    eng = engine_mod.Engine(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=20000)
    s0, q0, o0 = twin_arrays(b0[2])
    s1, q1, o1 = twin_arrays(b1[2])
    r0, _ = submit(eng, b0[0], b0[1], o0)
    r1, outs1 = submit(eng, b1[0], b1[1], o1, gzip_on=False, arrays=True)
    tbuf = eng.pinned_array(len(text2))
    tbuf[:] = np.frombuffer(text2, np.uint8)
    eng.submit_text(tbuf, gzip=True)
    assert eng.in_flight() == 3
    m0 = eng.wait()
    m1 = eng.wait()
    info, r2, lines, m2 = eng.wait_text()
    assert isinstance(m0, bytes) and m1 is None and eng.gzip_batches() == 2
    cnt = eng.counters()
    eng.close()
    assert outs1[0][:int(o1[-1])].tobytes() == s1.tobytes() and outs1[1][:int(o1[-1])].tobytes() == q1.tobytes()
    want0 = host_format(hostlib, tmp_path, twin_text(b0[2]), r0)
    assert len(want0) > 50_000 and inflate_all(m0, len(want0)) == want0
    want2 = host_format(hostlib, tmp_path, text2, r2)
    assert inflate_all(m2, len(want2)) == want2
    rbs, cb = csr_reference(engine_mod, C3, synth.START_ADAPTER, synth.END_ADAPTER, [], 20000,
                            [(s0, q0, o0), (s1, q1, o1), (seq2, qual2, off2)])
    assert r0.tobytes() == rbs[0].tobytes() and r1.tobytes() == rbs[1].tobytes() and r2.tobytes() == rbs[2].tobytes()
    assert np.array_equal(cnt, cb)
    # a gzip batch collected with the plain wait: its bytes are never made
    eng = engine_mod.Engine(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=20000)
    r0b, _ = submit(eng, b0[0], b0[1], o0, arrays=True)
    assert eng.wait(member=False) is None and eng.gzip_batches() == 0 and r0b.tobytes() == r0.tobytes()
    eng.close()
    # nothing passes: a required length no read has
    member, res, want = one_batch(engine_mod, hostlib, tmp_path, *b0, opts=dict(required_length=10_000_000))
    assert member == b"" and want == b""


def test_null_arrays_need_the_switch(engine_mod):
    rng = np.random.default_rng(25)
    raw, starts, recs = fast_bam(rng, 10, [100])
    _, _, off = twin_arrays(recs)
    eng = engine_mod.Engine(abi.FplOptions.default(), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=512)
    bam = eng.pinned_array(len(raw))
    bam[:] = np.frombuffer(raw, np.uint8)
    res = np.zeros(10, abi.RESULT_DTYPE)
    so = eng.pinned_array(2000)
    rc = eng.L.fpl_process_bam_async(eng.h, bam.ctypes.data, len(bam), starts.ctypes.data, off.ctypes.data, 10, None, None, res.ctypes.data)
    assert rc == abi.FPL_ERR_ARG  # the switch is off
    assert eng.L.fpl_set_bam_gzip(eng.h, 1) == 0
    rc = eng.L.fpl_process_bam_async(eng.h, bam.ctypes.data, len(bam), starts.ctypes.data, off.ctypes.data, 10, so.ctypes.data, None, res.ctypes.data)
    assert rc == abi.FPL_ERR_ARG  # both or neither
    assert eng.in_flight() == 0
    eng.close()
    eng = engine_mod.Engine(abi.FplOptions.default(break_enabled=1), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=512)
    assert eng.L.fpl_set_bam_gzip(eng.h, 1) == abi.FPL_ERR_STATE  # --break / --mask write from fragment lists
    eng.close()


def test_long_reads_of_200_kb_and_1_2_mb(engine_mod, hostlib, tmp_path):
    rng = np.random.default_rng(26)
    raw, starts, recs = fast_bam(rng, 6, [200_000, 1_200_000, 0, 1, 1_199_999, 199_999], flags=(0, 0x10, 0, 0x10, 0, 0x10))
    member, res, want = one_batch(engine_mod, hostlib, tmp_path, raw, starts, recs, opts=dict(adapter_enabled=0, qual_filter=0, length_filter=0),
                                  C=1_200_000)
    assert len(want) > 2 * 2_700_000


def _workload(kind, n, seed):
    """the reads of bench.py's workloads, as tests/test_gpu_gz.py builds them"""
    if kind == "c5_hifi64":
        seq, qual, off, ads = synth.hifi_like(n, seed=seed, mean_len=20000, sd_len=2000, n_adapters=64)
        return seq, qual, off, dict(), ads[0], synth.revcomp(ads[0]), list(ads)
    if kind == "c4_mixed":
        seq, qual, off = synth.ont_like(n, seed=seed, median_len=6673, sigma_len=0.9, min_len=200, max_len=200_000)
    else:
        seq, qual, off = synth.ont_like(n, seed=seed, median_len=8000, sigma_len=0.5)
    return seq, qual, off, (dict() if kind == "c2_adapter_only" else C3), synth.START_ADAPTER, synth.END_ADAPTER, []


@pytest.mark.parametrize("kind", ["c3_full_pipeline", "c2_adapter_only", "c4_mixed", "c5_hifi64"])
def test_member_size_against_zlib_level_1(engine_mod, hostlib, tmp_path, kind):
    """the bound the text form is held to (tests/test_gpu_gz.py): the composed bytes and the block coder are the same"""
    seq, qual, off, opts, start, end, fasta = _workload(kind, 700, 3)
    fq, _, _ = hostio.make_fastq(seq, qual, off)
    recs = [bamio.reverse_record(n, c, q) if i % 2 else (n, 0, c, q) for i, (n, _, c, q) in enumerate(bamio.fastq_to_records(fq))]
    _, st, raw = bamio.bam_bytes(recs)
    s2, q2, o2 = twin_arrays(recs)
    C = int(np.diff(o2.astype(np.int64)).max())
    eng = engine_mod.Engine(abi.FplOptions.default(**opts), start, end, fasta, device=0, max_cycles=C)
    res, _ = submit(eng, raw, np.array(st, np.uint64), o2)
    member = eng.wait()
    eng.close()
    want = host_format(hostlib, tmp_path, twin_text(recs), res)
    assert len(want) > len(fq) // 4
    assert inflate_all(member, len(want)) == want
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    l1 = len(c.compress(want) + c.flush())
    print("%s: text out %d, member %d, raw level 1 %d (%.3f x)" % (kind, len(want), len(member), l1, len(member) / l1))
    assert len(member) <= 1.05 * l1


def _members(data):
    got, n, rest = b"", 0, data
    while rest:
        d = zlib.decompressobj(31)
        got += d.decompress(rest) + d.flush()
        assert d.eof
        rest = d.unused_data
        n += 1
    return got, n


@pytest.mark.parametrize("chunk", ["20000", None])  # many batches / one batch
@pytest.mark.parametrize("case", ["c1_qualfilter", "c3_full", "c5_fasta"])
def test_cli_bam_to_gz_on_the_device(engine_mod, tmp_path, case, chunk):
    from tests.test_cli_bamgz_stub import case_bam, flags_of, reports

    build.build_all()
    bam, twin = case_bam(tmp_path, case)
    fl = flags_of(case)
    env = dict(os.environ)
    if chunk:
        env["FPLH_CHUNK_BYTES"] = chunk

    def cli(src, d, out, extra=()):
        d.mkdir(exist_ok=True)
        cmd = [build.CLI, "-i", str(src), "-o", str(d / out), "-j", str(d / "out.json"), "-h", str(d / "out.html"), "-V"] + fl + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stderr

    cli(twin, tmp_path / "fq", "out.fq")
    want = (tmp_path / "fq" / "out.fq").read_bytes()
    err = cli(bam, tmp_path / "bam", "out.fq.gz", ["--device_gzip"])
    data = (tmp_path / "bam" / "out.fq.gz").read_bytes()
    got, n_members = _members(data)
    assert len(want) > 1000 and got == want
    assert reports(tmp_path / "bam") == reports(tmp_path / "fq")
    assert SAID in err
    n = int(re.search(rb"device gzip: (\d+) members", err).group(1))
    assert n == n_members and n >= (3 if chunk else 1)
    assert data.count(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff") >= n  # (the device's header: no time, unknown system)
    # the host's deflate gives the same text
    err = cli(bam, tmp_path / "host", "out.fq.gz")  # (without the flag: the host's deflate)
    assert SAID not in err and gzip.decompress((tmp_path / "host" / "out.fq.gz").read_bytes()) == want
    # the project's own reader takes the file back
    cli(tmp_path / "bam" / "out.fq.gz", tmp_path / "z", "second.fq", ["--host_parse"])
    cli(tmp_path / "fq" / "out.fq", tmp_path / "p", "second.fq", ["--host_parse"])
    assert (tmp_path / "z" / "second.fq").read_bytes() == (tmp_path / "p" / "second.fq").read_bytes()
    # --failed_out: formatted on the host from the decoded arrays, --out still the device's members
    cli(twin, tmp_path / "fq2", "out.fq", ["--failed_out", str(tmp_path / "fq2" / "f.fq")])
    err = cli(bam, tmp_path / "bam2", "out.fq.gz", ["--device_gzip", "--failed_out", str(tmp_path / "bam2" / "f.fq")])
    assert SAID in err and _members((tmp_path / "bam2" / "out.fq.gz").read_bytes())[0] == want
    assert (tmp_path / "bam2" / "f.fq").read_bytes() == (tmp_path / "fq2" / "f.fq").read_bytes()


def test_cli_bam_to_gz_vs_ref_binary_on_the_twin(engine_mod, orc, tmp_path):
    """the reference program on the BAM's FASTQ twin against the CLI on the BAM with -o out.fq.gz: --out and fastplong.json"""
    if not orc.have_ref_bin():
        pytest.skip("oracle/_ref/fastplong_ref not built (needs the reference's sources at build time)")
    build.build_all()
    seq, qual, off = refbin.reads("dna", n=300, seed=5)
    fq, _, _ = hostio.make_fastq(seq, qual, off)
    recs = []
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(fq)):
        name = name.replace(b" ", b"_")
        recs.append(bamio.reverse_record(name, codes, q) if i % 3 == 1 else (name, 0x4, codes, q))
        if i % 5 == 2:
            recs.append((name + b"_sec", 0x100, codes[:50], q[:50]))
    data, _, _ = bamio.bam_bytes(recs, block=6000)
    (tmp_path / "x.bam").write_bytes(data)
    (tmp_path / "twin.fq").write_bytes(bamio.bam_to_fastq(data))
    fl = refbin.flags_of("full", tmp_path)
    refbin.run_ref(tmp_path / "twin.fq", tmp_path / "ref", fl)
    d = tmp_path / "cli"
    d.mkdir()
    cmd = [build.CLI, "-i", str(tmp_path / "x.bam"), "-o", str(d / "out.fq.gz"), "-j", str(d / "out.json"), "-h", str(d / "out.html"), "-w", "4",
           "-V", "--device_gzip"] + fl
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, FPLH_CHUNK_BYTES="40000"), cwd=str(d))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    assert SAID in p.stderr
    got, n = _members((d / "out.fq.gz").read_bytes())
    ref = refbin.outputs(tmp_path / "ref")
    assert n >= 3 and got == ref["out.fq"]
    js = [l for l in (d / "out.json").read_bytes().split(b"\n") if not l.startswith(b'\t"command":')]
    assert js == ref["json"]
