"""The HIP kernels against the whole reference program (oracle/_ref/fastplong_ref, compiled from the reference's own sources
by oracle.build()): per-read trimming decisions of the real library, formatted as --out / --failed_out, byte for byte against
what the reference writes for the same FASTQ.  Skipped where the reference program was not built.

  * the flag matrix of tests/refbin.py through bin/fastplong_amd on the real library: device-parse mode, --host_parse, and
    small FPLH_CHUNK_BYTES chunks whose cuts fall inside records; a BAM input against the reference's run on its FASTQ twin;
  * adapter batteries aimed at k_scan / k_resolve / k_redo and the end-trim kernels: adapter lengths around every form switch
    (the <= 32-base SHORT scan and six count planes, the 16-base carry-save groups, the 64-base limit of the fast Hamming scan,
    the short and mid end-trim modes), each length with an A / C / G / T-only pair (the fast forms where the length allows
    them) and with an N / lower-case pair (the byte-wise forms), copies with 0, thr and
    thr + 1 substitutions at and next to the 32-byte chunk and 1 984-byte tile boundaries of k_scan and at the last windows,
    periodic / homopolymer / N and lower-case adapters, reads of 100 kb to 1.2 Mb with the hit in the last tile -- once with
    the suite's hooks and once without;
  * one bench-sized batch (160 000 reads) with no hooks, through Engine and through the CLI."""
import os

import numpy as np
import pytest

from fastplong_amd import abi, build, synth
from tests import bamio, hostio, refbin
from tests import second_reading as sr

pytestmark = pytest.mark.gpu

SCAN_CHUNK = 32  # bytes of a k_scan chunk
SCAN_TILE = 1984  # bytes of a k_scan tile (62 lanes x 32)
# around the forms: <= 32 bases both adapters -> scan_short / six planes; 16-base CSA groups; <= 64 bases -> fast Hamming;
# 16..32 / 16..64 bases -> the short / mid end-trim modes
ALENS = (4, 5, 7, 8, 15, 16, 17, 24, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 250)
THREADS = 8


@pytest.fixture(scope="module")
def engine_mod(orc):
    import torch

    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    if not orc.have_ref_bin():
        pytest.skip("oracle/_ref/fastplong_ref not built (needs the reference's sources at build time)")
    from fastplong_amd import engine

    engine.load_library()
    build.build_host()
    return engine


def _subst(rng, ad, k):
    b = bytearray(ad)
    for i in rng.choice(len(b), size=min(k, len(b)), replace=False) if k else ():
        c = chr(b[i]).upper()
        b[i] = b"ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4] if c in "ACGT" else ord("A")
    return bytes(b)


def _rnd(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n))].tobytes()


def _engine_vs_ref(engine_mod, tmp_path, tag, seq, qual, off, start, end, ed=0.3, ext=10):
    """the batch through Engine (host buffers in) and through the reference on its FASTQ: --out / --failed_out equal"""
    d = tmp_path / tag
    d.mkdir()
    text, names, strands = hostio.make_fastq(seq, qual, off)
    (d / "in.fq").write_bytes(text)
    flags = ["-s", start, "-e", end, "-d", repr(ed), "--trimming_extension", str(ext)]
    refbin.run_ref(d / "in.fq", d / "ref", flags, threads=THREADS)
    C = max(1, int(np.diff(off.astype(np.int64)).max()))
    eng = engine_mod.Engine(abi.FplOptions.default(ed_max=ed, trimming_extension=ext), start, end, device=0, max_cycles=C)
    res = eng.process_host(seq, qual, off)
    forms = eng.batch_forms()
    eng.close()
    out, failed = hostio.expected_outputs(seq, qual, off, names, strands, res)
    want = {"out": (d / "ref" / "out.fq").read_bytes(), "failed": (d / "ref" / "failed.fq").read_bytes()}
    refbin.assert_same({"out": out, "failed": failed}, want)
    return res, forms


def _pairs(rng, alen):
    """the (start, end) adapter pairs a length is run with: both A / C / G / T only (the end one periodic or a homopolymer),
    which the library scans with its fast forms; the end one of another ACGT length on the other side of 32 (SHORT scan
    off, fast Hamming on); and the end one holding N and lower case, which sends the batch through the byte-wise scan and
    the general trims"""
    A = _rnd(rng, alen)
    E = (_rnd(rng, 2) * alen)[:alen] if alen % 2 else _rnd(rng, 1) * alen
    other = _rnd(rng, 33 if alen <= 32 else 32)
    odd = bytearray(_rnd(rng, alen))
    odd[alen // 3] = ord("N")
    odd[alen // 2:alen // 2 + 3] = bytes(odd[alen // 2:alen // 2 + 3]).lower()
    return [(A, E), (A, other), (A, bytes(odd))]


def _forms(A, E):
    """(ham_fast, scan_short, trim_mode) the library picks for a start / end adapter pair: an adapter counts as A / C / G / T
    only up to 64 bases (build_adapter, csrc/dev_types.h); ham_fast = both such; scan_short = ham_fast and both <= 32 bases
    (fpl_create, csrc/fpl_hip.hip); trim_mode 1 (short) = both 16..32 bases, 2 (mid) = both 16..64, else 0 (trim_mode_of)"""
    acgt = [len(x) <= 64 and all(c in b"ACGT" for c in x) for x in (A, E)]
    ham_fast = all(acgt)
    scan_short = ham_fast and len(A) <= 32 and len(E) <= 32
    short = all(acgt) and all(16 <= len(x) <= 32 for x in (A, E))
    mid = all(acgt) and all(16 <= len(x) <= 64 for x in (A, E))
    return ham_fast, scan_short, 1 if short else (2 if mid else 0)


def _battery(rng, A, E, ed):
    """reads for one adapter pair: copies with 0, thr and thr + 1 substitutions planted around the scan's chunk and tile
    boundaries and at the last windows, and end-adapter pieces at both ends"""
    alen = len(A)
    thr = sr.c_round(ed * alen)
    subs = sorted({0, thr, thr + 1})
    reads = []
    bounds = [SCAN_CHUNK * k + d for k in (1, 2, 7) for d in (-1, 0, 1)] + [SCAN_TILE * k + d for k in (1, 2) for d in (-1, 0, 1)]
    for ad in (A, E):
        for p in bounds:
            for at in (p, max(0, p - len(ad))):  # the copy starting at, or ending at, the boundary
                for s in subs:
                    L = at + len(ad) + int(rng.choice([0, 1, 2, 37, 250, SCAN_TILE]))
                    body = bytearray(_rnd(rng, L))
                    body[at:at + len(ad)] = _subst(rng, ad, s)
                    reads.append(bytes(body))
    for k in (1, 2, 3):  # the copy at the last window (never visited by the middle search) and the one before it
        for dl in (-1, 0, 1, 5):
            L = SCAN_TILE * k + dl
            for back in (0, 1, 2, 11):
                for ad in (A, E):
                    if L < len(ad) + back:
                        continue
                    body = bytearray(_rnd(rng, L))
                    at = L - len(ad) - back
                    body[at:at + len(ad)] = _subst(rng, ad, int(rng.choice(subs)))
                    reads.append(bytes(body))
    for _ in range(40):  # end adapters on both ends, as the end trims see them
        L = int(rng.integers(16, 3000))
        body = _subst(rng, A, int(rng.choice(subs)))[:int(rng.integers(1, len(A) + 1))] + _rnd(rng, L) + \
            _subst(rng, E, int(rng.choice(subs)))[:int(rng.integers(1, len(E) + 1))]
        reads.append(body)
    quals = [bytes(np.clip(rng.normal(22, 6, len(r)), 3, 40).astype(np.uint8) + 33) for r in reads]
    seq, qual, off = synth.pack([(np.frombuffer(r, np.uint8), np.frombuffer(q, np.uint8)) for r, q in zip(reads, quals)])
    return seq, qual, off


@pytest.mark.parametrize("hooks", ["suite_hooks", "plain_scan"])
def test_adapter_batteries_vs_ref_binary(tmp_path, engine_mod, monkeypatch, hooks):
    """k_scan / k_resolve / k_redo and the end trims on planted copies around every form switch and tile boundary: every
    length with an A / C / G / T pair (the fast forms where the length allows them) and with an N / lower-case pair"""
    if hooks == "plain_scan":
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)
    rng = np.random.default_rng(9100)
    split = 0
    ran = set()
    for alen in ALENS:
        for ed in ((0.3, 0.25) if alen in (8, 16, 32, 33, 64) else (0.3,)):
            for i, (A, E) in enumerate(_pairs(rng, alen)):
                seq, qual, off = _battery(rng, A, E, ed)
                res, _ = _engine_vs_ref(engine_mod, tmp_path, "a%d_%g_%d" % (alen, ed, i), seq, qual, off, A.decode("latin-1"),
                                        E.decode("latin-1"), ed=ed)
                split += int((res["n_frag"] == 2).sum())
                ran.add((alen,) + _forms(A, E))
    assert split > 200
    # both sides of every switch took the form it should: the SHORT scan (six count planes) up to 32 bases, fast Hamming up
    # to 64, the short end-trim mode for 16..32, the mid one for 16..64, and the byte-wise forms at every length
    for alen in ALENS:
        assert (alen, False, False, 0) in ran, alen
    for alen in (4, 5, 7, 8, 15, 16, 17, 24, 31, 32):
        assert any(r[0] == alen and r[2] for r in ran), alen
    for alen in (33, 47, 48, 49, 63, 64):
        assert (alen, True, False, 2) in ran, alen
    for alen in (16, 17, 24, 31, 32):
        assert (alen, True, True, 1) in ran and (alen, True, False, 2) in ran, alen
    for alen in (65, 100, 250):
        assert not any(r[0] == alen and r[1] for r in ran), alen


@pytest.mark.parametrize("hooks", ["suite_hooks", "plain_scan"])
def test_long_reads_hit_in_the_last_tile_vs_ref_binary(tmp_path, engine_mod, monkeypatch, hooks):
    """reads of 100 kb to 1.2 Mb with a middle-adapter copy in (or ending at) the last tile"""
    if hooks == "plain_scan":
        monkeypatch.delenv("FPL_TRIM_BATCH_MIN", raising=False)
        monkeypatch.delenv("FPL_SCAN_CHUNK", raising=False)
    rng = np.random.default_rng(9200)
    A, E = synth.START_ADAPTER.encode(), synth.END_ADAPTER.encode()
    reads = []
    for L, back, ad, s in ((100_000, 0, A, 0), (100_001, 1, E, 2), (131_072, 40, A, 7), (262_143, SCAN_TILE - 30, E, 0),
                           (500_000, 3, A, 8), (1_200_000, 2, A, 1), (1_200_000 - 17, 0, E, 0)):
        body = bytearray(_rnd(rng, L))
        at = L - len(ad) - back
        body[at:at + len(ad)] = _subst(rng, ad, s)
        reads.append(bytes(body))
    for _ in range(20):
        reads.append(_rnd(rng, int(rng.integers(50, 5000))))
    quals = [bytes(np.clip(rng.normal(22, 6, len(r)), 3, 40).astype(np.uint8) + 33) for r in reads]
    seq, qual, off = synth.pack([(np.frombuffer(r, np.uint8), np.frombuffer(q, np.uint8)) for r, q in zip(reads, quals)])
    res, _ = _engine_vs_ref(engine_mod, tmp_path, "long", seq, qual, off, synth.START_ADAPTER, synth.END_ADAPTER)
    assert (res["n_frag"][:7] == 2).sum() >= 4


@pytest.mark.parametrize("mode", ["device_parse", "host_parse", "small_chunks"])
def test_cli_matrix_vs_ref_binary(tmp_path, engine_mod, mode):
    """the flag matrix of tests/refbin.py on the real library: every output byte for byte against the reference program"""
    extra_env = {"FPLH_CHUNK_BYTES": "30000"} if mode == "small_chunks" else {}
    extra_flags = ["--host_parse"] if mode == "host_parse" else []
    for name in sorted(refbin.CASES):
        d = tmp_path / name
        d.mkdir()
        refbin.write_input(d / "in.fq", refbin.CASES[name][0])
        fl = refbin.flags_of(name, d)
        pr = refbin.run_ref(d / "in.fq", d / "ref", fl)
        pc = refbin.run_cli(os.environ, d / "in.fq", d / "cli", fl, extra_env=extra_env, extra_flags=extra_flags)
        try:
            refbin.assert_same(refbin.outputs(d / "cli"), refbin.outputs(d / "ref"))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        if name.startswith("auto"):
            assert refbin.detection_lines(pc) == refbin.detection_lines(pr), name


def test_cli_bam_vs_ref_binary_on_the_twin(tmp_path, engine_mod):
    """a BAM input (some records reverse-strand, secondary / supplementary ones skipped) through the real library against
    the reference program on the BAM's FASTQ twin"""
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
    refbin.run_cli(os.environ, tmp_path / "x.bam", tmp_path / "cli", fl, extra_env={"FPLH_CHUNK_BYTES": "40000"})
    refbin.assert_same(refbin.outputs(tmp_path / "cli"), refbin.outputs(tmp_path / "ref"))


def test_bench_sized_batch_no_hooks_vs_ref_binary(tmp_path, engine_mod, monkeypatch):
    """160 000 reads in one batch with no hooks: k_trim_ends_batched and k_stats_sorted are taken, and the outputs equal the
    reference's; then the same file through the CLI in one chunk"""
    for k in ("FPL_TRIM_BATCH_MIN", "FPL_SCAN_CHUNK", "FPL_STATS_SORT_MIN"):
        monkeypatch.delenv(k, raising=False)
    seq, qual, off = synth.ont_like(160_000, seed=31, median_len=350, sigma_len=0.6, min_len=20, max_len=6000, p_middle=0.2)
    res, forms = _engine_vs_ref(engine_mod, tmp_path, "bench", seq, qual, off, synth.START_ADAPTER, synth.END_ADAPTER)
    assert forms["trim_batched"] == 1 and forms["stats_sorted"] == 1 and forms["reads"] == 160_000, forms
    assert (res["n_frag"] == 2).sum() > 1000
    d = tmp_path / "bench"
    fl = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER]
    refbin.run_ref(d / "in.fq", d / "ref2", fl, threads=THREADS)
    refbin.run_cli(os.environ, d / "in.fq", d / "cli", fl, threads=THREADS, extra_flags=["--chunk_mb", "1024"])
    refbin.assert_same(refbin.outputs(d / "cli"), refbin.outputs(d / "ref2"))
