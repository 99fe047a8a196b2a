"""-m gpu: the gzip batches' bytes as unaligned BAM records in BGZF blocks (fpl_set_gzip_records; csrc/bam_emit.h: k_bamout_layout,
k_bamout_compose and their BAM-source forms, then the BGZF block kernels) through Engine and the CLI on the real library.

Every output is BGZF blocks of 49 152 record bytes (the last one short) that gzip.decompress takes one by one; joined they are,
byte for byte, what the host's converter (fplh::fastq_to_bam_records, pinned against plain Python in tests/test_host_bam_out.py)
and tests/bam_out_cases.py's own restatement of the rule make of the host-formatted text of the same records; with the header block
and the EOF block around them tests/bamio.py reads the file back; the device's own inflater (Inflater.inflate) returns status 0 for
every block.  Size condition (tests/test_bam_out_emu.py): output <= total + 5 * deflate blocks + 31 * ceil(total / 49 152), the
deflate blocks counted from the cut rule in Python."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bam_out_cases as bc
from tests import bamio, hostio
from tests.bgzf_out_cases import STRIPE, exact_text, forced_starts_text, one_long_read_text, short_reads_text
from tests.gzcheck import GOLD, gz, host_format, inflate_all, load_hostlib

pytestmark = pytest.mark.gpu

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
PLAIN = dict(adapter_enabled=0, qual_filter=0, length_filter=0)  # the output is the input


@pytest.fixture(scope="module")
def hostlib():
    L = load_hostlib()
    L.fplh_fastq_to_bam_records.restype = C.c_int
    L.fplh_fastq_to_bam_records.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    return L


@pytest.fixture(scope="module")
def engine_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fastplong_amd import engine

    return engine


@pytest.fixture(scope="module")
def inflater(engine_mod):
    inf = engine_mod.Inflater(0)
    yield inf
    inf.close()


def host_records(L, text):
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_fastq_to_bam_records(text, len(text), C.byref(out), C.byref(n)) == 0
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    return s


def pinned(eng, data):
    a = eng.pinned_array(max(len(data), 1))
    a[:len(data)] = np.frombuffer(data, np.uint8)
    return a[:len(data)]


def new_engine(engine_mod, opts, bam=True, C=20480):
    adapters = ("", "") if opts is PLAIN else (synth.START_ADAPTER, synth.END_ADAPTER)
    eng = engine_mod.Engine(abi.FplOptions.default(**opts), adapters[0], adapters[1], device=0, max_cycles=C)
    if bam:
        eng.set_gzip_records(True)
    return eng


def check_device_bytes(hostlib, inflater, data, formatted, label, readable=True):
    """the checks of the module's docstring -> the records' bytes"""
    want = host_records(hostlib, formatted)
    assert want == bc.records(formatted)
    if not want:
        assert data == b""
        return want
    blocks = bc.check_device_blocks(data, want)
    desc, _ = bgzf.blocks(data)
    out, status = inflater.inflate(np.frombuffer(data, np.uint8), desc)
    assert len(status) == len(blocks) and (status == 0).all(), status
    assert out.tobytes() == want
    nb, total = bc.deflate_blocks(formatted)
    print("%s: records %d (text %d), BGZF %d in %d blocks of %d deflate blocks" % (label, total, len(formatted), len(data), len(blocks), nb))
    assert total == len(want) and len(data) <= total + 5 * nb + 31 * len(blocks)
    if readable:
        assert bamio.bam_to_fastq(bc.file_bytes(data)) == bc.cut_text(formatted)
        assert bamio.bam_to_fastq(bgzf.bam_header() + data + bgzf.eof()) == bc.cut_text(formatted)  # a library caller's file
    return want


def text_case(engine_mod, hostlib, inflater, tmp_path, text, opts, label, C=20480, readable=True):
    eng = new_engine(engine_mod, opts, True, C)
    eng.submit_text(pinned(eng, text), gzip=True)
    info, res, lines, data = eng.wait_text()
    n_gz = eng.gzip_batches()
    eng.close()
    assert info["status"] == abi.FPL_TEXT_OK
    formatted = host_format(hostlib, tmp_path, text, res)
    assert n_gz == (1 if formatted else 0)
    check_device_bytes(hostlib, inflater, data, formatted, label, readable)
    return data, formatted


def test_fragment_lengths_and_names(engine_mod, hostlib, inflater, tmp_path):
    text, plan = bc.lengths_text()
    data, formatted = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "lengths")
    got = [len(s) for n, s, q in bc.fastq_records(formatted)]
    assert set(bc.FRAG_LENGTHS) - {0} <= set(got) and len(got) >= 60  # (an empty read does not pass)
    names = [r[1] for r in bamio.parse(bc.file_bytes(data))]
    assert b"L1.0" in names and b"L1.1" in names and b"L15.3_" + b"n" * 248 in names  # cut at a space, at a tab, at 254 bytes


def test_every_base_and_quality_value(engine_mod, hostlib, inflater, tmp_path):
    vals = bytes(v for v in range(33, 256))  # (what the device's parser takes in a bases line; the emulator test has the rest)
    q = bytes(v for v in range(33, 127)) * 3
    text = b"".join(b"@v%d\n%s\n+\n%s\n" % (k, s, q[:len(s)]) for k, s in enumerate([vals, b"A" + vals, vals[:77], b"=acgtn" + vals[100:133]]))
    data, formatted = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "values", readable=False)
    recs = bamio.parse(bc.file_bytes(data))
    assert len(recs) == 4 and set(formatted.split(b"\n")[1]) == set(vals)
    assert [list(r[3]) for r in recs] == [[bc.TABLE[b] for b in l] for l in formatted.split(b"\n")[1::4]]
    assert [r[4] for r in recs] == [bytes(c - 33 for c in l) for l in formatted.split(b"\n")[3::4]]


@pytest.mark.parametrize("total", [49151, 49152, 49153])
def test_stripe_edges(engine_mod, hostlib, inflater, tmp_path, total):
    data, formatted = text_case(engine_mod, hostlib, inflater, tmp_path, bc.exact_records_text(total), PLAIN, "edge %d" % total)
    assert len(bgzf.blocks(data)[0]) == -(-total // STRIPE)


def test_every_part_of_a_record_across_a_block_edge(engine_mod, hostlib, inflater, tmp_path):
    text, where = bc.straddle_text()
    text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "straddle")


def test_one_read_of_200_kb(engine_mod, hostlib, inflater, tmp_path):
    data, _ = text_case(engine_mod, hostlib, inflater, tmp_path, one_long_read_text(), PLAIN, "one long read", C=200_000)
    assert len(bgzf.blocks(data)[0]) == 7


def ont_text():
    seq, qual, off = synth.ont_like(700, seed=5, median_len=900, p_middle=0.25)
    return hostio.make_fastq(seq, qual, off)[0]


def test_splits_trims_and_failing_reads(engine_mod, hostlib, inflater, tmp_path):
    data, formatted = text_case(engine_mod, hostlib, inflater, tmp_path, ont_text(), C3, "splits", C=65536)
    assert b"@split-by-adapter-left-" in formatted and b"@split-by-adapter-right-" in formatted


def test_no_read_passes(engine_mod):
    eng = new_engine(engine_mod, dict(required_length=10_000_000), True)
    eng.submit_text(pinned(eng, exact_text(20000)), gzip=True)
    info, res, lines, data = eng.wait_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] > 0 and data == b"" and eng.gzip_batches() == 0
    eng.close()


@pytest.mark.parametrize("case", ["lengths", "splits"])
def test_bam_batches_with_reversed_records(engine_mod, hostlib, inflater, tmp_path, case):
    fq, opts = (bc.lengths_text()[0], PLAIN) if case == "lengths" else (ont_text(), C3)
    recs = []
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(fq)):
        name = name.split(b"\t")[0][:200]  # (a BAM name holds no tab and fits l_read_name)
        recs.append(bamio.reverse_record(name, codes, q) if i % 3 == 1 else (name, 0, codes, q))
    _, st, raw = bamio.bam_bytes(recs, n_cigar=1, tags=b"RGZx\0")
    twin = b"".join(bamio.twin_record(*r) for r in recs)
    off = np.concatenate([[0], np.cumsum([len(r[2]) for r in recs])]).astype(np.uint64)
    eng = new_engine(engine_mod, opts, True, C=65536)
    res = np.zeros(len(recs), abi.RESULT_DTYPE)
    eng.submit_bam(pinned(eng, raw), np.array(st, np.uint64), off, res=res, gzip=True)
    data = eng.wait()
    assert eng.gzip_batches() == 1
    eng.close()
    formatted = host_format(hostlib, tmp_path, twin, res)
    check_device_bytes(hostlib, inflater, data, formatted, "BAM " + case)


def test_records_switch_between_submissions_three_deep(engine_mod, hostlib, inflater, tmp_path):
    texts = [exact_text(60000, seed=31), forced_starts_text(seed=32), short_reads_text(seed=33)[:120000].rsplit(b"\n@", 1)[0] + b"\n"]

    def run(forms):
        eng = new_engine(engine_mod, PLAIN, False)
        bufs = [pinned(eng, t) for t in texts]
        for b, f in zip(bufs, forms):
            eng.set_gzip_records(f)
            eng.submit_text(b, gzip=True)
        assert eng.in_flight() == 3
        eng.set_gzip_records(not forms[-1])  # (a switch with everything in flight reaches none of them)
        outs = [eng.wait_text()[3] for _ in range(3)]
        eng.close()
        return outs

    mixed = run([False, True, False])
    fastq = run([False, False, False])
    bam = run([True, True, True])
    assert mixed[0] == fastq[0] and mixed[2] == fastq[2] and mixed[1] == bam[1]
    assert mixed[0][:4] == b"\x1f\x8b\x08\x00" and mixed[2][:4] == b"\x1f\x8b\x08\x00"  # members: the framing was never touched
    check_device_bytes(hostlib, inflater, mixed[1], texts[1], "switched")
    for k in (0, 2):
        assert inflate_all(mixed[k], len(texts[k])) == texts[k]
        check_device_bytes(hostlib, inflater, bam[k], texts[k], "unswitched %d" % k)


def test_other_values_are_refused(engine_mod):
    eng = new_engine(engine_mod, PLAIN, False)
    for v in (-1, 2, 7):
        assert eng.L.fpl_set_gzip_records(eng.h, v) == abi.FPL_ERR_ARG
    assert eng.L.fpl_set_gzip_records(None, 1) == abi.FPL_ERR_ARG
    eng.close()


def cli(args, env=None):
    p = subprocess.run([build.CLI] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stderr


def inflated(path):
    """the uncompressed bytes of a BAM file the CLI wrote: header block first, EOF block last"""
    import gzip

    data = open(path, "rb").read()
    assert data.endswith(bgzf.EOF)
    first = data[:bgzf.block_len(data, 0)]
    assert gzip.decompress(first) == bc.HEADER_RAW
    return gzip.decompress(data), data


def test_cli_writes_bam_from_fastq_and_from_bam(engine_mod, tmp_path):
    build.build_all()
    case = "c3_full"
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    lines = gz(os.path.join(GOLD, case, "in.fq.gz")).split(b"\n")
    lines[1::4] = [l.upper() for l in lines[1::4]]  # (a BAM holds no lower-case bases)
    bam = bamio.bam_bytes(bamio.fastq_to_records(b"\n".join(lines)))[0]
    text = bamio.bam_to_fastq(bam)  # the FASTQ input is the BAM's twin: what is no code letter in the golden is N in both
    assert len(text) == len(b"\n".join(lines)) - sum(len(l) - 1 for l in lines[2::4])
    (tmp_path / "in.fq").write_bytes(text)
    (tmp_path / "in.bam").write_bytes(bam)
    env = dict(FPLH_CHUNK_BYTES="30000")
    common = ["-j", tmp_path / "o.json", "-h", tmp_path / "o.html", "--reader_threads", "3", "-V"] + list(meta["flags"])
    cli(["-i", tmp_path / "in.fq", "-o", tmp_path / "plain.fq"] + common, env)
    plain = (tmp_path / "plain.fq").read_bytes()
    assert len(plain) > 100_000 and b"@split-by-adapter-" in plain
    want = bc.cut_text(plain)
    raws = {}
    for name, inp, extra in (("fq_dev", "in.fq", ["--device_gzip"]), ("bam_dev", "in.bam", ["--device_gzip"]), ("fq_host", "in.fq", []),
                             ("bam_host", "in.bam", [])):
        err = cli(["-i", tmp_path / inp, "-o", tmp_path / (name + ".bam")] + common + extra, env)
        raws[name], data = inflated(tmp_path / (name + ".bam"))
        n_dev = int(err.split(b"BAM records: BGZF blocks framed on the device: ")[1].split()[0])
        if extra:
            assert b"output: BAM records, packed and deflated on the device" in err and n_dev >= 1
        else:
            assert b"output: BAM records, packed and deflated by the host" in err and n_dev == 0
        assert bamio.bam_to_fastq(data) == want
    assert raws["fq_dev"] == raws["bam_dev"] == raws["fq_host"] == raws["bam_host"]
    # the written file goes back in: trimming and filters off, the output is its twin
    cli(["-i", tmp_path / "fq_dev.bam", "-o", tmp_path / "back.fq", "-j", tmp_path / "b.json", "-h", tmp_path / "b.html", "-A", "-Q", "-L"])
    assert (tmp_path / "back.fq").read_bytes() == want


def test_the_resident_walk_takes_the_written_blocks(engine_mod, hostlib, inflater, tmp_path):
    """header + a batch's blocks + EOF through Engine.submit_bgzf: the same reads as the text they were made from"""
    text = forced_starts_text()
    data, formatted = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "forced starts")
    file = bgzf.bam_header() + data + bgzf.eof()
    eng = new_engine(engine_mod, C3, False)
    eng.submit_text(pinned(eng, text))
    info, ref_res, lines = eng.wait_text()
    eng.close()
    eng = new_engine(engine_mod, C3, False)
    desc, _ = bgzf.blocks(file)
    h, res, names, seq, qual, _ = eng.submit_bgzf(pinned(eng, file), desc, skip=bgzf.header_len(file)).wait()
    eng.close()
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == 40 == info["n_reads"]
    assert [n.lstrip(b"@") for n in names] == [bc.cut_name(l) for l in text.split(b"\n")[0::4][:40]]
    assert res.tobytes() == ref_res.tobytes()
    assert seq.tobytes() == b"".join(text.split(b"\n")[1::4]) and qual.tobytes() == b"".join(text.split(b"\n")[3::4])
