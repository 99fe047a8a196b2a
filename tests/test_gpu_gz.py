"""-m gpu: gzip members deflated on the device (fpl_set_text_gzip / fpl_wait_text_gz, ABI v9; csrc/gz_emit.h) through Engine.
The member of every batch is inflated with zlib, gzip and libdeflate (CRC-32 and ISIZE checked by each) and compared with what
the host's formatter (fplh_format_batch) writes for the same text and the records the same call returned; the coder is
deterministic, so two runs give the same bytes; fpl_get_gzip_batches says the device form ran."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, build, synth
from tests import gz_cases, hostio
from tests.emu_gz import build as emu_gz
from tests.gzcheck import GOLD, gz, host_format, inflate_all, load_hostlib

pytestmark = pytest.mark.gpu

PLAIN = dict(adapter_enabled=0, qual_filter=0, length_filter=0)  # the output is the input
C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)


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


def _pinned(eng, data):
    a = eng.pinned_array(len(data))
    a[:] = np.frombuffer(data, np.uint8)
    return a


def _workload(kind, n, seed):
    """the reads of bench.py's workloads (ONT-like full pipeline, adapter-only, HiFi-like) as FASTQ text"""
    if kind == "c5_hifi64":
        seq, qual, off, ads = synth.hifi_like(n, seed=seed, mean_len=20000, sd_len=2000, n_adapters=64)
        return seq, qual, off, dict(), ads[0], synth.revcomp(ads[0]), list(ads)
    if kind == "c4_mixed":
        seq, qual, off = synth.ont_like(n, seed=seed, median_len=6673, sigma_len=0.9, min_len=200, max_len=200_000)
    else:
        seq, qual, off = synth.ont_like(n, seed=seed, median_len=8000, sigma_len=0.5)
    return seq, qual, off, (dict() if kind == "c2_adapter_only" else C3), synth.START_ADAPTER, synth.END_ADAPTER, []


def _run(engine_mod, text, opts, start, end, fasta, C):
    eng = engine_mod.Engine(abi.FplOptions.default(**opts), start, end, fasta, device=0, max_cycles=C)
    buf = _pinned(eng, text)
    eng.submit_text(buf, gzip=True)
    info, res, lines, member = eng.wait_text()
    n_gz = eng.gzip_batches()
    eng.close()
    assert info["status"] == abi.FPL_TEXT_OK
    return info, res, member, n_gz


@pytest.mark.parametrize("kind", ["c3_full_pipeline", "c2_adapter_only", "c4_mixed", "c5_hifi64"])
def test_member_inflates_to_the_formatter_output(engine_mod, hostlib, tmp_path, kind):
    seq, qual, off, opts, start, end, fasta = _workload(kind, 700, 3)
    text, _, _ = hostio.make_fastq(seq, qual, off, strand_names=True)
    C = int(np.diff(off.astype(np.int64)).max())
    info, res, member, n_gz = _run(engine_mod, text, opts, start, end, fasta, C)
    assert info["n_reads"] == 700 and n_gz == 1
    want = host_format(hostlib, tmp_path, text, res)
    assert len(want) > len(text) // 4
    assert inflate_all(member, len(want)) == want
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    l1 = len(c.compress(want) + c.flush())
    print("%s: text out %d, member %d, raw level 1 %d (%.3f x)" % (kind, len(want), len(member), l1, len(member) / l1))
    assert len(member) <= 1.05 * l1
    # deterministic
    info2, res2, member2, _ = _run(engine_mod, text, opts, start, end, fasta, C)
    assert member2 == member and res2.tobytes() == res.tobytes()


def test_one_batch_of_150000_reads(engine_mod, hostlib, tmp_path):
    seq, qual, off = synth.ont_like(150_000, seed=5, median_len=500, sigma_len=0.6)
    text, _, _ = hostio.make_fastq(seq, qual, off)
    C = int(np.diff(off.astype(np.int64)).max())
    info, res, member, n_gz = _run(engine_mod, text, C3, synth.START_ADAPTER, synth.END_ADAPTER, [], C)
    assert info["n_reads"] == 150_000 and n_gz == 1
    want = host_format(hostlib, tmp_path, text, res)
    assert inflate_all(member, len(want)) == want


def test_batches_in_flight_switch_per_batch_and_empty_output(engine_mod, hostlib, tmp_path):
    """three batches in the three slots: gzip, plain, gzip; then a batch in which no read passes"""
    opts = dict(C3)
    eng = engine_mod.Engine(abi.FplOptions.default(**opts), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=20000)
    texts = []
    for k in range(3):
        seq, qual, off = synth.ont_like(300 + 50 * k, seed=20 + k, median_len=2000, p_middle=0.2, max_len=20000)
        texts.append(hostio.make_fastq(seq, qual, off, crlf=(k == 2))[0])
    bufs = [_pinned(eng, t) for t in texts]
    eng.submit_text(bufs[0], gzip=True)
    eng.submit_text(bufs[1])
    eng.submit_text(bufs[2], gzip=True)
    outs = [eng.wait_text() for _ in range(3)]
    assert len(outs[0]) == 4 and len(outs[1]) == 3 and len(outs[2]) == 4
    assert eng.gzip_batches() == 2
    for k in (0, 2):
        want = host_format(hostlib, tmp_path, texts[k], outs[k][1])
        assert b"split-by-adapter-" in want and b"\r" not in want
        assert inflate_all(outs[k][3], len(want)) == want
    eng.close()
    # nothing passes: a required length no read has
    eng = engine_mod.Engine(abi.FplOptions.default(required_length=10_000_000), synth.START_ADAPTER, synth.END_ADAPTER, device=0,
                            max_cycles=20000)
    eng.submit_text(_pinned(eng, texts[0]), gzip=True)
    info, res, lines, member = eng.wait_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] == 300 and member == b"" and eng.gzip_batches() == 0
    eng.close()


def _plain_members(engine_mod, texts, C=20480):
    """the members of `texts`, one submission each on ONE engine that changes nothing -> [(records, member)]"""
    eng = engine_mod.Engine(abi.FplOptions.default(**PLAIN), "", "", device=0, max_cycles=C)
    out = []
    for text in texts:
        eng.submit_text(_pinned(eng, text), gzip=True)
        info, res, lines, member = eng.wait_text()
        assert info["status"] == abi.FPL_TEXT_OK
        out.append((res, member))
    assert eng.gzip_batches() == len(texts)
    eng.close()
    return out


def test_battery_in_name_lines(engine_mod, hostlib, tmp_path):
    """the inputs that reach the coder's limits (tests/gz_cases.py: 15-bit and 7-bit limits, the stored form, two- and three-symbol
    blocks, 250+ symbols, bytes from 0x80 up) through k_gz_block: every block meets gz_cases.check_block, and the member is, byte for
    byte, the emulator's -- the coder is deterministic, and a difference says which block the device got wrong"""
    text, where = gz_cases.as_fastq(gz_cases.block_battery())
    (res, member), = _plain_members(engine_mod, [text])
    want = host_format(hostlib, tmp_path, text, res)
    assert want == text and inflate_all(member, len(want)) == want
    blocks = gz_cases.member_blocks(member, want)
    for name, m in gz_cases.check_battery(blocks, where, 1).items():
        print(gz_cases.excess_line(name, m))
    emu, _ = emu_gz.emit(text, res)
    emu_blocks = gz_cases.member_blocks(emu, want)
    assert [b["raw"] == e["raw"] for b, e in zip(blocks, emu_blocks)] == [True] * len(emu_blocks), [b["start"] for b in blocks]
    assert member == emu


def test_tail_lengths(engine_mod, hostlib, tmp_path):
    """a last block of every length at the edges of a thread's stretch of 64 symbols and of the 16-byte loads and stores"""
    texts = [gz_cases.tail_text(r) for r in gz_cases.TAIL_LENGTHS]
    for r, text, (res, member) in zip(gz_cases.TAIL_LENGTHS, texts, _plain_members(engine_mod, texts)):
        assert len(res) == text.count(b"\n") // 4 and (res["code"][:, 0] == abi.FPL_PASS_FILTER).all() and (res["n_frag"] == 1).all()
        assert inflate_all(member, len(text)) == text, r
        blocks = gz_cases.member_blocks(member, text)
        assert len(blocks) == 4 and blocks[-1]["n"] == r
        for b in blocks:
            gz_cases.check_block(b, 1)
        assert member == emu_gz.emit(text, res)[0], r


GOLDEN_TEXT = ["c1_qualfilter", "c3_full", "c5_fasta"]  # (--break / --mask output keeps the host's deflate: never a text batch)


@pytest.mark.parametrize("chunk", ["30000", None])  # many batches / one chunk size that holds the whole input
@pytest.mark.parametrize("case", GOLDEN_TEXT)
def test_cli_on_the_device_writes_gz_members(engine_mod, tmp_path, case, chunk):
    """bin/fastplong_amd -o out.fq.gz on the device: zlib, libdeflate and the project's own multi-member reader (a second pass
    with -i out.fq.gz) give the bytes of the plain --out run"""
    build.build_all()
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    inp = tmp_path / "in.fq"
    inp.write_bytes(gz(os.path.join(GOLD, case, "in.fq.gz")))
    flags = [f if f != "ADAPTERS.fa" else os.path.join(GOLD, case, "ADAPTERS.fa") for f in meta["flags"]]
    env = dict(os.environ)
    if chunk:
        env["FPLH_CHUNK_BYTES"] = chunk

    def cli(src, out, extra=()):
        cmd = [build.CLI, "-i", str(src), "-o", str(out), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html"), "--reader_threads", "3",
               "-V"] + flags + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stderr

    err = cli(inp, tmp_path / "out.fq.gz")
    want = gz(os.path.join(GOLD, case, "expected.out.fq.gz"))
    data = (tmp_path / "out.fq.gz").read_bytes()
    if chunk:
        assert b"output: gzip members deflated on the device" in err
        n = int(err.split(b"device gzip: ")[1].split()[0])
        assert n >= 3 and data.count(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff") == n  # every member is the device's
    d = zlib.decompressobj(31)
    got = b""
    rest = data
    while rest:  # member after member
        d = zlib.decompressobj(31)
        got += d.decompress(rest) + d.flush()
        assert d.eof
        rest = d.unused_data
    assert got == want
    cli(inp, tmp_path / "host.fq.gz", ["--host_gzip"])
    assert gz(tmp_path / "host.fq.gz") == want
    # the project's own reader takes the file back
    cli(tmp_path / "out.fq.gz", tmp_path / "second_z.fq", ["--host_parse"])
    (tmp_path / "twin.fq").write_bytes(want)
    cli(tmp_path / "twin.fq", tmp_path / "second_p.fq", ["--host_parse"])
    assert (tmp_path / "second_z.fq").read_bytes() == (tmp_path / "second_p.fq").read_bytes()
