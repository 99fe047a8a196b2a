"""-m gpu: the gzip batches' bytes as BGZF blocks (fpl_set_gzip_framing; csrc/gz_emit.h: k_gz_block_bgzf, k_gz_finish_bgzf,
k_gz_frame) through Engine and the CLI on the real library.

Every output is cut into blocks (fastplong_amd.bgzf.blocks must cover it), every block but the last holds 49 152 bytes of text and
is at most 65 536 bytes long, gzip.decompress takes each block alone (CRC-32 and ISIZE), the blocks join to what the host's
formatter writes for the same text and records -- and the device's own inflater (Inflater.inflate) returns status 0 for every
block, with the same bytes.  '+' is the third line everywhere: the resident walk refuses third lines that repeat the name.

Size cap: len(bgzf) <= len(member) - 23 + 31 * n_bgzf + 8 * n_blocks (derived in tests/test_bgzf_out_emu.py); the deflate blocks
are counted from the layout's rule in Python, never read back from the code under test."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bamio, gz_cases, hostio
from tests.bgzf_out_cases import (EDGE_TOTALS, STRIPE, check_blocks, exact_text, forced_starts_text, one_long_read_text,
                                  short_reads_text)
from tests.emu_bgzfout import build as emu_bgzfout
from tests.emu_gz import build as emu_gz
from tests.gzcheck import GOLD, gz, host_format, inflate_all, load_hostlib

pytestmark = pytest.mark.gpu

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
PLAIN = dict(adapter_enabled=0, qual_filter=0, length_filter=0)  # the output is the input
GZ_B, GZ_L = 16384, 1024


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


@pytest.fixture(scope="module")
def inflater(engine_mod):
    inf = engine_mod.Inflater(0)
    yield inf
    inf.close()


def pinned(eng, data):
    a = eng.pinned_array(max(len(data), 1))
    a[:len(data)] = np.frombuffer(data, np.uint8)
    return a[:len(data)]


def new_engine(engine_mod, opts, bgzf_on, C=20480):
    adapters = ("", "") if opts is PLAIN else (synth.START_ADAPTER, synth.END_ADAPTER)
    eng = engine_mod.Engine(abi.FplOptions.default(**opts), adapters[0], adapters[1], device=0, max_cycles=C)
    if bgzf_on:
        eng.set_gzip_framing(True)
    return eng


def run_text(engine_mod, text, opts, bgzf_on, C=20480):
    eng = new_engine(engine_mod, opts, bgzf_on, C)
    eng.submit_text(pinned(eng, text), gzip=True)
    info, res, lines, data = eng.wait_text()
    n_gz = eng.gzip_batches()
    eng.close()
    assert info["status"] == abi.FPL_TEXT_OK
    return res, data, n_gz


def deflate_blocks(want):
    """how many deflate blocks k_gz_layout cuts the formatted text into: every multiple of GZ_B, and the name line and the '+' line
    of a record whose bases line has at least GZ_L bytes"""
    starts, o = set(range(0, len(want), GZ_B)), 0
    lines = want.split(b"\n")
    for i in range(0, len(lines) - 1, 4):
        a = len(lines[i]) + len(lines[i + 1]) + 2
        if len(lines[i + 1]) + 1 >= GZ_L:
            starts.update((o, o + a))
        o += a + len(lines[i + 2]) + len(lines[i + 3]) + 2
    return len(starts)


def check_device_blocks(inflater, data, member, want, label):
    """the checks of the module's docstring -> the blocks"""
    assert inflate_all(member, len(want)) == want
    blocks = check_blocks(data, want, piece=STRIPE)
    desc, _ = bgzf.blocks(data)
    out, status = inflater.inflate(np.frombuffer(data, np.uint8), desc)
    assert len(status) == len(blocks) and (status == 0).all(), status
    assert out.tobytes() == want
    nb, n_bgzf = deflate_blocks(want), len(blocks)
    grow = len(data) - (len(member) - 23)
    print("%s: text %d, member %d, BGZF %d in %d blocks of %d deflate blocks: +%d bytes = %d frames + %.2f per deflate block" % (
        label, len(want), len(member), len(data), n_bgzf, nb, grow, 31 * n_bgzf, (grow - 31 * n_bgzf) / nb))
    assert len(data) <= len(member) - 23 + 31 * n_bgzf + 8 * nb
    return blocks


def text_case(engine_mod, hostlib, inflater, tmp_path, text, opts, label, C=20480):
    res, data, n_gz = run_text(engine_mod, text, opts, True, C)
    res_m, member, _ = run_text(engine_mod, text, opts, False, C)
    assert res.tobytes() == res_m.tobytes() and n_gz == 1
    want = host_format(hostlib, tmp_path, text, res)
    check_device_blocks(inflater, data, member, want, label)
    return data, want


@pytest.mark.parametrize("total", EDGE_TOTALS)
def test_stripe_edges(engine_mod, hostlib, inflater, tmp_path, total):
    text = exact_text(total)
    data, want = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "edge %d" % total)
    assert want == text and len(bgzf.blocks(data)[0]) == -(-total // STRIPE)


def test_forced_starts_fill_a_stripe_and_the_file_goes_back_in(engine_mod, hostlib, inflater, tmp_path):
    text = forced_starts_text()
    data, want = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "forced starts")
    assert want == text and deflate_blocks(want) >= 80 and len(want) < 2 * STRIPE
    # the blocks through the resident BGZF text path on a second context, against submit_text of the inflated text
    eng = new_engine(engine_mod, C3, False)
    eng.submit_text(pinned(eng, want))
    info, ref_res, lines = eng.wait_text()
    eng.close()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] == 40
    eng = new_engine(engine_mod, C3, False)
    desc, _ = bgzf.blocks(data)
    h, res, names, seq, qual, _ = eng.submit_bgzf_text(pinned(eng, data), desc).wait()
    eng.close()
    assert h["status"] == abi.FPL_TXTW_OK and h["n_reads"] == 40
    assert names == want.split(b"\n")[0::4][:40]
    assert res.tobytes() == ref_res.tobytes()


def test_short_reads_merged_blocks(engine_mod, hostlib, inflater, tmp_path):
    text_case(engine_mod, hostlib, inflater, tmp_path, short_reads_text(), PLAIN, "short reads")


def test_one_read_over_nine_stripes(engine_mod, hostlib, inflater, tmp_path):
    data, want = text_case(engine_mod, hostlib, inflater, tmp_path, one_long_read_text(), PLAIN, "one long read", C=200_000)
    assert len(bgzf.blocks(data)[0]) == 9


def test_battery_in_name_lines(engine_mod, hostlib, inflater, tmp_path):
    """the inputs that reach the coder's limits (tests/gz_cases.py) through k_gz_block_bgzf and k_gz_block: every deflate block
    meets gz_cases.check_block, the device's inflater takes the BGZF blocks back (15-bit codes go down its bit-serial walk), and
    both outputs are, byte for byte, the emulator's for the same text and records"""
    text, where = gz_cases.as_fastq(gz_cases.block_battery())
    res, data, _ = run_text(engine_mod, text, PLAIN, True)
    res_m, member, _ = run_text(engine_mod, text, PLAIN, False)
    want = host_format(hostlib, tmp_path, text, res)
    assert want == text and res.tobytes() == res_m.tobytes()
    check_device_blocks(inflater, data, member, want, "battery")
    blocks = gz_cases.bgzf_blocks(data, want)
    for name, m in gz_cases.check_battery(blocks, where, 2).items():
        print(gz_cases.excess_line(name, m))
    gz_cases.check_battery(gz_cases.member_blocks(member, want), where, 1)
    emu, _ = emu_bgzfout.emit(text, res, True)
    emu_blocks = gz_cases.bgzf_blocks(emu, want)
    assert [b["raw"] == e["raw"] for b, e in zip(blocks, emu_blocks)] == [True] * len(emu_blocks), [b["start"] for b in blocks]
    assert data == emu
    assert member == emu_gz.emit(text, res)[0]


def test_tail_lengths(engine_mod, hostlib, inflater, tmp_path):
    """a last deflate block of every length at the edges of a thread's stretch and of the 16-byte loads and stores, in a BGZF
    block of its own (the text is one stripe and the tail)"""
    eng = new_engine(engine_mod, PLAIN, True)
    for r in gz_cases.TAIL_LENGTHS:
        text = gz_cases.tail_text(r)
        eng.submit_text(pinned(eng, text), gzip=True)
        info, res, lines, data = eng.wait_text()
        assert info["status"] == abi.FPL_TEXT_OK and (res["code"][:, 0] == abi.FPL_PASS_FILTER).all() and (res["n_frag"] == 1).all()
        frames = check_blocks(data, text, piece=STRIPE)
        assert len(frames) == 2
        blocks = gz_cases.bgzf_blocks(data, text)
        assert len(blocks) == 4 and blocks[-1]["n"] == r
        for b in blocks:
            gz_cases.check_block(b, 2)
        desc, _ = bgzf.blocks(data)
        out, status = inflater.inflate(np.frombuffer(data, np.uint8), desc)
        assert (status == 0).all() and out.tobytes() == text, r
    eng.close()


@pytest.mark.parametrize("n_reads, per", [(530, 2), (4300, 9)])
def test_more_than_1024_deflate_blocks(engine_mod, hostlib, inflater, tmp_path, n_reads, per):
    """k_gz_finish_bgzf's threads take runs of `per` consecutive deflate blocks that cross stripes, and both finishes' prefix sums
    go round more than once (tests/test_bgzf_out_emu.py has the list of what only runs then)"""
    text = gz_cases.many_blocks_text(n_reads)
    nb = deflate_blocks(text)
    assert gz_cases.per_thread_runs(nb) == per and nb > 1024 * (per - 1) and nb % per != 0
    data, want = text_case(engine_mod, hostlib, inflater, tmp_path, text, PLAIN, "%d reads" % n_reads)
    assert want == text and len(bgzf.blocks(data)[0]) == -(-len(text) // STRIPE) >= 23


def ont_text():
    seq, qual, off = synth.ont_like(700, seed=5, median_len=900, p_middle=0.25)
    return hostio.make_fastq(seq, qual, off)[0]


def test_splits_with_both_prefixes(engine_mod, hostlib, inflater, tmp_path):
    data, want = text_case(engine_mod, hostlib, inflater, tmp_path, ont_text(), C3, "splits", C=65536)
    assert b"@split-by-adapter-left-" in want and b"@split-by-adapter-right-" in want


def test_no_read_passes(engine_mod):
    eng = new_engine(engine_mod, dict(required_length=10_000_000), True)
    eng.submit_text(pinned(eng, exact_text(20000)), gzip=True)
    info, res, lines, data = eng.wait_text()
    assert info["status"] == abi.FPL_TEXT_OK and info["n_reads"] > 0 and data == b"" and eng.gzip_batches() == 0
    eng.close()


@pytest.mark.parametrize("case", ["forced", "splits"])
def test_bam_batches(engine_mod, hostlib, inflater, tmp_path, case):
    fq, opts = (forced_starts_text(), PLAIN) if case == "forced" else (ont_text(), C3)
    recs = []
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(fq)):
        recs.append(bamio.reverse_record(name, codes, q) if i % 3 == 1 else (name, 0, codes, q))
    _, st, raw = bamio.bam_bytes(recs, n_cigar=1, tags=b"RGZx\0")
    twin = b"".join(bamio.twin_record(*r) for r in recs)
    off = np.concatenate([[0], np.cumsum([len(r[2]) for r in recs])]).astype(np.uint64)
    outs = []
    for on in (True, False):
        eng = new_engine(engine_mod, opts, on, C=65536)
        res = np.zeros(len(recs), abi.RESULT_DTYPE)
        eng.submit_bam(pinned(eng, raw), np.array(st, np.uint64), off, res=res, gzip=True)
        outs.append((eng.wait(), res))
        assert eng.gzip_batches() == 1
        eng.close()
    (data, res), (member, res_m) = outs
    assert res.tobytes() == res_m.tobytes()
    want = host_format(hostlib, tmp_path, twin, res)
    assert len(want) > STRIPE
    check_device_blocks(inflater, data, member, want, "BAM " + case)


def test_framing_switches_between_submissions_three_deep(engine_mod, hostlib, inflater, tmp_path):
    texts = [exact_text(60000, seed=31), forced_starts_text(seed=32), short_reads_text(seed=33)[:120000].rsplit(b"\n@", 1)[0] + b"\n"]

    def run(framings):
        eng = new_engine(engine_mod, PLAIN, False)
        bufs = [pinned(eng, t) for t in texts]
        for b, f in zip(bufs, framings):
            eng.set_gzip_framing(f)
            eng.submit_text(b, gzip=True)
        assert eng.in_flight() == 3
        eng.set_gzip_framing(not framings[-1])  # (a switch with everything in flight reaches none of them)
        outs = [eng.wait_text()[3] for _ in range(3)]
        eng.close()
        return outs

    mixed = run([False, True, False])
    members = run([False, False, False])
    blocks = run([True, True, True])
    assert mixed[0] == members[0] and mixed[2] == members[2] and mixed[1] == blocks[1]
    assert mixed == run([False, True, False])
    assert mixed[0][:4] == b"\x1f\x8b\x08\x00" and mixed[2][:4] == b"\x1f\x8b\x08\x00"
    check_device_blocks(inflater, mixed[1], members[1], texts[1], "switched")
    for k in (0, 2):
        assert inflate_all(mixed[k], len(texts[k])) == texts[k]


def test_other_framing_values_are_refused(engine_mod):
    eng = new_engine(engine_mod, PLAIN, False)
    for v in (-1, 2, 7):
        assert eng.L.fpl_set_gzip_framing(eng.h, v) == abi.FPL_ERR_ARG
    eng.close()


def test_cli_writes_bgzf_on_the_device_and_on_the_host(engine_mod, inflater, tmp_path):
    build.build_all()
    case = "c3_full"
    meta = json.load(open(os.path.join(GOLD, case, "case.json")))
    inp = tmp_path / "in.fq"
    inp.write_bytes(gz(os.path.join(GOLD, case, "in.fq.gz")))
    env = dict(os.environ, FPLH_CHUNK_BYTES="30000")

    def cli(out, extra=()):
        cmd = [build.CLI, "-i", str(inp), "-o", str(out), "-j", str(tmp_path / "o.json"), "-h", str(tmp_path / "o.html"), "--reader_threads", "3",
               "-V"] + list(meta["flags"]) + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return p.stderr

    cli(tmp_path / "member.fq.gz")
    want = gz(tmp_path / "member.fq.gz")
    assert want == gz(os.path.join(GOLD, case, "expected.out.fq.gz"))
    assert not (tmp_path / "member.fq.gz").read_bytes()[3] & 4  # without the flag: no FEXTRA, the members of before
    err = cli(tmp_path / "out.fq.gz", ["--bgzf"])
    data = (tmp_path / "out.fq.gz").read_bytes()
    assert b"output: BGZF blocks" in err
    n_dev = int(err.split(b"BGZF blocks framed on the device: ")[1].split()[0])
    blocks = check_blocks(data, want, eof=True)
    assert 3 <= n_dev <= len(blocks)
    desc, _ = bgzf.blocks(data)
    out, status = inflater.inflate(np.frombuffer(data, np.uint8), desc)
    assert (status == 0).all() and out.tobytes() == want
    err = cli(tmp_path / "host.fq.gz", ["--host_gzip", "--bgzf"])
    assert b"BGZF blocks framed on the device: 0 " in err
    check_blocks((tmp_path / "host.fq.gz").read_bytes(), want, eof=True)
