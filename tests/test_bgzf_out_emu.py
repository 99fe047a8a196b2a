"""The BGZF form of the gzip kernels (fpl_set_gzip_framing; fastplong_amd/csrc/gz_emit.h: k_gz_block_bgzf, k_gz_finish_bgzf,
k_gz_frame) on the CPU emulator, as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/emu_bgzfout).  The output must be BGZF blocks of 49 152 text bytes each that gzip takes block by block, that join to what
the host's formatter writes -- and that the device's OWN inflater (k_bgzf_inflate on the emulator, tests/emu_bgzf) takes, every
block with status 0: the member form's single distance code is what it refuses.  The member form out of the same driver is, byte
for byte, tests/emu_gz's.

Size cap: len(bgzf) <= len(member) - 23 + 31 * n_bgzf + 8 * n_blocks.  Inside a deflate block the only difference is one more
code length in its header: the symbol twice at no more than 7 bits, up to four more 3-bit HCLEN entries, a reshaped code-length
code -- about 5 bytes, 8 allowed."""
import os
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, synth
from tests import gz_cases, hostio
from tests.bgzf_out_cases import (EDGE_TOTALS, STRIPE, check_blocks, exact_text, forced_starts_text, lengths, one_long_read_text,
                                  short_reads_text)
from tests.emu_bgzf import build as emu_inflate
from tests.emu_bgzfout import build as emu_out
from tests.emu_gz import build as emu_gz
from tests.gzcheck import GOLD, GOLDEN_OPTS, fasta_list, gz, host_format, load_hostlib, parse_fastq
from tests.test_gz_emit_emu import whole

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def check(hostlib, tmp_path, text, res, label):
    want = host_format(hostlib, tmp_path, text, res)
    jobs = [emu_out.start(text, res, True), emu_out.start(text, res, False)]  # (side by side: two processes)
    data, info = emu_out.finish(jobs[0])
    member, minfo = emu_out.finish(jobs[1])
    ref_member, ref_info = emu_gz.emit(text, res)
    assert member == ref_member and minfo["n_blocks"] == ref_info["n_blocks"] == info["n_blocks"]
    assert info["total"] == len(want) and minfo["crc"] == ref_info["crc"]
    if not want:
        assert data == b"" and member == b""
        return data, info
    assert info["crc"] == zlib.crc32(want)  # GzHeader.crc keeps its meaning: the whole composed text
    n_bgzf = -(-len(want) // STRIPE)
    assert len(data) == info["gz_len"] <= info["out_cap"] == len(want) + 5 * info["n_blocks"] + 31 * n_bgzf
    blocks = check_blocks(data, want, piece=STRIPE)
    assert len(blocks) == n_bgzf
    # the device's inflater, on the emulator under the sanitizers: every block, status 0, the same bytes
    desc, _ = bgzf.blocks(data)
    out, got = emu_inflate.inflate(np.frombuffer(data, np.uint8), desc, np.zeros(len(want), np.uint8))
    assert len(got) == n_bgzf and (got["status"] == 0).all(), got["status"]
    assert out.tobytes() == want
    grow = len(data) - (len(member) - 23)
    print("%s: text %d, member %d, BGZF %d in %d blocks of %d deflate blocks: +%d bytes = %d frames + %.2f per deflate block" % (
        label, len(want), len(member), len(data), n_bgzf, info["n_blocks"], grow, 31 * n_bgzf, (grow - 31 * n_bgzf) / info["n_blocks"]))
    assert len(data) <= len(member) - 23 + 31 * n_bgzf + 8 * info["n_blocks"]
    return data, info


@pytest.mark.parametrize("total", EDGE_TOTALS)
def test_stripe_edges(hostlib, tmp_path, total):
    text = exact_text(total)
    data, info = check(hostlib, tmp_path, text, whole(lengths(text)), "edge %d" % total)
    assert len(bgzf.blocks(data)[0]) == -(-total // STRIPE)


def test_forced_starts_fill_one_stripe(hostlib, tmp_path):
    text = forced_starts_text()
    data, info = check(hostlib, tmp_path, text, whole(lengths(text)), "forced starts")
    assert info["n_blocks"] >= 80 and len(text) < 2 * STRIPE  # two stripes of 40+ deflate blocks each


def test_short_reads_merged_blocks(hostlib, tmp_path):
    text = short_reads_text()
    check(hostlib, tmp_path, text, whole(lengths(text)), "short reads")


def test_one_read_over_nine_stripes(hostlib, tmp_path):
    text = one_long_read_text()
    data, info = check(hostlib, tmp_path, text, whole(lengths(text)), "one long read")
    assert len(bgzf.blocks(data)[0]) == 9


def test_splits_with_both_prefixes(orc, hostlib, tmp_path):
    seq, qual, off = synth.ont_like(700, seed=5, median_len=900, p_middle=0.25)
    text, _, _ = hostio.make_fastq(seq, qual, off)
    cfg = orc.Config(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER)
    res, _ = orc.process_batch(cfg, seq, qual, off)
    want = host_format(hostlib, tmp_path, text, res)
    assert b"split-by-adapter-left-" in want and b"split-by-adapter-right-" in want
    check(hostlib, tmp_path, text, res, "splits")


def test_no_read_passes(hostlib, tmp_path):
    text = exact_text(20000)
    data, info = check(hostlib, tmp_path, text, whole(lengths(text), code=abi.FPL_FAIL_LENGTH), "nothing passes")
    assert data == b""


@pytest.mark.parametrize("case", sorted(GOLDEN_OPTS))
def test_golden_through_the_oracle(orc, hostlib, tmp_path, case):
    okw, start, end = GOLDEN_OPTS[case]
    text = gz(os.path.join(GOLD, case, "in.fq.gz"))
    seq, qual, off, names, strands = parse_fastq(text)
    cfg = orc.Config(abi.FplOptions.default(**okw), start, end, fasta_list(case))
    res, _ = orc.process_batch(cfg, seq, qual, off)
    data, info = check(hostlib, tmp_path, text, res, case)
    assert b"".join(bgzf.inflate_block(data, o) for o in bgzf.blocks(data)[1]) == gz(os.path.join(GOLD, case, "expected.out.fq.gz"))


@pytest.mark.parametrize("n_reads, per", [(530, 2), (1400, 3), (4300, 9)])
def test_more_than_1024_deflate_blocks(hostlib, tmp_path, n_reads, per):
    """k_gz_finish_bgzf gives each of its 1 024 threads a run of `per` consecutive blocks: runs that cross stripes, more than one
    trip of the eight-loads loop, a clamped last run, threads with no run, and further trips of both finishes' prefix sums"""
    text = gz_cases.many_blocks_text(n_reads)
    data, info = check(hostlib, tmp_path, text, whole(lengths(text)), "%d reads" % n_reads)
    nb = info["n_blocks"]
    assert nb == len(gz_cases.block_starts(text)) >= 2 * n_reads
    assert gz_cases.per_thread_runs(nb) == per and nb > 1024 * (per - 1) and nb % per != 0
    assert len(bgzf.blocks(data)[0]) == -(-len(text) // STRIPE) >= 23  # (49 deflate blocks a stripe: runs cross stripes all along)


def test_battery_in_name_lines(hostlib, tmp_path):
    """the inputs that reach the coder's limits (tests/gz_cases.py) with two distance lengths in every header; check() hands the
    blocks to the device's inflater too, whose bit-serial walk takes the 15-bit codes"""
    text, where = gz_cases.as_fastq(gz_cases.block_battery())
    data, info = check(hostlib, tmp_path, text, whole(lengths(text)), "battery")
    blocks = gz_cases.bgzf_blocks(data, text)
    assert len(blocks) == info["n_blocks"]
    for name, m in gz_cases.check_battery(blocks, where, 2).items():
        print(gz_cases.excess_line(name, m))
