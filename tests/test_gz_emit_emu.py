"""The gzip kernels (fastplong_amd/csrc/gz_emit.h) on the CPU emulator: the emitted members are inflated with Python's zlib / gzip
and, when the machine has it, with libdeflate through ctypes (both check CRC-32 and ISIZE), and compared with what the host's
formatter (fplh_format_batch) writes for the same batch and records.

Size: the members are at most 1.05 x raw zlib level 1 of the same text on the golden outputs, and smaller than level 1 on reads
of 5 kb and more (one table per line kind beats level 1's mixed tables; see docs/kernels.md)."""
import ctypes as C
import ctypes.util
import gzip
import os
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, build, synth
from tests import gz_cases, hostio
from tests.bgzf_out_cases import exact_text, lengths
from tests.emu_gz import build as emu_gz
from tests.gzcheck import GOLD, GOLDEN_OPTS, fasta_list, gz, host_format, inflate_all, load_hostlib, parse_fastq

RES = np.dtype(abi.RESULT_DTYPE)


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


def whole(lengths, code=abi.FPL_PASS_FILTER):
    """records that pass every read whole"""
    res = np.zeros(len(lengths), RES)
    res["n_frag"] = 1
    res["frag_len"][:, 0] = lengths
    res["r1_len"] = lengths
    res["code"][:, 0] = code
    return res


def check(hostlib, tmp_path, text, res):
    want = host_format(hostlib, tmp_path, text, res)
    data, info, comp = emu_gz.emit(text, res, want_composed=True)
    assert comp == want  # k_gz_layout + k_gz_compose
    assert info["total"] == len(want)
    if not want:
        assert data == b"" and info["n_blocks"] == 0
        return data, info, want
    assert len(data) == info["gz_len"] <= emu_gz.bound(info["total"], info["n_blocks"])  # the bound the buffers are sized by
    assert inflate_all(data, len(want)) == want
    assert info["crc"] == zlib.crc32(want)
    assert data[:4] == b"\x1f\x8b\x08\x00" and data[-8:] == (zlib.crc32(want)).to_bytes(4, "little") + (len(want) % 2 ** 32).to_bytes(4, "little")
    return data, info, want


def level(text, lv):
    c = zlib.compressobj(lv, zlib.DEFLATED, -15)
    return len(c.compress(text) + c.flush())


def fastq(reads):
    """[(name, bases, strand, qualities)] -> text"""
    return b"".join(b"%s\n%s\n%s\n%s\n" % r for r in reads)


def rand_read(rng, n, name, strand=b"+"):
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    q = np.clip(rng.normal(22, 7, n), 1, 60).astype(np.uint8) + 33
    return (name, s, strand, q.tobytes())


@pytest.mark.parametrize("case", sorted(GOLDEN_OPTS))
def test_golden_members_and_size(orc, hostlib, tmp_path, case):
    okw, start, end = GOLDEN_OPTS[case]
    text = gz(os.path.join(GOLD, case, "in.fq.gz"))
    seq, qual, off, names, strands = parse_fastq(text)
    cfg = orc.Config(abi.FplOptions.default(**okw), start, end, fasta_list(case))
    res, _ = orc.process_batch(cfg, seq, qual, off)
    data, info, want = check(hostlib, tmp_path, text, res)
    assert want == gz(os.path.join(GOLD, case, "expected.out.fq.gz"))
    l1 = level(want, 1)
    print("%s: text %d, device form %d, raw level 1 %d (%.3f x), level 4 %d, blocks %d" % (
        case, len(want), len(data), l1, len(data) / l1, level(want, 4), info["n_blocks"]))
    assert len(data) <= 1.05 * l1


def test_long_reads_are_smaller_than_level_1(hostlib, tmp_path):
    rng = np.random.default_rng(3)
    text = fastq([rand_read(rng, int(n), b"@r%d runid=0a1b ch=%d" % (i, i)) for i, n in enumerate(rng.integers(5000, 30000, 24))])
    res = whole([len(l) for l in text.split(b"\n")[1::4]])
    data, info, want = check(hostlib, tmp_path, text, res)
    l1 = level(want, 1)
    print("long reads: text %d, device form %d, raw level 1 %d (%.3f x), level 4 %d" % (len(want), len(data), l1, len(data) / l1, level(want, 4)))
    assert len(data) < l1


@pytest.mark.parametrize("seed", [1, 2])
def test_synthetic_batches_through_the_oracle(orc, hostlib, tmp_path, seed):
    """adapters, trims and middle-adapter splits (both prefixes) as the oracle finds them"""
    seq, qual, off = synth.ont_like(160, seed=seed, median_len=900, p_middle=0.25)
    text, _, _ = hostio.make_fastq(seq, qual, off, strand_names=True)
    cfg = orc.Config(abi.FplOptions.default(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1,
                                            complexity_filter=1), synth.START_ADAPTER, synth.END_ADAPTER)
    res, _ = orc.process_batch(cfg, seq, qual, off)
    data, info, want = check(hostlib, tmp_path, text, res)
    assert b"split-by-adapter-left-" in want and b"split-by-adapter-right-" in want


def test_no_read_passes_one_read_and_all_dropped_but_one(hostlib, tmp_path):
    rng = np.random.default_rng(4)
    reads = [rand_read(rng, 700 + i, b"@n%d" % i) for i in range(9)]
    text = fastq(reads)
    lens = [700 + i for i in range(9)]
    res = whole(lens, code=abi.FPL_FAIL_LENGTH)
    data, info, want = check(hostlib, tmp_path, text, res)
    assert data == b"" and want == b""
    res = whole(lens)
    res["dropped"] = 1
    res["dropped"][5] = 0
    data, info, want = check(hostlib, tmp_path, text, res)
    assert want == fastq(reads[5:6])
    check(hostlib, tmp_path, fastq(reads[:1]), whole(lens[:1]))
    check(hostlib, tmp_path, b"", whole([]))


def test_split_read_both_prefixes_and_windows(hostlib, tmp_path):
    rng = np.random.default_rng(6)
    reads = [rand_read(rng, 5000, b"@a"), rand_read(rng, 9000, b"@split me", b"+split me"), rand_read(rng, 40, b"@z")]
    res = whole([5000, 9000, 40])
    res[1]["n_frag"] = 2
    res[1]["frag_start"][:] = [17, 4100]
    res[1]["frag_len"][:] = [3000, 4883]
    res[1]["kind"][:] = [1, 2]
    res[0]["frag_start"][0], res[0]["frag_len"][0] = 33, 4000
    data, info, want = check(hostlib, tmp_path, fastq(reads), res)
    assert want.count(b"@split-by-adapter-left-split me\n") == 1 and want.count(b"@split-by-adapter-right-split me\n") == 1
    res[1]["code"][0] = abi.FPL_FAIL_LENGTH  # only the right fragment is written
    data, info, want = check(hostlib, tmp_path, fastq(reads), res)
    assert b"left" not in want and b"right" in want


def test_a_read_of_1_2_megabases(hostlib, tmp_path):
    rng = np.random.default_rng(7)
    reads = [rand_read(rng, 300, b"@s"), rand_read(rng, 1_200_000, b"@ultra long"), rand_read(rng, 300, b"@t")]
    data, info, want = check(hostlib, tmp_path, fastq(reads), whole([300, 1_200_000, 300]))
    assert info["n_blocks"] >= 2 * 1_200_000 // emu_gz.block_bytes()
    assert len(data) < level(want, 1)


def test_300_base_reads_only(hostlib, tmp_path):
    rng = np.random.default_rng(8)
    reads = [rand_read(rng, 300, b"@short%d ch=%d" % (i, i % 7)) for i in range(400)]
    data, info, want = check(hostlib, tmp_path, fastq(reads), whole([300] * 400))
    l1 = level(want, 1)
    print("300-base reads: text %d, device form %d, raw level 1 %d (%.3f x)" % (len(want), len(data), l1, len(data) / l1))
    assert info["n_blocks"] == -(-len(want) // emu_gz.block_bytes())  # short lines are merged up to the block size
    assert len(data) <= 1.05 * l1


def test_high_bytes_strand_names_and_crlf(hostlib, tmp_path):
    rng = np.random.default_rng(9)
    reads = []
    for i in range(40):
        name = b"@r%d \xc3\xa9\xff\x80 caf\xe9" % i
        reads.append(rand_read(rng, int(rng.integers(1, 3000)), name, b"+" + name[1:] if i % 2 else b"+"))
    lens = [len(r[1]) for r in reads]
    text = fastq(reads)
    check(hostlib, tmp_path, text, whole(lens))
    crlf = text.replace(b"\n", b"\r\n")
    data, info, want = check(hostlib, tmp_path, crlf, whole(lens))
    assert b"\r" not in want and want == text


def test_one_symbol_block(hostlib, tmp_path):
    """a block that holds one byte value only: a two-symbol code (the byte and end-of-block)"""
    B = emu_gz.block_bytes()
    n = 3 * B
    reads = [(b"@" + b"A" * (B - 2), b"A" * n, b"+", b"A" * n)]
    data, info, want = check(hostlib, tmp_path, fastq(reads), whole([n]))
    assert len(data) < len(want) // 7
    for k in (1, 2, B - 1, B, B + 1):
        g, d = emu_gz.deflate(b"G" * k)
        assert inflate_all(g, k) == b"G" * k


def test_fibonacci_name_needs_the_length_limit(hostlib, tmp_path):
    """70 000 name bytes whose counts fall off like Fibonacci numbers: an unlimited Huffman code would be 20+ bits deep"""
    rng = np.random.default_rng(10)
    fib = [1, 1]
    while sum(fib) < 70_000:
        fib.append(fib[-1] + fib[-2])
    alphabet = [c for c in range(40, 40 + len(fib))]
    name = np.concatenate([np.full(f, c, np.uint8) for f, c in zip(fib, alphabet)])[:69_999]
    rng.shuffle(name)
    assert len(fib) >= 22
    reads = [(b"@" + name.tobytes(), b"ACGT" * 50, b"+", b"I" * 200)]
    data, info, want = check(hostlib, tmp_path, fastq(reads), whole([200]))
    assert len(data) < len(want) // 2  # (coded, not stored)
    # ... but cut into blocks of 16 384 bytes no block's tree is deeper than 15: every block costs exactly the optimum
    ms = [gz_cases.check_block(b, 1) for b in gz_cases.member_blocks(data, want)]
    assert all(not m["stored"] and m["depth"] <= 15 and m["cost"] == m["optimum"] for m in ms)
    # the limit is reached by Lucas counts in ONE block: the unlimited tree is 18 deep, the longest code has 15 bits
    blk = gz_cases.block_battery()["lucas_sorted"]
    g, d = emu_gz.deflate(blk)
    assert inflate_all(g, d["total"]) == blk
    m = gz_cases.check_block(gz_cases.member_blocks(g, blk, [0])[0], 1)
    gz_cases.check_case("lucas_sorted", m, alone=True)
    assert m["depth"] == 18 and m["longest"] == 15 and m["optimum"] == 39566


def test_random_name_is_stored(hostlib, tmp_path):
    rng = np.random.default_rng(11)
    pool = np.array([c for c in range(256) if c not in (10, 13)], np.uint8)
    name = pool[rng.integers(0, len(pool), 69_999)].tobytes()
    reads = [(b"@" + name, b"ACGT" * 50, b"+", b"I" * 200)]
    data, info, want = check(hostlib, tmp_path, fastq(reads), whole([200]))
    B = emu_gz.block_bytes()
    assert len(data) <= emu_gz.bound(len(want), info["n_blocks"])
    assert len(data) > 4 * B  # (the name went out as it is)
    assert data[10] == 0 and data[11:15] == bytes([B & 255, B >> 8, ~B & 255, (~B >> 8) & 255])  # a stored block of B bytes


def test_crc_stage_at_stretch_boundaries():
    rng = np.random.default_rng(12)
    S, B = emu_gz.stretch(), emu_gz.block_bytes()
    data = rng.integers(0, 256, 3 * B + 2, dtype=np.uint8).tobytes()
    for n in sorted({1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 77 * S - 1, 77 * S + 1, B - S - 1, B - S, B - S + 1, B - 1, B, B + 1,
                     B + S - 1, B + S + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 2}):
        g, d = emu_gz.deflate(data[:n])
        assert d["crc"] == zlib.crc32(data[:n]), n
        assert inflate_all(g, n) == data[:n]
    text = (b"@q\nACGTTGCA\n+\nIIIIHHHH\n") * 3000
    g, d = emu_gz.deflate(text)
    assert d["crc"] == zlib.crc32(text) and inflate_all(g, len(text)) == text


def test_the_reference_itself():
    """tests/gz_cases.py against itself and against zlib: the length-limited optimum is the Huffman cost when the limit does not
    bind, never falls when the limit shrinks, and the header parser reads what zlib writes"""
    rng = np.random.default_rng(13)
    for k in range(40):
        f = (rng.geometric(rng.uniform(0.002, 0.5), int(rng.integers(1, 258))) - 1) * (rng.random() < 0.8 or 1)
        depth, cost = gz_cases.huffman_depth(f), gz_cases.huffman_cost(f)
        assert gz_cases.package_merge(f, max(depth, 1)) == cost == gz_cases.package_merge(f, 32)
        if depth > 9:
            assert gz_cases.package_merge(f, depth - 1) > cost
            assert gz_cases.package_merge(f, 9) >= gz_cases.package_merge(f, 10) >= cost
    assert gz_cases.package_merge([1, 1, 2, 3, 5, 8, 13], 3) == 2 * 13 + 3 * 20  # (7 leaves in 3 bits: one code of 2 bits, the commonest symbol's)
    assert gz_cases.huffman_depth([1, 1] + gz_cases.lucas_counts()[1:]) == 18
    text = exact_text(9000)
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    raw = c.compress(text) + c.flush()
    h = gz_cases.parse_dynamic_header(raw)
    freqs = np.bincount(np.frombuffer(text, np.uint8), minlength=257)
    freqs[256] = 1
    lens = np.array(h["lit"] + [0] * (257 - len(h["lit"])))[:257]
    assert h["final"] == 1 and ((lens > 0) == (freqs > 0)).all() and gz_cases.kraft(lens, 15) == 1 << 15
    assert int((freqs * lens).sum()) == gz_cases.huffman_cost(freqs) == gz_cases.package_merge(freqs, 15)
    assert h["end"] + int((freqs * lens).sum()) <= 8 * len(raw) < h["end"] + int((freqs * lens).sum()) + 8


@pytest.mark.parametrize("name", gz_cases.BATTERY_NAMES)
def test_battery_block_alone(name):
    """every input that reaches a limit of the coder (tests/gz_cases.py), as a deflate block of its own"""
    blk = gz_cases.block_battery()[name]
    g, d = emu_gz.deflate(blk)
    assert inflate_all(g, len(blk)) == blk and d["crc"] == zlib.crc32(blk) and d["n_blocks"] == 1
    m = gz_cases.check_block(gz_cases.member_blocks(g, blk, [0])[0], 1)
    print(gz_cases.excess_line(name, m))
    gz_cases.check_case(name, m, alone=True)


def test_battery_in_name_lines(hostlib, tmp_path):
    """the battery through the layout, the compose and the block kernels: FASTQ with every block in a name line"""
    text, where = gz_cases.as_fastq(gz_cases.block_battery())
    data, info, want = check(hostlib, tmp_path, text, whole(lengths(text)))
    assert want == text
    blocks = gz_cases.member_blocks(data, want)
    assert len(blocks) == info["n_blocks"]
    for name, m in gz_cases.check_battery(blocks, where, 1).items():
        print(gz_cases.excess_line(name, m))


def test_tail_lengths(hostlib, tmp_path):
    """the last block's length at the edges of a thread's stretch of 64 symbols and of the 16-byte loads and stores"""
    for r in gz_cases.TAIL_LENGTHS:
        text = gz_cases.tail_text(r)
        data, info, want = check(hostlib, tmp_path, text, whole(lengths(text)))
        blocks = gz_cases.member_blocks(data, want)
        assert want == text and len(blocks) == info["n_blocks"] == 4 and blocks[-1]["n"] == r
        for b in blocks:
            gz_cases.check_block(b, 1)
