"""The BAM forms of the gzip layout and compose kernels (fastplong_amd/csrc/gz_emit.h: k_gz_layout_bam, k_gz_compose_bam) on the CPU
emulator, behind the decode kernel and in front of the unchanged block kernels.

The expected bytes never come from the kernels: the composed text is compared with what the host's formatter (fplh_format_batch)
writes for the FASTQ twin of the records (tests/bamio.py) and the same per-read records, the member is inflated with zlib / gzip /
libdeflate (CRC-32 and ISIZE checked), and the block starts are compared with a plain restatement of the block rule.

The text form shares its cuts, its length arithmetic and its compose loop with the BAM form (one template over a record source).
TEXT_MEMBERS pins that the refactor changed nothing: the SHA-256 of the members the emulator's text form gives on inputs of
tests/test_gz_emit_emu.py, TAKEN FROM THE PARENT COMMIT'S BUILD (the commit before the BAM form existed)."""
import hashlib
import os
import zlib

import numpy as np
import pytest

from fastplong_amd import abi
from tests import bamio
from tests.gzcheck import GOLD, gz, host_format, inflate_all, load_hostlib

RES = np.dtype(abi.RESULT_DTYPE)


@pytest.fixture(scope="module")
def hostlib():
    return load_hostlib()


@pytest.fixture(scope="module")
def emu():
    from tests.emu_bamgz import build
    build.lib()
    return build


def stream(records, n_cigar=2, tags=b"NMi\x05\0\0\0RGZgrp1\0"):
    """records -> (uncompressed record bytes, record starts, CSR offsets, twin text)"""
    _, starts, raw = bamio.bam_bytes(records, n_cigar=n_cigar, tags=tags)
    off = np.zeros(len(records) + 1, np.uint64)
    off[1:] = np.cumsum([len(r[2]) for r in records])
    # (a name ends at its first NUL, as bamio.parse and the host's reader take it: random_records' names have some inside)
    return raw, np.array(starts, np.uint64), off, b"".join(bamio.twin_record(r[0].split(b"\0")[0], *r[1:]) for r in records)


def whole(lengths, code=abi.FPL_PASS_FILTER):
    res = np.zeros(len(lengths), RES)
    res["n_frag"] = 1
    res["frag_len"][:, 0] = lengths
    res["r1_len"] = lengths
    res["code"][:, 0] = code
    return res


def made_up(rng, lengths):
    """records as no run would give them, but every shape the output rule knows: pass / fail / dropped, one and two fragments with
    kind 1 and 2, frag_start > 0"""
    res = whole(lengths)
    for i, L in enumerate(lengths):
        k = int(rng.integers(0, 8))
        if k == 0:
            res[i]["code"][0] = abi.FPL_FAIL_LENGTH
        elif k == 1:
            res[i]["dropped"] = 1
        elif k in (2, 3) and L >= 2:
            cut = int(rng.integers(1, L))
            a0 = int(rng.integers(0, cut))
            b0 = int(rng.integers(cut, L))
            res[i]["n_frag"] = 2
            res[i]["frag_start"][:] = [a0, b0]
            res[i]["frag_len"][:] = [cut - a0, L - b0]
            res[i]["kind"][:] = [1, 2]
            if k == 3:
                res[i]["code"][int(rng.integers(0, 2))] = abi.FPL_FAIL_QUALITY
        elif k == 4 and L >= 3:
            s = int(rng.integers(1, L))
            res[i]["frag_start"][0] = s
            res[i]["frag_len"][0] = int(rng.integers(0, L - s + 1))
            res[i]["kind"][0] = int(rng.integers(0, 3))
    return res


def block_rule(records, res, B, L):
    """the block starts, restated: every multiple of B of the output, and for a fragment whose bases line has at least L bytes its
    name line and its '+' line"""
    starts, o = [], 0

    def cuts(s, e, force):
        if e <= s:
            return
        if force or s % B == 0:
            starts.append(s)
        starts.extend(range((s // B + 1) * B, e, B))

    for (name, flag, codes, qual), r in zip(records, res):
        if r["dropped"]:
            continue
        nl = 1 + len(name.split(b"\0")[0])
        for f in range(min(int(r["n_frag"]), 2)):
            if r["code"][f] != abi.FPL_PASS_FILTER:
                continue
            fl = int(r["frag_len"][f])
            a = nl + {1: 22, 2: 23}.get(int(r["kind"][f]), 0) + 1 + fl + 1
            b = 1 + 1 + fl + 1
            if fl + 1 >= L:
                cuts(o, o + a, True)
                cuts(o + a, o + a + b, True)
            else:
                cuts(o, o + a + b, False)
            o += a + b
    return starts + [o]


def check(emu, hostlib, tmp_path, records, res):
    raw, starts, off, twin = stream(records)
    want = host_format(hostlib, tmp_path, twin, res)
    data, info, comp, blk = emu.emit(raw, starts, off, res)
    assert comp == want  # k_bam_decode + k_gz_layout_bam + k_gz_compose_bam
    assert info["total"] == len(want)
    assert blk == block_rule(records, res, emu.block_bytes(), emu.long_line())
    assert all(0 < b - a <= emu.block_bytes() for a, b in zip(blk, blk[1:]))
    if not want:
        assert data == b"" and info["n_blocks"] == 0
        return data, info, want
    assert len(data) == info["gz_len"] <= emu.bound(info["total"], info["n_blocks"])
    assert inflate_all(data, len(want)) == want
    assert info["crc"] == zlib.crc32(want)
    assert data[-8:] == zlib.crc32(want).to_bytes(4, "little") + (len(want) % 2 ** 32).to_bytes(4, "little")
    return data, info, want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_records(emu, hostlib, tmp_path, seed):
    rng = np.random.default_rng(seed)
    recs = bamio.random_records(rng, 300, max_len=700, flags=(0, 0x10, 0x4, 0x14))
    lens = [len(r[2]) for r in recs]
    assert {0, 1, 2, 3} <= set(lens)
    data, info, want = check(emu, hostlib, tmp_path, recs, made_up(rng, lens))
    assert b"@split-by-adapter-left-r" in want and b"@split-by-adapter-right-r" in want
    check(emu, hostlib, tmp_path, recs, whole(lens))
    data, info, want = check(emu, hostlib, tmp_path, recs, whole(lens, abi.FPL_FAIL_N_BASE))
    assert want == b"" and data == b""


def test_no_records(emu, hostlib, tmp_path):
    data, info, want = check(emu, hostlib, tmp_path, [], whole([]))
    assert data == b""


def test_empty_read_name_is_what_the_formatter_writes(emu, hostlib, tmp_path):
    """l_read_name == 1: the name line is the lone '@', which is NOT an empty line -- the prefix of a split read goes in behind it"""
    rng = np.random.default_rng(5)
    recs = bamio.random_records(rng, 12, flags=(0, 0x10), lengths=[40, 0, 1, 2000])
    recs = [(b"" if i % 2 == 0 else r[0], r[1], r[2], r[3]) for i, r in enumerate(recs)]
    lens = [len(r[2]) for r in recs]
    res = whole(lens)
    res[0]["n_frag"] = 2
    res[0]["frag_start"][:] = [1, 20]
    res[0]["frag_len"][:] = [15, 20]
    res[0]["kind"][:] = [1, 2]
    res[4]["kind"][0] = 2
    data, info, want = check(emu, hostlib, tmp_path, recs, res)
    assert want.startswith(b"@split-by-adapter-left-\n") and b"\n@split-by-adapter-right-\n" in want and b"\n@\n" in want


def test_names_of_1_and_254_bytes_and_a_name_with_a_nul_inside(emu, hostlib, tmp_path):
    rng = np.random.default_rng(6)
    recs = bamio.random_records(rng, 9, flags=(0, 0x10), lengths=[300, 5, 1500])
    names = [b"x", bytes(rng.integers(33, 127, 254, dtype=np.uint8)), b"ab\0cd", b"\xc3\xa9\xff\x80", b"12345678", b"1234567", b"123456789",
             b"q" * 16, b"z" * 17]
    recs = [(n, r[1], r[2], r[3]) for n, r in zip(names, recs)]
    lens = [len(r[2]) for r in recs]
    res = whole(lens)
    res["kind"][:, 0] = [0, 1, 2, 0, 1, 2, 0, 1, 2]
    data, info, want = check(emu, hostlib, tmp_path, recs, res)
    assert b"@split-by-adapter-right-ab\n" in want
    assert b"@split-by-adapter-left-" + names[1] + b"\n" in want


def test_reads_on_both_sides_of_the_long_line(emu, hostlib, tmp_path):
    rng = np.random.default_rng(7)
    L = emu.long_line()
    assert L == 1024
    lens = [50, L - 2, 60, L - 1, 70, L, 80, L + 1, 90]
    recs = bamio.random_records(rng, len(lens), flags=(0, 0x10), lengths=lens)
    data, info, want = check(emu, hostlib, tmp_path, recs, whole(lens))
    # the block at 0, then two for every fragment of L - 1 bases and more (a bases line of L bytes with its line end); the short
    # read behind a long one joins its quality block
    assert info["n_blocks"] == 1 + 2 * 3
    res = whole(lens)
    res["frag_start"][:, 0] = 1
    res["frag_len"][:, 0] -= 1
    check(emu, hostlib, tmp_path, recs, res)


def test_reads_that_span_several_blocks(emu, hostlib, tmp_path):
    rng = np.random.default_rng(8)
    B = emu.block_bytes()
    lens = [3 * B + 5, 10, 2 * B, 0, B - 1, B, 5 * B + 17, 1]
    recs = bamio.random_records(rng, len(lens), flags=(0, 0x10), lengths=lens)
    data, info, want = check(emu, hostlib, tmp_path, recs, whole(lens))
    assert info["n_blocks"] >= 2 * sum(l // B for l in lens)
    res = whole(lens)
    res[0]["n_frag"] = 2
    res[0]["frag_start"][:] = [3, B + 100]
    res[0]["frag_len"][:] = [B + 1, 2 * B - 100]
    res[0]["kind"][:] = [1, 2]
    res[6]["frag_start"][0], res[6]["frag_len"][0] = 4 * B, B
    check(emu, hostlib, tmp_path, recs, res)


# ---- the text form is what it was ----
TEXT_MEMBERS = {  # SHA-256 of the member, from the parent commit's build of tests/emu_gz
    "split": "08a4c100afc6d0d502f8ac123ad8fc81631f675bb8e0b5193c3887e62b80d951",
    "long": "d9d4bb90eaf342be686f37166a3ce32cfd32b01af992fe90e1323e9e286fa641",
    "high_bytes": "ba9207d819199d08cb8927fd03f29cd0bf9a6b8c038ea8dbbbd8280fb65b5446",
    "crlf": "ba9207d819199d08cb8927fd03f29cd0bf9a6b8c038ea8dbbbd8280fb65b5446",
    "short": "9429b977782602266c0ca051b048385aa628fc3023cb38dd9ba51251ff2201aa",
    "golden_c3_whole": "53ba8bbfd40412e93bc849a0d461fe64d557b2e0a10613b9170f413f79f9caf4",
}


def fastq(reads):
    return b"".join(b"%s\n%s\n%s\n%s\n" % r for r in reads)


def rand_read(rng, n, name, strand=b"+"):
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    q = np.clip(rng.normal(22, 7, n), 1, 60).astype(np.uint8) + 33
    return (name, s, strand, q.tobytes())


def text_input(which):
    """inputs of tests/test_gz_emit_emu.py, built the same way"""
    if which == "split":
        rng = np.random.default_rng(6)
        reads = [rand_read(rng, 5000, b"@a"), rand_read(rng, 9000, b"@split me", b"+split me"), rand_read(rng, 40, b"@z")]
        res = whole([5000, 9000, 40])
        res[1]["n_frag"] = 2
        res[1]["frag_start"][:] = [17, 4100]
        res[1]["frag_len"][:] = [3000, 4883]
        res[1]["kind"][:] = [1, 2]
        res[0]["frag_start"][0], res[0]["frag_len"][0] = 33, 4000
        return fastq(reads), res
    if which == "long":
        rng = np.random.default_rng(3)
        text = fastq([rand_read(rng, int(n), b"@r%d runid=0a1b ch=%d" % (i, i)) for i, n in enumerate(rng.integers(5000, 30000, 24))])
        return text, whole([len(l) for l in text.split(b"\n")[1::4]])
    if which in ("high_bytes", "crlf"):
        rng = np.random.default_rng(9)
        reads = []
        for i in range(40):
            name = b"@r%d \xc3\xa9\xff\x80 caf\xe9" % i
            reads.append(rand_read(rng, int(rng.integers(1, 3000)), name, b"+" + name[1:] if i % 2 else b"+"))
        text = fastq(reads)
        return (text if which == "high_bytes" else text.replace(b"\n", b"\r\n")), whole([len(r[1]) for r in reads])
    if which == "short":
        rng = np.random.default_rng(8)
        reads = [rand_read(rng, 300, b"@short%d ch=%d" % (i, i % 7)) for i in range(400)]
        res = whole([300] * 400)
        res["dropped"][::7] = 1
        res["code"][3::5, 0] = abi.FPL_FAIL_LENGTH
        return fastq(reads), res
    text = gz(os.path.join(GOLD, "c3_full", "in.fq.gz"))
    return text, whole([len(l) for l in text.split(b"\n")[1::4]])


@pytest.mark.parametrize("which", sorted(TEXT_MEMBERS))
def test_text_form_members_are_those_of_the_parent_commit(which):
    from tests.emu_gz import build as emu_gz
    text, res = text_input(which)
    data, info = emu_gz.emit(text, res)
    assert hashlib.sha256(data).hexdigest() == TEXT_MEMBERS[which]
