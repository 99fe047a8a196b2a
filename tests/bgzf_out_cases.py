"""Test helpers shared by the BGZF output tests (tests/test_bgzf_out_emu.py, tests/test_gpu_bgzf_out.py, tests/test_host_bgzf_out.py,
tests/test_cli_bgzf_out_stub.py): the input texts of the cases and the checks every BGZF output has to meet."""
import gzip
import struct

import numpy as np

from fastplong_amd import bgzf

STRIPE = 49152     # fpl::GZ_STRIPE: the text bytes of a device-framed block
HOST_PIECE = 65280  # the text bytes of a host-framed block (htslib's size)
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
EDGE_TOTALS = [49151, 49152, 49153, 98304]


def rand_read(rng, n, name):
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()
    q = (np.clip(rng.normal(22, 7, n), 1, 60).astype(np.uint8) + 33).tobytes()
    return b"%s\n%s\n+\n%s\n" % (name, s, q)


def exact_text(total, seed=11):
    """regular FASTQ ('+' third lines) of exactly `total` bytes: reads of 600 bases, the last one sized to fit"""
    rng = np.random.default_rng(seed)
    out, i = b"", 0
    while total - len(out) > 2500:
        out += rand_read(rng, 600, b"@e%d" % i)
        i += 1
    left = total - len(out)  # a record is len(name) + 2 n + 5 bytes
    name = b"@z" if left % 2 else b"@zz"
    out += rand_read(rng, (left - len(name) - 5) // 2, name)
    assert len(out) == total
    return out


def forced_starts_text(seed=12):
    """40 reads of 1 024 - 1 100 bases: two forced block starts per record, about 45 deflate blocks in one stripe"""
    rng = np.random.default_rng(seed)
    return b"".join(rand_read(rng, int(n), b"@f%d ch=%d" % (i, i % 5)) for i, n in enumerate(rng.integers(1024, 1101, 40)))


def short_reads_text(seed=13):
    rng = np.random.default_rng(seed)
    return b"".join(rand_read(rng, int(n), b"@s%d" % i) for i, n in enumerate(rng.integers(20, 201, 3000)))


def one_long_read_text(seed=14):
    return rand_read(np.random.default_rng(seed), 200_000, b"@one read over nine stripes")


def lengths(text):
    return [len(l.rstrip(b"\r")) for l in text.split(b"\n")[1::4]]


def split_blocks(data, eof=False):
    """the BGZF blocks of data as byte strings, the structure checked: the exact 18-byte header, sizes, and -- with eof -- the EOF
    block at the end (left out of the result).  The blocks cover data exactly."""
    out, pos = [], 0
    while pos < len(data):
        n = bgzf.block_len(data, pos)
        assert data[pos:pos + 16] == HEAD, "header at %d" % pos
        assert struct.unpack_from("<H", data, pos + 16)[0] == n - 1 and n <= 65536
        out.append(data[pos:pos + n])
        pos += n
    assert pos == len(data)
    if eof:
        assert out and out[-1] == bgzf.EOF
        out.pop()
        assert bgzf.EOF not in out
    return out


def check_blocks(data, want, piece=None, eof=False):
    """data is BGZF blocks that inflate, block by block, to want (gzip.decompress checks every block's CRC-32 and ISIZE);
    piece: every block but the last holds exactly that many bytes.  -> the blocks"""
    blocks = split_blocks(data, eof)
    desc, _ = bgzf.blocks(data)
    assert len(desc) == len(blocks)  # (no empty block in front of the end)
    got = []
    for k, b in enumerate(blocks):
        t = gzip.decompress(b)
        assert len(t) == struct.unpack_from("<I", b, len(b) - 4)[0] <= 65536
        if piece is not None and k + 1 < len(blocks):
            assert len(t) == piece, (k, len(t))
        got.append(t)
    assert b"".join(got) == want
    if piece is not None:
        assert len(blocks) == -(-len(want) // piece)
    return blocks
