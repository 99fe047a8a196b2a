"""A BAM file's bytes cut into what Engine.submit_bgzf takes: the BGZF blocks' descriptors, and where the first record starts.
Pure Python; the structure checks are the reader's (host/bam.cpp): a block is a gzip member with the BC extra field."""
import struct
import zlib

import numpy as np

from . import abi


# the empty block that ends every BGZF file (SAM specification, 4.1.2)
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# the fixed header of every BAM file this project writes (README "BAM output"): magic, l_text, the text, n_ref = 0
BAM_HEADER_TEXT = b"@HD\tVN:1.6\tSO:unknown\n@PG\tID:fastplong_amd\tPN:fastplong_amd\n"


def eof():
    """the 28-byte block that ends a BGZF file"""
    return EOF


def read_group_lines(header_text):
    """every line of a BAM header's text (taken to end at its first NUL) that starts with "@RG\\t", verbatim and in order, a
    line end added where the last one lacks it: what bam_header(read_groups=...) takes"""
    lines = [l for l in header_text.split(b"\0", 1)[0].splitlines(keepends=True) if l.startswith(b"@RG\t")]
    if lines and not lines[-1].endswith(b"\n"):
        lines[-1] += b"\n"
    return b"".join(lines)


def bam_header(read_groups=b""):
    """the BGZF block that opens a BAM file of Engine.set_gzip_records(True) batches: header + the batches' bytes + eof().
    The bytes are stored, not deflated: every inflater takes that, the device's strict one included.
    read_groups: with Engine.set_bam_tags(True), the input header's "@RG\\t...\\n" lines (read_group_lines), which go between the
    @HD and the @PG line so that the records' RG:Z: fields point at something; a header of more than 65 280 bytes takes several
    blocks, which hold nothing but header."""
    hd, pg = BAM_HEADER_TEXT.split(b"\n")[0] + b"\n", BAM_HEADER_TEXT.split(b"\n")[1] + b"\n"
    text = hd + read_groups + pg
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
    out = []
    for at in range(0, len(raw), 65280):
        piece = raw[at:at + 65280]
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 18 + len(body) + 8 - 1) + body +
                   struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))
    return b"".join(out)


class BgzfError(ValueError):
    pass


def block_len(data, pos):
    """BSIZE + 1 of the block whose header starts at pos"""
    if len(data) - pos < 18 or data[pos:pos + 3] != b"\x1f\x8b\x08" or not data[pos + 3] & 4:
        raise BgzfError("no BGZF block at offset %d" % pos)
    xlen = struct.unpack_from("<H", data, pos + 10)[0]
    k = 0
    while k + 4 <= xlen:
        f = pos + 12 + k
        slen = struct.unpack_from("<H", data, f + 2)[0]
        if data[f:f + 2] == b"BC" and slen == 2:
            n = struct.unpack_from("<H", data, f + 4)[0] + 1
            if n < 12 + xlen + 8 or pos + n > len(data):
                break
            return n
        k += 4 + slen
    raise BgzfError("no BGZF block at offset %d" % pos)


def blocks(data, begin=0, end=None):
    """the blocks of data[begin:end) -> (descriptors as an array of abi.BGZF_BLOCK_DTYPE with comp_off relative to `begin` and
    out_off counted from this stretch's first inflated byte, file offsets of the blocks).  Empty blocks (the EOF marker) make no
    bytes and are left out.  Headers with a name, a comment or a header CRC (which BGZF does not allow) are refused here."""
    end = len(data) if end is None else end
    desc, offs, pos, out = [], [], begin, 0
    while pos < end:
        n = block_len(data, pos)
        if data[pos + 3] & (2 | 8 | 16):
            raise BgzfError("the block at offset %d has header fields BGZF does not allow" % pos)
        hdr = 12 + struct.unpack_from("<H", data, pos + 10)[0]
        crc, isize = struct.unpack_from("<II", data, pos + n - 8)
        if isize > 65536:
            raise BgzfError("the block at offset %d has a bad size" % pos)
        if isize:
            desc.append((pos + hdr - begin, out, n - hdr - 8, isize, crc, 1))
            offs.append(pos)
            out += isize
        pos += n
    return np.array(desc, dtype=np.dtype(abi.BGZF_BLOCK_DTYPE)), offs


def inflate_block(data, pos):
    """the bytes of the block at pos, by zlib (the trailer is NOT checked: the recovery path of a caller that judges it itself)"""
    n = block_len(data, pos)
    hdr = 12 + struct.unpack_from("<H", data, pos + 10)[0]
    return zlib.decompressobj(-15).decompress(data[pos + hdr:pos + n - 8])


def header_len(data):
    """bytes of the inflated stream in front of the first record: magic, l_text, text, n_ref and the references.  Inflates as many
    leading blocks as the header needs."""
    raw, pos = b"", 0

    def need(n):
        nonlocal raw, pos
        while len(raw) < n:
            if pos >= len(data):
                raise BgzfError("the file ends inside the BAM header")
            raw += inflate_block(data, pos)
            pos += block_len(data, pos)

    need(12)
    if raw[:4] != b"BAM\1":
        raise BgzfError("the inflated stream does not start with BAM\\1")
    p = 8 + struct.unpack_from("<I", raw, 4)[0]
    need(p + 4)
    n_ref = struct.unpack_from("<I", raw, p)[0]
    p += 4
    for _ in range(n_ref):
        need(p + 4)
        p += 4 + struct.unpack_from("<I", raw, p)[0]
        need(p + 4)
        p += 4
    return p
