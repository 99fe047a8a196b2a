"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_frag/emu_frag_run: the fragment forms of the device output (csrc/frag_index.h, the
k_gz_*_frag kernels of gz_emit.h, the k_emit_*_frag / k_emit_mask kernels of emit.h) on the host (tests/emu/hip_emu.h), with
AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.  One job per run:
    in:  u64 text bytes, records, fragments, regions, fragment capacity, bgzf (0 / 1), CSR capacity in reads, in bytes; u32 counts[4]
         (what k_break_mask leaves: fragments, regions, the overflow flag, 0); the text (regular: four lines a record, "\\n" ends);
         the records (36 bytes each); the fragment list (32 each, in ANY order); the regions (8 each)
    out: FragIndex (n, status); first[records + 1]; order[n];
         GzHeader after the layout, and for status 0: rec_off[n + 1], blk_start[blocks + 1], the composed text, GzHeader after the
         finish, the member (or the BGZF blocks);
         fpl_emit_info, d_off_out[0], and for status 0: d_off_out[1 ..], d_src, d_kind, the break_no array, bases, qualities
Every buffer the kernels see is a heap block of exactly its promised size, so leaving one ends the run with a report."""
import os
import struct

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_frag_run")
GZ_HEADER = struct.Struct("<QQIIII")
GZ_FIELDS = ("total", "gz_len", "n_blocks", "status", "crc", "pad")
EMIT_INFO = struct.Struct("<QIII12x")


def build():
    return cbuild.emu_program(EXE, "tests/emu_frag/driver.cpp", __file__)


def _take(raw, at, dtype, n):
    a = np.frombuffer(raw, dtype, n, at).copy()
    return a, at + a.nbytes


def run(text, res, frags, regs, frag_cap=None, bgzf=False, cap_reads=None, cap_bytes=None, overflow=False, count=None):
    """-> dict: index (n, status, first, order), gz (layout header, rec_off, blk_start, composed, header, bytes), csr (info fields,
    off, src, kind, break_no, seq, qual).  frag_cap: the list's capacity (default: a little more than it holds); count: what
    counts[0] says (default: the list's length); overflow: counts[2]"""
    res, frags, regs = np.ascontiguousarray(res), np.ascontiguousarray(frags), np.ascontiguousarray(regs)
    n_rec, n_frag, n_reg = len(res), len(frags), len(regs)
    frag_cap = n_frag + 7 if frag_cap is None else frag_cap
    cap_reads = n_frag if cap_reads is None else cap_reads
    cap_bytes = len(text) // 2 if cap_bytes is None else cap_bytes

    def payload(f):
        f.write(struct.pack("<8Q4I", len(text), n_rec, n_frag, n_reg, frag_cap, int(bgzf), cap_reads, cap_bytes,
                            n_frag if count is None else count, n_reg, int(overflow), 0))
        f.write(text + res.tobytes() + frags.tobytes() + regs.tobytes())

    raw = emujob.run(build(), payload, "emu_frag_")
    n, status = struct.unpack_from("<II", raw, 0)
    n = 0 if status else n  # (frag_index_len: under a status there is no list)
    at = 8
    first, at = _take(raw, at, "<u4", n_rec + 1)
    order, at = _take(raw, at, "<u4", n)
    out = dict(index=dict(n=n, status=status, first=first, order=order))
    lay = dict(zip(GZ_FIELDS, GZ_HEADER.unpack_from(raw, at)))
    at += GZ_HEADER.size
    gz = dict(layout=lay)
    if lay["status"] == 0:
        gz["rec_off"], at = _take(raw, at, "<u8", n + 1)
        gz["blk_start"], at = _take(raw, at, "<u8", lay["n_blocks"] + 1)
        gz["composed"] = raw[at:at + lay["total"]]
        at += lay["total"]
        gz["header"] = dict(zip(GZ_FIELDS, GZ_HEADER.unpack_from(raw, at)))
        at += GZ_HEADER.size
        m = gz["header"]["gz_len"] if lay["total"] and gz["header"]["status"] == 0 else 0
        gz["bytes"] = raw[at:at + m]
        at += m
    out["gz"] = gz
    n_bytes, n_out, max_len, st = EMIT_INFO.unpack_from(raw, at)
    at += EMIT_INFO.size
    off0, at = _take(raw, at, "<u8", 1)
    csr = dict(n_bytes=n_bytes, n_out=n_out, max_len=max_len, status=st, off0=int(off0[0]))
    if st == 0:
        rest, at = _take(raw, at, "<u8", n_out)
        csr["off"] = [int(off0[0])] + rest.tolist()
        csr["src"], at = _take(raw, at, "<u4", n_out)
        csr["kind"], at = _take(raw, at, "u1", n_out)
        csr["break_no"], at = _take(raw, at, "<u2", n_out)
        csr["seq"] = raw[at:at + n_bytes]
        csr["qual"] = raw[at + n_bytes:at + 2 * n_bytes]
        at += 2 * n_bytes
    out["csr"] = csr
    assert at == len(raw)
    return out
