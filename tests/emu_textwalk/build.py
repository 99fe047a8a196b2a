"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_textwalk/emu_textwalk_run: the kernels of fastplong_amd/csrc/text_walk.h and
text_parse.h on the host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.
A script of operations on one context at a time goes in as a file and the results come out as one:
    in:  u64 n_ops; per op u64 kind and
           0 new context:  u64 tail_cap
           1 submission:   u64 n_bytes, n_blocks; the inflated bytes; u32 status per block
           2 tail out
           3 tail in:      u64 len; the bytes          (clears the refusal flag; len 0: a new file)
           4 resume                                    (clears the refusal flag)
           5 tail capacity: u64 bytes
           6 whole chunk:  u64 n_bytes (> 0); the bytes   (the six kernels of fpl_process_text_async, no context)
    out: 1: i64 rc (-1: the arguments were refused), fpl_text_window, u64 lo (where the text started in the buffer), and for rc 0
            and status 0 the line starts [4 n] (u32, buffer positions), the read lengths [n] (u32), the offsets [n + 1], the name
            offsets [n + 1], the names, the bases and the qualities
         2: u64 len; the bytes
         6: TextHeader, and for status 0 the line starts [4 n], the lengths [n], the offsets [n + 1], the bases and the qualities
Every buffer the kernels see is a heap block of exactly its promised size, so leaving one ends the run with a report."""
import os
import struct

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_textwalk_run")
WINDOW = struct.Struct("<IIQIIQQIIQQ")
FIELDS = ("status", "n_reads", "n_bases", "max_read_len", "n_lines", "name_bytes", "records_seen", "tail_bytes", "reserved", "bad_index",
          "bad_pos")
HEADER = struct.Struct("<IIIIQQ")
HEADER_FIELDS = ("n_lines", "n_records", "status", "max_len", "n_bases", "bad_record")
NONE = (1 << 64) - 1


def build():
    return cbuild.emu_program(EXE, "tests/emu_textwalk/driver.cpp", __file__, main="EMU_TEXTWALK_MAIN")


def new(tail_cap):
    return ("new", int(tail_cap))


def submit(data, block_status=()):
    return ("submit", bytes(data), list(block_status))


def whole(data):
    return ("whole", bytes(data))


def _take(raw, at, dtype, n):
    a = np.frombuffer(raw, dtype, n, at).copy()
    return a, at + a.nbytes


def run(ops):
    """ops: a list of new() / submit() / whole() / ("tail_get",) / ("tail_set", bytes) / ("resume",) / ("reserve", bytes) -> one
    result per submit (a dict: rc, lo, the header's fields, and for an accepted one line, len, off, name_off, names, seq, qual), per
    whole (a dict: the TextHeader's fields, and for status 0 line, len, off, seq, qual) and per tail_get (bytes), in order; raises
    with the sanitizers' report when the run did not end clean"""
    def payload(f):
        f.write(struct.pack("<Q", len(ops)))
        for op in ops:
            if op[0] == "submit":
                _, data, bst = op
                f.write(struct.pack("<3Q", 1, len(data), len(bst)) + data + struct.pack("<%dI" % len(bst), *bst))
            elif op[0] == "whole":
                f.write(struct.pack("<QQ", 6, len(op[1])) + op[1])
            elif not emujob.write_context_op(f, op):
                raise ValueError(op[0])

    raw = emujob.run(build(), payload, "emu_textwalk_")
    res, at = [], 0
    for op in ops:
        if op[0] == "submit":
            (rc,) = struct.unpack_from("<q", raw, at)
            r = dict(zip(FIELDS, WINDOW.unpack_from(raw, at + 8)), rc=rc)
            at += 8 + WINDOW.size
            (r["lo"],) = struct.unpack_from("<Q", raw, at)
            at += 8
            if rc == 0 and r["status"] == 0:
                n = r["n_reads"]
                r["line"], at = _take(raw, at, "<u4", 4 * n)
                r["line"] = r["line"].reshape(n, 4)
                r["len"], at = _take(raw, at, "<u4", n)
                r["off"], at = _take(raw, at, "<u8", n + 1)
                r["name_off"], at = _take(raw, at, "<u8", n + 1)
                for key, m in (("names", r["name_bytes"]), ("seq", r["n_bases"]), ("qual", r["n_bases"])):
                    r[key] = raw[at:at + m]
                    at += m
            res.append(r)
        elif op[0] == "whole":
            r = dict(zip(HEADER_FIELDS, HEADER.unpack_from(raw, at)))
            at += HEADER.size
            if r["status"] == 0:
                n = r["n_records"]
                r["line"], at = _take(raw, at, "<u4", 4 * n)
                r["line"] = r["line"].reshape(n, 4)
                r["len"], at = _take(raw, at, "<u4", n)
                r["off"], at = _take(raw, at, "<u8", n + 1)
                for key in ("seq", "qual"):
                    r[key] = raw[at:at + r["n_bases"]]
                    at += r["n_bases"]
            res.append(r)
        elif op[0] == "tail_get":
            (n,) = struct.unpack_from("<Q", raw, at)
            res.append(raw[at + 8:at + 8 + n])
            at += 8 + n
    assert at == len(raw)
    return res
