"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bamwalk/emu_bamwalk_run: the kernels of fastplong_amd/csrc/bam_walk.h on the host
(tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own.  A script of operations on
one context at a time goes in as a file and the results come out as one:
    in:  u64 n_ops; per op u64 kind and
           0 new context:  u64 tail_cap
           1 submission:   u64 n_bytes, skip, seg_bytes, rec_cap (0: the library's), n_blocks; the inflated bytes; u32 status per block
           2 tail out
           3 tail in:      u64 len; the bytes          (clears the refusal flag; len 0: a new file)
           4 resume                                    (clears the refusal flag)
           5 tail capacity: u64 bytes
    out: 1: i64 rc (-1: the arguments were refused), fpl_bam_window, u64 n_seg, the candidates, and for rc 0 and status 0 the record
            starts [n], the offsets [n + 1], the name offsets [n + 1] and the names
         2: u64 len; the bytes
Every buffer the kernels see is a heap block of exactly its promised size, so leaving one ends the run with a report."""
import os
import struct

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bamwalk_run")
WINDOW = struct.Struct("<IIQIIQQIIQQ")
FIELDS = ("status", "n_reads", "n_bases", "max_read_len", "segments", "name_bytes", "records_seen", "tail_bytes", "rewalked", "bad_index",
          "bad_pos")
NO_CAND = (1 << 64) - 1


def build():
    return cbuild.emu_program(EXE, "tests/emu_bamwalk/driver.cpp", __file__, main="EMU_BAMWALK_MAIN")


def new(tail_cap):
    return ("new", int(tail_cap))


def submit(data, skip=0, seg_bytes=256, rec_cap=0, block_status=()):
    return ("submit", bytes(data), int(skip), int(seg_bytes), int(rec_cap), list(block_status))


def run(ops):
    """ops: a list of new() / submit() / ("tail_get",) / ("tail_set", bytes) / ("resume",) / ("reserve", bytes) -> one result per
    submit (a dict: rc, the header's fields, cand, and for an accepted one rec, off, name_off, names) and per tail_get (bytes), in
    order; raises with the sanitizers' report when the run did not end clean"""
    def payload(f):
        f.write(struct.pack("<Q", len(ops)))
        for op in ops:
            if op[0] == "submit":
                _, data, skip, seg, cap, bst = op
                f.write(struct.pack("<6Q", 1, len(data), skip, seg, cap, len(bst)) + data + struct.pack("<%dI" % len(bst), *bst))
            elif not emujob.write_context_op(f, op):
                raise ValueError(op[0])

    raw = emujob.run(build(), payload, "emu_bamwalk_")
    res, at = [], 0
    for op in ops:
        if op[0] == "submit":
            (rc,) = struct.unpack_from("<q", raw, at)
            r = dict(zip(FIELDS, WINDOW.unpack_from(raw, at + 8)), rc=rc)
            at += 8 + WINDOW.size
            (ns,) = struct.unpack_from("<Q", raw, at)
            r["cand"] = np.frombuffer(raw, "<u8", ns, at + 8).copy()
            at += 8 + 8 * ns
            if rc == 0 and r["status"] == 0:
                n = r["n_reads"]
                r["rec"] = np.frombuffer(raw, "<u8", n, at).copy()
                at += 8 * n
                r["off"] = np.frombuffer(raw, "<u8", n + 1, at).copy()
                at += 8 * (n + 1)
                r["name_off"] = np.frombuffer(raw, "<u8", n + 1, at).copy()
                at += 8 * (n + 1)
                r["names"] = raw[at:at + r["name_bytes"]]
                at += r["name_bytes"]
            res.append(r)
        elif op[0] == "tail_get":
            (n,) = struct.unpack_from("<Q", raw, at)
            res.append(raw[at + 8:at + 8 + n])
            at += 8 + n
    assert at == len(raw)
    return res
