"""usage: python tools/bam_e2e.py [--reads N] [--dir DIR] [--procs P] [--keep]
BAM input end to end on one MI355X (README "BAM input"): the configs[2] reads (bench.py's c3_full_pipeline workload,
synth.device_batch, seed 1) written as an unaligned BAM at BGZF level 1 -- by a pool of at most 16 processes, each
compressing a slice of the records into whole blocks -- and as its FASTQ twin; the CLI run on both to /dev/null with --json
and -V; the two reports must agree (all but the command line).  Prints, for each input, the whole-process time and
Gbases/s, the host pipeline's wall time and Gbases/s (the CLI's "host pipeline" line) and its busy seconds per stage, and
names the bound: the reader (BGZF inflate + record walk on the worker pool / the FASTQ parsers) or the device side
(copies + kernels).

The reads are made on the GPU in a child process of their own and handed over as .npy files; this process never opens the
GPU, so its pool may fork freely."""
import argparse
import ctypes as C
import multiprocessing as mp
import os
import re
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastplong_amd import build  # noqa: E402

CODE = np.full(256, 15, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[_c] = _i
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
FLAGS = ["-s", "AAGGATTCATTCCCACGGTAACAC", "-e", "GTGTTACCGTGGGAATGAATCCTT", "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]


def generate(d, n):
    """(child process) the configs[2] batch on cuda:0 -> seq.npy, qual.npy, off.npy"""
    import torch

    from fastplong_amd import synth

    seq_t, qual_t, off_t, _ = synth.device_batch(n, seed=1, device=torch.device("cuda:0"))
    np.save(os.path.join(d, "seq.npy"), seq_t.cpu().numpy())
    np.save(os.path.join(d, "qual.npy"), qual_t.cpu().numpy())
    np.save(os.path.join(d, "off.npy"), off_t.cpu().numpy().astype(np.uint64))


def _block(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    cdata = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 12 + 6 + len(cdata) + 8 - 1) + cdata +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


_G = {}


def _slice(args):
    """(pool worker) records [a, b) -> whole BGZF blocks in part file `path`"""
    a, b, path = args
    seq, qual, off = _G["seq"], _G["qual"], _G["off"]
    out, buf = open(path, "wb"), bytearray()
    for i in range(a, b):
        o0, o1 = int(off[i]), int(off[i + 1])
        L = o1 - o0
        codes = CODE[seq[o0:o1]]
        if L % 2:
            codes = np.append(codes, 0)
        packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
        name = b"r%d\0" % i
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, 4, L, -1, -1, 0) + name + packed + \
            (qual[o0:o1] - 33).tobytes()
        buf += struct.pack("<I", len(body)) + body
        while len(buf) >= 65280:
            out.write(_block(bytes(buf[:65280])))
            del buf[:65280]
    if buf:
        out.write(_block(bytes(buf)))
    out.close()


def write_bam(path, seq, qual, off, procs):
    n = len(off) - 1
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    hdr = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0)
    _G.update(seq=seq, qual=qual, off=off)
    k = max(1, min(procs, 16)) * 8
    cuts = [n * j // k for j in range(k + 1)]
    parts = ["%s.part%d" % (path, j) for j in range(k)]
    with mp.get_context("fork").Pool(max(1, min(procs, 16))) as pool:
        pool.map(_slice, [(cuts[j], cuts[j + 1], parts[j]) for j in range(k)])
    with open(path, "wb") as f:
        f.write(_block(hdr))
        for p in parts:
            with open(p, "rb") as g:
                while True:
                    chunk = g.read(64 << 20)
                    if not chunk:
                        break
                    f.write(chunk)
            os.unlink(p)
        f.write(EOF_BLOCK)


def run_cli(inp, d, tag, bases):
    js = os.path.join(d, tag + ".json")
    cmd = [build.CLI, "-i", inp, "-o", "/dev/null", "-j", js, "-h", os.path.join(d, tag + ".html"), "-V"] + FLAGS
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("CLI on %s failed (rc %d):\n%s" % (inp, r.returncode, r.stderr[-3000:]))
    line = next((l for l in r.stderr.splitlines() if l.startswith("host pipeline:")), "")
    m = re.search(r"wall ([0-9.e+-]+) s; busy: parse ([0-9.e+-]+) s.*copies \+ kernels \(waits\) ([0-9.e+-]+) s, format .*? ([0-9.e+-]+) s, write ([0-9.e+-]+)",
                  line)
    wall, parse, dev = (float(m.group(1)), float(m.group(2)), float(m.group(3))) if m else (float("nan"),) * 3
    print("%-5s whole process %.2f s -> %.2f Gbases/s; host pipeline wall %.2f s -> %.2f Gbases/s" % (
        tag, dt, bases / dt / 1e9, wall, bases / wall / 1e9))
    for l in r.stderr.splitlines():
        if l.startswith(("start-up:", "host pipeline:", "device thread", "input:")):
            print("      " + l)
    bound = "the reader (%s)" % ("BGZF inflate + record walk" if tag == "bam" else "FASTQ parsers") if parse >= dev else \
        "the device side (copies + kernels)"
    print("      busy: reader %.2f s, copies + kernels %.2f s -> bound by %s" % (parse, dev, bound))
    return js


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000, help="reads of the configs[2] batch (bench.py times 1 M; 200 k = 1.8 Gbases)")
    ap.add_argument("--dir", default="/tmp/bam_e2e")
    ap.add_argument("--procs", type=int, default=16, help="BAM writer processes (at most 16)")
    ap.add_argument("--keep", action="store_true", help="keep the inputs")
    ap.add_argument("--generate", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    if a.generate:
        generate(a.dir, a.reads)
        return
    t0 = time.perf_counter()
    subprocess.run([sys.executable, os.path.abspath(__file__), "--generate", "--reads", str(a.reads), "--dir", a.dir], check=True,
                   timeout=900)
    seq = np.load(os.path.join(a.dir, "seq.npy"), mmap_mode="r")
    qual = np.load(os.path.join(a.dir, "qual.npy"), mmap_mode="r")
    off = np.load(os.path.join(a.dir, "off.npy"))
    n, bases = len(off) - 1, int(off[-1])
    fq, bam = os.path.join(a.dir, "twin.fq"), os.path.join(a.dir, "reads.bam")
    H = C.CDLL(build.HOST_LIB)
    H.fplh_write_fastq.restype = C.c_int
    H.fplh_write_fastq.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_int]
    s, q = np.ascontiguousarray(seq), np.ascontiguousarray(qual)
    if H.fplh_write_fastq(fq.encode(), s.ctypes.data, q.ctypes.data, off.ctypes.data, n, b"r", 16) != 0:
        raise SystemExit("writing the FASTQ twin failed")
    t1 = time.perf_counter()
    write_bam(bam, s, q, off, a.procs)
    t2 = time.perf_counter()
    print("configs[2] reads: %d, %.2f Gbases; FASTQ twin %.2f GB (%.2f B/base), BAM %.2f GB (%.2f B/base, level 1, written in %.1f s); "
          "inputs ready after %.1f s" % (n, bases / 1e9, os.path.getsize(fq) / 1e9, os.path.getsize(fq) / bases, os.path.getsize(bam) / 1e9,
                                        os.path.getsize(bam) / bases, t2 - t1, t2 - t0))
    reports = {}
    for tag, inp in (("fastq", fq), ("bam", bam)):
        subprocess.run(["cat", inp], stdout=subprocess.DEVNULL, check=True)  # (both from the page cache)
        js = run_cli(inp, a.dir, tag, bases)
        reports[tag] = [l for l in open(js, "rb").read().split(b"\n") if not l.startswith(b'\t"command":')]
    same = reports["bam"] == reports["fastq"]
    print("fastplong.json of the BAM run %s that of its FASTQ twin" % ("equals" if same else "DIFFERS from"))
    if not a.keep:
        for p in (fq, bam, "seq.npy", "qual.npy", "off.npy"):
            p = p if os.path.isabs(p) else os.path.join(a.dir, p)
            if os.path.exists(p):
                os.unlink(p)
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
