"""usage: python tools/gzip_inflate_e2e.py [--reads N] [--dir DIR] [--runs K]
A one-member .fastq.gz inflated on the device against the host's inflate, end to end on one MI355X (README "gzip input"): the
configs[2] reads of tools/bam_e2e.py as FASTQ, gzipped as ONE member at -6, through `-i reads.fastq.gz -o OUT -V` with and without
--device_inflate, K whole-process runs each, interleaved.  Per run one raw line: wall time, Gbases/s, the host pipeline's own
line and the input lines; per form the MD5 of its first output, which must be equal.  This process never opens the GPU."""
import argparse
import hashlib
import os
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bam_e2e  # noqa: E402
from fastplong_amd import build, synth  # noqa: E402

FORMS = [("host", []), ("device", ["--device_inflate"])]


def md5_of(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def write_member(path, seq, qual, off, step=20000):
    """the reads as FASTQ text through ONE zlib stream at level 6"""
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "wb") as f:
        for i in range(0, len(off) - 1, step):
            j = min(len(off) - 1, i + step)
            a, b = int(off[i]), int(off[j])
            piece = synth.to_fastq(seq[a:b], qual[a:b], off[i:j + 1] - off[i], prefix="r%d_" % i)
            f.write(c.compress(piece))
        f.write(c.flush())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--dir", default="/tmp/gzip_inflate_e2e")
    ap.add_argument("--out", default="/dev/shm/gzip_inflate_e2e.out.fq")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--keep", action="store_true", help="keep the inputs and the last output")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bam_e2e.py"), "--generate", "--reads", str(a.reads), "--dir", a.dir],
                   check=True, timeout=900)
    seq = np.ascontiguousarray(np.load(os.path.join(a.dir, "seq.npy"), mmap_mode="r"))
    qual = np.ascontiguousarray(np.load(os.path.join(a.dir, "qual.npy"), mmap_mode="r"))
    off = np.load(os.path.join(a.dir, "off.npy"))
    bases = int(off[-1])
    gz = os.path.join(a.dir, "reads.fastq.gz")
    write_member(gz, seq, qual, off)
    print("input: %d reads, %.3f Gbases, one gzip member of %.2f GB" % (len(off) - 1, bases / 1e9, os.path.getsize(gz) / 1e9), flush=True)
    subprocess.run(["cat", gz], stdout=subprocess.DEVNULL, check=True)  # (from the page cache)
    md5 = {}
    for r in range(a.runs):
        for tag, extra in FORMS:  # (interleaved: a drift of the machine hits both forms alike)
            cmd = [build.CLI, "-i", gz, "-o", a.out, "-j", os.path.join(a.dir, tag + ".json"), "-h", os.path.join(a.dir, tag + ".html"),
                   "-V"] + bam_e2e.FLAGS + extra
            t0 = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                raise SystemExit("%s failed (rc %d):\n%s" % (tag, p.returncode, p.stderr[-3000:]))
            print("%-6s run %d: whole process %.3f s -> %.3f Gbases/s" % (tag, r, dt, bases / dt / 1e9))
            for l in p.stderr.splitlines():
                if l.startswith(("host pipeline:", "input: gzip")):
                    print("          " + l)
            if tag not in md5:
                md5[tag] = md5_of(a.out)
                print("          md5 of the output: %s" % md5[tag], flush=True)
    if len(set(md5.values())) != 1:
        raise SystemExit("the outputs DIFFER: %r" % md5)
    print("the outputs are identical across forms")
    if a.keep:
        return
    for p in (a.out, gz, os.path.join(a.dir, "seq.npy"), os.path.join(a.dir, "qual.npy"), os.path.join(a.dir, "off.npy")):
        if os.path.exists(p):
            os.unlink(p)


if __name__ == "__main__":
    main()
