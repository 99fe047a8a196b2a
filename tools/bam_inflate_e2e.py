"""usage: python tools/bam_inflate_e2e.py [--reads N] [--dir DIR] [--runs K] [--chunks 32,128,256]
BGZF inflate on the device against the host's, end to end on one MI355X (README "BAM input"): tools/bam_e2e.py's input (the
configs[2] reads as an unaligned BAM at BGZF level 1) through `-i reads.bam -o OUT -V` with and without --device_inflate, K whole
process runs each at every --chunk_mb, interleaved.  Per run one raw line: wall time, Gbases/s, the host pipeline's own line and
the inflater's line; per form and chunk size the MD5 of its first output, which must all be equal.  This process never opens the GPU."""
import argparse
import hashlib
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bam_e2e  # noqa: E402
from fastplong_amd import build  # noqa: E402

FORMS = [("host", []), ("device", ["--device_inflate"])]


def md5_of(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--dir", default="/tmp/bam_inflate_e2e")
    ap.add_argument("--out", default="/dev/shm/bam_inflate_e2e.out.fq")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunks", default="32,128,256")
    ap.add_argument("--keep", action="store_true", help="keep the inputs and the last output")
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bam_e2e.py"), "--generate", "--reads", str(a.reads), "--dir", a.dir],
                   check=True, timeout=900)
    seq = np.ascontiguousarray(np.load(os.path.join(a.dir, "seq.npy"), mmap_mode="r"))
    qual = np.ascontiguousarray(np.load(os.path.join(a.dir, "qual.npy"), mmap_mode="r"))
    off = np.load(os.path.join(a.dir, "off.npy"))
    bases = int(off[-1])
    bam = os.path.join(a.dir, "reads.bam")
    bam_e2e.write_bam(bam, seq, qual, off, 16)
    print("input: %d reads, %.3f Gbases, BAM %.2f GB" % (len(off) - 1, bases / 1e9, os.path.getsize(bam) / 1e9), flush=True)
    subprocess.run(["cat", bam], stdout=subprocess.DEVNULL, check=True)  # (from the page cache)
    md5 = {}
    for chunk in [int(c) for c in a.chunks.split(",")]:
        for r in range(a.runs):
            for tag, extra in FORMS:  # (interleaved: a drift of the machine hits both forms alike)
                cmd = [build.CLI, "-i", bam, "-o", a.out, "-j", os.path.join(a.dir, tag + ".json"), "-h", os.path.join(a.dir, tag + ".html"),
                       "-V", "--chunk_mb", str(chunk)] + bam_e2e.FLAGS + extra
                t0 = time.perf_counter()
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1800)
                dt = time.perf_counter() - t0
                if p.returncode != 0:
                    raise SystemExit("%s failed (rc %d):\n%s" % (tag, p.returncode, p.stderr[-3000:]))
                print("chunk_mb %-3d %-6s run %d: whole process %.3f s -> %.3f Gbases/s" % (chunk, tag, r, dt, bases / dt / 1e9))
                for l in p.stderr.splitlines():
                    if l.startswith(("host pipeline:", "input: BGZF")):
                        print("          " + l)
                if (tag, chunk) not in md5:
                    md5[(tag, chunk)] = md5_of(a.out)
                    print("          md5 of the output: %s" % md5[(tag, chunk)], flush=True)
    if len(set(md5.values())) != 1:
        raise SystemExit("the outputs DIFFER: %r" % md5)
    print("the outputs are identical across forms and chunk sizes")
    if a.keep:
        return
    for p in (a.out, bam, os.path.join(a.dir, "seq.npy"), os.path.join(a.dir, "qual.npy"), os.path.join(a.dir, "off.npy")):
        if os.path.exists(p):
            os.unlink(p)


if __name__ == "__main__":
    main()
