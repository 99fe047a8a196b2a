"""usage: python tools/bgzf_inflate_prof.py --profile DIR [--blocks N]
The BGZF inflate kernel (k_bgzf_inflate, fastplong_amd/csrc/bgzf_inflate.h) on a set of level-1 blocks of BAM-like data: N blocks
(default 4096, 16 distinct payloads of 65 280 bytes, what a BAM writer cuts) through fpl_inflate_bgzf three times.
With --profile this process -- which never opens the GPU -- starts `rocprofv3 --kernel-trace --stats --output-format csv -d DIR
-o bgzf -- python tools/bgzf_inflate_prof.py --blocks N` as a child in a run of its own, reads k_bgzf_inflate's row out of the
kernel stats file rocprofv3 writes, and prints the KERNEL's GB/s of inflated bytes (fastest and average call).  Without it the
tool is that child: it prints the whole call's wall time and GB/s, copies included; every status must be 0 and one block of
each payload is compared with zlib."""
import argparse
import csv
import os
import subprocess
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, engine  # noqa: E402


def bam_like(n, seed):
    """packed 4-bit bases, then qualities with a skewed distribution, record after record"""
    r = np.random.RandomState(seed)
    out = bytearray()
    while len(out) < n:
        l = int(r.randint(2000, 20000))
        nib = r.choice(np.array([1, 2, 4, 8], np.uint8), size=l + (l & 1))
        out += bytes(36) + b"read_%08x\0" % int(r.randint(0, 1 << 30)) + ((nib[0::2] << 4) | nib[1::2]).tobytes()
        out += np.clip(r.normal(30, 8, l), 2, 50).astype(np.uint8).tobytes()
    return bytes(out[:n])


def profile(d, n_blocks):
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bgzf", "--", sys.executable,
           os.path.abspath(__file__), "--blocks", str(n_blocks)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    sys.stdout.write(p.stdout[-3000:])
    if p.returncode != 0:
        raise SystemExit("the profiled run failed (rc %d)" % p.returncode)
    stats = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
    if not stats:
        raise SystemExit("no kernel stats file under %s" % d)
    total = 65280 * n_blocks
    for row in csv.DictReader(open(sorted(stats)[-1])):
        if "k_bgzf_inflate" in row["Name"]:
            print("k_bgzf_inflate: %s calls, fastest %.1f us, average %.1f us -> %.2f GB/s (fastest), %.2f GB/s (average) of inflated bytes, %d blocks"
                  % (row["Calls"], float(row["MinNs"]) / 1e3, float(row["AverageNs"]) / 1e3, total / float(row["MinNs"]),
                     total / float(row["AverageNs"]), n_blocks))
            return
    raise SystemExit("k_bgzf_inflate is not in %s" % stats[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--profile", metavar="DIR", help="run under rocprofv3 as a child and report the kernel's rate")
    a = ap.parse_args()
    if a.profile:
        return profile(a.profile, a.blocks)
    data = [bam_like(65280, 10 + k) for k in range(16)]
    comp = []
    for d in data:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        comp.append(c.compress(d) + c.flush())
    starts = np.cumsum([0] + [len(c) for c in comp])
    blocks = np.zeros(a.blocks, np.dtype(abi.BGZF_BLOCK_DTYPE))
    for i in range(a.blocks):
        k = i % 16
        blocks[i] = (starts[k], 65280 * i, len(comp[k]), 65280, zlib.crc32(data[k]), 1)
    cbuf = np.frombuffer(b"".join(comp), np.uint8)
    total = 65280 * a.blocks
    print("%d blocks, %.1f MB inflated, %.1f MB of payloads uploaded per call (16 distinct)" % (a.blocks, total / 1e6, len(cbuf) / 1e6))
    inf = engine.Inflater(0)
    out = np.zeros(total, np.uint8)
    for k in range(a.calls):
        t0 = time.perf_counter()
        _, status = inf.inflate(cbuf, blocks, out)
        dt = time.perf_counter() - t0
        if status.any():
            raise SystemExit("refused blocks: %r" % np.flatnonzero(status)[:10])
        print("fpl_inflate_bgzf %d: %.4f s wall -> %.2f GB/s of inflated bytes (copies included)" % (k, dt, total / dt / 1e9), flush=True)
    for k in range(16):
        i = a.blocks - 16 + k if a.blocks >= 16 else k
        if i < a.blocks and out[65280 * i:65280 * (i + 1)].tobytes() != data[i % 16]:
            raise SystemExit("block %d differs from zlib's bytes" % i)
    inf.close()


if __name__ == "__main__":
    main()
