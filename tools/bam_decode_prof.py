"""The BAM decode kernel (k_bam_decode, fastplong_amd/csrc/bam_decode.h) on a resident batch of >= 1 Gbases, for
`rocprofv3 --kernel-trace --stats -- python tools/bam_decode_prof.py`: 1000 reads of 1 Mb (both strands) decoded three times
through fpl_decode_bam.  The kernel moves 3.5 bytes per base (0.5 packed base + 1 quality read, 2 written); its roofline at
8 TB/s is 3.5 / 8e12 s per base.  Prints the whole call's wall time (copies included) for reference."""
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import engine  # noqa: E402


def main(n=1000, L=1_000_000):
    rng = np.random.default_rng(1)
    packed = rng.integers(0, 256, (L + 1) // 2, dtype=np.uint8).tobytes()
    qual = rng.integers(0, 60, L, dtype=np.uint8).tobytes()
    parts, starts, pos = [], [], 0
    for i in range(n):
        name = b"r%d\0" % i
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, 0x10 if i % 2 else 0, L, -1, -1, 0) + name + packed + qual
        rec = struct.pack("<I", len(body)) + body
        starts.append(pos)
        parts.append(rec)
        pos += len(rec)
    raw = np.frombuffer(b"".join(parts), np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    st = np.array(starts, np.uint64)
    for k in range(3):
        t0 = time.time()
        engine.decode_bam(0, raw, st, off)
        print("fpl_decode_bam %d: %.3f s wall for %.2f Gbases (copies included)" % (k, time.time() - t0, n * L / 1e9))
    print("roofline of the kernel alone at 8 TB/s: %.2f ms" % (n * L * 3.5 / 8e12 * 1e3))


if __name__ == "__main__":
    main()
