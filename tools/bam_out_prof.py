"""The BAM record kernels (k_bamout_layout / k_bamout_compose, fastplong_amd/csrc/bam_emit.h) and the BGZF block kernels behind them
on one resident text batch, for `rocprofv3 --kernel-trace --stats -- python tools/bam_out_prof.py [Mbases] [--bam]`: reads of 10 kb
with ONT-like qualities, every read passing whole, submitted three times through Engine.submit_text(gzip=True).  Without --bam
the batch is the BGZF FASTQ form (Engine.set_gzip_framing: k_gz_layout / k_gz_compose), the form to compare with IN THE SAME
SESSION; with it the records' form (Engine.set_gzip_records).

Bytes k_bamout_compose moves per base: 2 read (base, quality), 1.5 written = 3.5; the roofline printed is that count at 8 TB/s,
next to the whole design's (compose as above, k_gz_block_bgzf reads the 1.5 and writes the coded block, k_gz_compact reads and
writes that again).  The wall time printed holds the upload, the parse, the per-read kernels and the bytes' way back as well."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, bgzf, engine  # noqa: E402


def main(mbases=1000, L=10_000, bam=False):
    rng = np.random.default_rng(1)
    n = max(1, mbases * 1_000_000 // L)
    pool = 64  # distinct reads; the kernels do not care that reads repeat
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes() for _ in range(pool)]
    quals = [(np.clip(rng.normal(18, 8, L), 1, 60).astype(np.uint8) + 33).tobytes() for _ in range(pool)]
    text = b"".join(b"@read%d runid=abc ch=%d\n%s\n+\n%s\n" % (i, i % 512, seqs[i % pool], quals[i % pool]) for i in range(n))
    eng = engine.Engine(abi.FplOptions.default(adapter_enabled=0, qual_filter=0, length_filter=0), "", "", device=0, max_cycles=L)
    if bam:
        eng.set_gzip_records(True)
    else:
        eng.set_gzip_framing(True)
    buf = eng.pinned_array(len(text))
    buf[:] = np.frombuffer(text, np.uint8)
    for k in range(3):
        t0 = time.time()
        eng.submit_text(buf, gzip=True)
        info, res, lines, out = eng.wait_text()
        dt = time.time() - t0
        print("batch %d: %.3f s wall, %d reads, %.3f Gbases, text %d bytes -> %s in BGZF blocks: %d bytes (%.3f of the text)" % (
            k, dt, info["n_reads"], info["n_bases"] / 1e9, len(text), "BAM records" if bam else "FASTQ", len(out), len(out) / len(text)))
    composed, pos = 0, 0
    while pos < len(out):  # block after block: ISIZE says what went in (the tests inflate; 0.9 GB here would take minutes)
        size = bgzf.block_len(out, pos)
        composed += int.from_bytes(out[pos + size - 4:pos + size], "little")
        pos += size
    n_bases = n * L
    print("composed: %d bytes in front of the block kernels (%.3f per base)" % (composed, composed / n_bases))
    if bam:
        print("k_bamout_compose moves 3.5 bytes a base: at 8 TB/s %.3f ms" % (3.5 * n_bases / 8e12 * 1e3))
        moved = 2 * n_bases + 2 * composed + 4 * len(out)
    else:
        moved = 3 * composed + 4 * len(out)
    print("bytes the design moves: %.2f per base; at 8 TB/s: %.3f ms" % (moved / n_bases, moved / 8e12 * 1e3))
    eng.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--bam"]
    main(*(int(a) for a in args[:1]), bam="--bam" in sys.argv[1:])
