"""The gzip kernels (k_gz_layout / k_gz_compose / k_gz_block / k_gz_finish / k_gz_compact, fastplong_amd/csrc/gz_emit.h) on one
resident text batch, for `rocprofv3 --kernel-trace --stats -- python tools/gz_emit_prof.py [Mbases] [--bgzf]`: reads of 10 kb with
ONT-like qualities, every read passing whole, submitted three times through Engine.submit_text(gzip=True).  --bgzf: the BGZF
framing (Engine.set_gzip_framing: k_gz_block_bgzf / k_gz_finish_bgzf / k_gz_frame in place of k_gz_block / k_gz_finish).

Bytes the design moves per byte of output text (n): compose reads n and writes n; k_gz_block reads n and writes the coded block
(about 0.46 n); k_gz_compact reads and writes that again: 3 n + 4 * 0.46 n = 4.8 n, i.e. 9.7 bytes per base (two text bytes a
base).  The roofline printed is that count at 8 TB/s.  The wall time printed holds the upload, the parse, the per-read kernels and
the member's way back as well."""
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, engine  # noqa: E402


def main(mbases=1000, L=10_000, bgzf=False):
    rng = np.random.default_rng(1)
    n = max(1, mbases * 1_000_000 // L)
    pool = 64  # distinct reads; the kernels do not care that reads repeat
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes() for _ in range(pool)]
    quals = [(np.clip(rng.normal(18, 8, L), 1, 60).astype(np.uint8) + 33).tobytes() for _ in range(pool)]
    text = b"".join(b"@read%d runid=abc ch=%d\n%s\n+\n%s\n" % (i, i % 512, seqs[i % pool], quals[i % pool]) for i in range(n))
    eng = engine.Engine(abi.FplOptions.default(adapter_enabled=0, qual_filter=0, length_filter=0), "", "", device=0, max_cycles=L)
    if bgzf:
        eng.set_gzip_framing(True)
    buf = eng.pinned_array(len(text))
    buf[:] = np.frombuffer(text, np.uint8)
    for k in range(3):
        t0 = time.time()
        eng.submit_text(buf, gzip=True)
        info, res, lines, member = eng.wait_text()
        dt = time.time() - t0
        print("batch %d: %.3f s wall, %d reads, %.3f Gbases, text %d bytes -> %s %d bytes (%.3f of the text)" % (
            k, dt, info["n_reads"], info["n_bases"] / 1e9, len(text), "BGZF blocks" if bgzf else "member", len(member), len(member) / len(text)))
    if len(text) <= 300_000_000:
        got, rest = [], member
        while rest:  # one member, or block after block
            d = zlib.decompressobj(31)
            got.append(d.decompress(rest) + d.flush())
            assert d.eof
            rest = d.unused_data
        assert b"".join(got) == text, "the output does not inflate to the text"
        print("inflated and compared: equal (%d gzip members)" % len(got))
    moved = 3 * len(text) + 4 * len(member)
    print("bytes the design moves: %.2f per output byte; at 8 TB/s: %.3f ms" % (moved / len(text), moved / 8e12 * 1e3))
    eng.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--bgzf"]
    main(*(int(a) for a in args[:1]), bgzf="--bgzf" in sys.argv[1:])
