"""The fragment forms of the device's gzip output (k_frag_count / k_frag_first / k_frag_place, fastplong_amd/csrc/frag_index.h;
k_gz_layout_frag / k_gz_compose_frag, csrc/gz_emit.h) on the resident text batch of tools/gz_emit_prof.py, for
`rocprofv3 --kernel-trace --stats -- python tools/frag_out_prof.py [Mbases] [--plain]` in a run of its own, without counters.

Default: --break and --mask on (windows 100 / 50, quality 10), fpl_set_fragment_output on; about a quarter of the reads carry one
stretch of low quality and break there.  --plain: the same reads with both options off -- k_gz_layout / k_gz_compose of the same
session for comparison.  Take three processes of each form, alternating; the kernel table then gives the index, the layout and
the compose of the fragment form beside the record form's, and k_gz_block (the bulk of either) for scale.  The wall time printed
holds the upload, the parse, the per-read kernels and the member's way back as well."""
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, engine  # noqa: E402


def main(mbases=1000, L=10_000, plain=False):
    rng = np.random.default_rng(1)
    n = max(1, mbases * 1_000_000 // L)
    pool = 64  # distinct reads; the kernels do not care that reads repeat
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes() for _ in range(pool)]
    quals = []
    for i in range(pool):
        q = np.clip(rng.normal(30, 4, L), 20, 60).astype(np.uint8) + 33
        if i % 4 == 0:  # a quarter of the reads: one stretch far below the thresholds
            a = int(rng.integers(1000, L - 1500))
            q[a:a + 300] = 35
        quals.append(q.tobytes())
    text = b"".join(b"@read%d runid=abc ch=%d\n%s\n+\n%s\n" % (i, i % 512, seqs[i % pool], quals[i % pool]) for i in range(n))
    okw = dict(adapter_enabled=0, qual_filter=0, length_filter=0)
    if not plain:
        okw.update(break_enabled=1, break_window=100, break_quality=10, mask_enabled=1, mask_window=50, mask_quality=10)
    eng = engine.Engine(abi.FplOptions.default(**okw), "", "", device=0, max_cycles=L)
    if not plain:
        eng.set_fragment_output(True)
    buf = eng.pinned_array(len(text))
    buf[:] = np.frombuffer(text, np.uint8)
    for k in range(3):
        t0 = time.time()
        eng.submit_text(buf, gzip=True)
        info, res, lines, member = eng.wait_text()
        dt = time.time() - t0
        print("%s batch %d: %.3f s wall, %d reads, %.3f Gbases, text %d bytes -> member %d bytes" % (
            "plain" if plain else "fragment", k, dt, info["n_reads"], info["n_bases"] / 1e9, len(text), len(member)))
    if not plain:
        frags, regs = eng.fragments()
        print("fragments: %d of %d reads (%d with a break_no, %d passing), regions: %d" % (
            len(frags), info["n_reads"], int((frags["break_no"] > 0).sum()), int((frags["code"] == 0).sum()), len(regs)))
    d = zlib.decompressobj(31)
    out = d.decompress(member) + d.flush()
    assert d.eof and d.unused_data == b""
    print("inflated: %d bytes, CRC-32 %08x" % (len(out), zlib.crc32(out)))
    eng.close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--plain"]
    main(*(int(a) for a in args[:1]), plain="--plain" in sys.argv[1:])
