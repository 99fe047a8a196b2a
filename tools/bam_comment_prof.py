"""The comment kernels (k_bam_comment_tags, k_bam_comment_len, k_gz_layout_bam_comments, k_gz_compose_bam_comments,
fastplong_amd/csrc/bam_comments.h) and the gzip block kernels behind them on one resident BAM batch, for
`rocprofv3 --kernel-trace --stats -- python tools/bam_comment_prof.py off|mods|all [Mbases]`.

The batch is the one of `tools/bam_out_prof.py --mods`: ONT-like reads with adapters (median 5 kb, a middle adapter in three of
ten) that carry generated modification calls -- C+mh? at CpGs, A+a. at every fourth A, a sparse N+n group --, submitted three times
through Engine.submit_bam(gzip=True) in the FASTQ gzip form: without the switch (`off`: k_gz_layout_bam / k_gz_compose_bam, the
form to compare with IN THE SAME SESSION), with set_bam_comments(["MM", "ML"]) (`mods`) or with set_bam_comments("*") (`all`)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, engine, synth  # noqa: E402

SELECTIONS = {"off": None, "mods": ["MM", "ML"], "all": "*"}


def main(what="all", mbases=100):
    from tests import bam_mod_cases as mc
    from tests import bamio, hostio
    L = 5000
    pool = 256  # distinct reads: generating the calls in Python is the slow part; the kernels do not care that reads repeat
    rng = np.random.default_rng(2)
    seq, qual, off = synth.ont_like(pool, seed=3, median_len=L, p_middle=0.3)
    encoded = []
    for i, (_, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        occ = mc.occurrences(codes, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(codes) and codes[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(codes, b"A", 4, 3)),
                (b"N+n", mc.every(codes, b"N", 997, 11))]
        encoded.append((len(codes), bamio.encode_record(b"read%d" % i, 4, codes, q, tags=mc.fields_of(codes, spec, rng))))
    n = max(1, mbases * 1_000_000 // L)
    raw, starts, offs = bytearray(), [], [0]
    for i in range(n):
        starts.append(len(raw))
        offs.append(offs[-1] + encoded[i % pool][0])
        raw += encoded[i % pool][1]
    starts, offs = np.array(starts, np.uint64), np.array(offs, np.uint64)
    eng = engine.Engine(abi.FplOptions.default(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5), synth.START_ADAPTER,
                        synth.END_ADAPTER, device=0, max_cycles=int(max(e[0] for e in encoded)) + 64)
    eng.set_bam_comments(SELECTIONS[what])
    buf = eng.pinned_array(len(raw))
    buf[:] = np.frombuffer(bytes(raw), np.uint8)
    res = np.zeros(n, abi.RESULT_DTYPE)
    for k in range(3):
        t0 = time.time()
        eng.submit_bam(buf, starts, offs, res=res, gzip=True)
        out = eng.wait()
        print("batch %d (comments: %s): %.3f s wall, %d records of %d bytes, %.3f Gbases -> a gzip member of %d bytes; %d split reads" % (
            k, what, time.time() - t0, n, len(raw), int(offs[-1]) / 1e9, len(out), int((res["n_frag"] == 2).sum())))
    print("comment counts (records, fields, bytes, left out), three batches: %s" % (eng.bam_comment_stats(),))
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    main(args[0] if args else "all", *(int(a) for a in args[1:2]))
