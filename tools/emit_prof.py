"""fpl_emit_batch_device (fastplong_amd/csrc/emit.h) against a plain copy of the same bytes, in ONE process and session: the
configs[2] batch (bench.py's c3_full_pipeline: synth.device_batch, 1 M reads unless --reads says otherwise) made resident and
processed once, then HIP-event times of the emit call (layout + gather) over --reps repetitions and of two device-to-device
torch.Tensor.copy_ of info.n_bytes bytes each -- the traffic of the gather, 2 bytes read and 2 written per passing base, with
nothing to find.  The figure of merit is emit time / copy time.

    python tools/emit_prof.py [--reads N] [--reps K] [--out profiles/emit/emit_prof.txt]
    rocprofv3 --kernel-trace --stats -- python tools/emit_prof.py --reads N      # the four kernels one by one
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, engine, synth  # noqa: E402

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)


def timed(fn, reps):
    """-> the milliseconds of each of `reps` runs of fn(), between HIP events on the current stream"""
    import torch

    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000, help="reads of the batch (the bench's: 1 000 000)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = args.reads
    seq_t, qual_t, off_t, max_len = synth.device_batch(n, seed=1, median_len=8000, sigma_len=0.5)
    eng = engine.Engine(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER, device=0, max_cycles=max_len)
    rt = eng.process_device(seq_t, qual_t, off_t, max_len)
    torch.cuda.synchronize()
    say("batch: %d reads, %d bases (synth.device_batch seed 1, median 8000, sigma 0.5), c3_full_pipeline options, processed once%s" % (
        n, seq_t.numel(), "" if n == 1_000_000 else "  [NOT the bench's 1 000 000 reads]"))
    out = eng.emit_device(seq_t, qual_t, off_t, rt)
    info = eng.emit_info(out[5])
    say("emit: %d output reads, %d bytes (%.1f %% of the input), longest %d, status %d" % (
        info["n_out"], info["n_bytes"], 100.0 * info["n_bytes"] / seq_t.numel(), info["max_len"], info["status"]))
    so, qo, oo, src, kind, _ = out
    nb = info["n_bytes"]

    def emit():
        eng.emit_device(seq_t, qual_t, off_t, rt, seq_out=so, qual_out=qo, off_out=oo, src=src, kind=kind)

    c1, c2 = torch.empty(nb, dtype=torch.uint8, device="cuda"), torch.empty(nb, dtype=torch.uint8, device="cuda")

    def copy():
        c1.copy_(seq_t[:nb])
        c2.copy_(qual_t[:nb])

    timed(emit, 2), timed(copy, 2)  # warm-up: workspace, first launches
    te, tc = timed(emit, args.reps), timed(copy, args.reps)
    for name, t in (("fpl_emit_batch_device", te), ("2 x copy_ of n_bytes", tc)):
        say("%-24s ms per call: %s" % (name, " ".join("%.3f" % x for x in t)))
    me, mc = float(np.median(te)), float(np.median(tc))
    moved = 4.0 * nb  # 2 bytes read and 2 written per passing base
    say("median: emit %.3f ms = %.2f TB/s of gathered traffic (%.1f %% of the 8 TB/s roofline), copy %.3f ms = %.2f TB/s" % (
        me, moved / me / 1e9, 100.0 * moved / me / 1e9 / 8.0, mc, moved / mc / 1e9))
    say("emit / copy = %.2f" % (me / mc))
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
