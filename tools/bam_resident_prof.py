"""usage: python tools/bam_resident_prof.py --bam FILE [--out profiles/bam_resident] [--windows 32,256] [--runs 3]
The resident BAM path (fpl_process_bgzf_bam_async: inflate, record walk, decode and the per-read kernels chained on the device)
on tools/bam_e2e.py's input (`python tools/bam_e2e.py --keep` leaves it as DIR/in.bam).  Two measurements, raw lines into --out:

  kernels   for every window size, a child of this process under `rocprofv3 --kernel-trace --stats` (a run of its own, the
            program after `--`) submits windows of that many MB of inflated bytes; from the ONE trace: the time of
            k_bgzf_inflate, of the five walk kernels (k_bam_place_tail, k_bam_find, k_bam_walk_seg, k_bam_chain, k_bam_compact)
            and of k_bam_decode per window.  The figure that decides whether the serial chain matters is the walk's time
            against the upload time of the same window's compressed bytes.  The trace holds kernels only, so the latter is NOT
            from it: the child times, on the host, a copy of the first window's payloads to the device through torch, with the
            copy alone on the device.  torch takes the source for pageable memory, so the figure is an upper bound on what the
            library's own upload from page-locked memory takes.
  wall      the whole file through submit_bgzf ... wait three deep, against the same file through fplh_bam_read_all (BamReader,
            the host's inflate) + submit_bam; --runs runs each, records compared once.

No threshold is set on any of it in advance.  This process never opens the GPU itself."""
import argparse
import csv
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastplong_amd import abi, bgzf, build  # noqa: E402

KERNELS = ["k_bgzf_inflate", "k_bam_place_tail", "k_bam_find", "k_bam_walk_seg", "k_bam_chain", "k_bam_compact", "k_bam_decode"]
OPTS = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
START, END = "AAGGATTCATTCCCACGGTAACAC", "GTGTTACCGTGGGAATGAATCCTT"


def stretches(data, window):
    """file offsets that cut the file into stretches of about `window` inflated bytes, each of whole blocks"""
    blk, offs = bgzf.blocks(data)
    cuts, acc = [0], 0
    for i in range(len(blk)):
        acc += int(blk["isize"][i])
        if acc >= window and i + 1 < len(blk):
            cuts.append(offs[i + 1])
            acc = 0
    return cuts + [len(data)]


def resident(eng, data, window, want_reads, deep=abi.FPL_MAX_IN_FLIGHT, pool=None):
    """-> (records of the whole file, seconds, rewalked, segments).  pool: a list that keeps the page-locked output pairs from one
    call to the next, so that only the first run allocates them"""
    pool = [] if pool is None else pool

    def collect(batch):
        if not want_reads:
            return batch.wait(False)[:2]
        need = batch.peek()["n_bases"]
        pair = pool.pop() if pool else None
        if pair is None or len(pair[0]) < need:
            pair = (eng.pinned_array(need + need // 4 + 1, keep=False), eng.pinned_array(need + need // 4 + 1, keep=False))
        out = batch.wait(True, pair[0], pair[1])[:2]
        pool.append(pair)  # (nothing here reads the decoded arrays: the pair is free again)
        return out

    cuts = stretches(data, window)
    parts = []
    for k in range(len(cuts) - 1):
        blk, _ = bgzf.blocks(data, cuts[k], cuts[k + 1])
        comp = eng.pinned_array(cuts[k + 1] - cuts[k])
        comp[:] = np.frombuffer(data, np.uint8, cuts[k + 1] - cuts[k], cuts[k])
        parts.append((comp, blk))
    eng.set_bam_tail(b"")
    eng.reset_counters()
    pending, res, rew, seg = [], [], 0, 0
    t0 = time.perf_counter()
    for k, (comp, blk) in enumerate(parts):
        pending.append(eng.submit_bgzf(comp, blk, skip=bgzf.header_len(data) if k == 0 else 0))
        if len(pending) == deep:
            h, r = collect(pending.pop(0))
            if h["status"] != abi.FPL_BAMW_OK:
                raise SystemExit("refused: %r" % h)
            res.append(r), (rew := rew + h["rewalked"]), (seg := seg + h["segments"])
    while pending:
        h, r = collect(pending.pop(0))
        if h["status"] != abi.FPL_BAMW_OK:
            raise SystemExit("refused: %r" % h)
        res.append(r), (rew := rew + h["rewalked"]), (seg := seg + h["segments"])
    return np.concatenate(res), time.perf_counter() - t0, rew, seg


def host_path(eng, path, chunk):
    """the same file through BamReader (host inflate and walk) + submit_bam, batch by batch -> (records, seconds)"""
    build.build_host()
    L = C.CDLL(build.HOST_LIB)
    L.fplh_bam_read_all.restype = C.c_void_p
    L.fplh_bam_read_all.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64]
    for f in ("fplh_bam_all_bytes", "fplh_bam_all_rec", "fplh_bam_all_off"):
        getattr(L, f).restype = C.c_void_p
    L.fplh_bam_all_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fplh_bam_all_rec.argtypes = L.fplh_bam_all_off.argtypes = [C.c_void_p]
    L.fplh_bam_all_n.restype = C.c_uint32
    L.fplh_bam_all_n.argtypes = L.fplh_bam_all_free.argtypes = [C.c_void_p]
    eng.reset_counters()
    t0 = time.perf_counter()
    h = L.fplh_bam_read_all(path.encode(), chunk, 0, 0)
    n = L.fplh_bam_all_n(h)
    nb = C.c_uint64()
    raw = np.ctypeslib.as_array(C.cast(L.fplh_bam_all_bytes(h, C.byref(nb)), C.POINTER(C.c_uint8)), (nb.value,))
    rec = np.ctypeslib.as_array(C.cast(L.fplh_bam_all_rec(h), C.POINTER(C.c_uint64)), (n,))
    off = np.ctypeslib.as_array(C.cast(L.fplh_bam_all_off(h), C.POINTER(C.c_uint64)), (n + 1,))
    t_read = time.perf_counter() - t0
    res = np.zeros(n, abi.RESULT_DTYPE)
    so, qo = eng.pinned_array(int(off[-1]) + 1), eng.pinned_array(int(off[-1]) + 1)
    per = max(1, int(n * chunk // max(int(nb.value), 1)))
    inflight = 0
    for a in range(0, n, per):
        b = min(n, a + per)
        eng.submit_bam(raw, np.ascontiguousarray(rec[a:b]), np.ascontiguousarray(off[a:b + 1]), so, qo, res[a:b])
        inflight += 1
        if inflight == abi.FPL_MAX_IN_FLIGHT:
            eng.wait()
            inflight -= 1
    while inflight:
        eng.wait()
        inflight -= 1
    dt = time.perf_counter() - t0
    out = res.copy()
    L.fplh_bam_all_free(h)
    return out, dt, t_read


def child(a):
    """(under rocprofv3) windows of a.window_mb MB through the resident path; prints the upload time of a window's payloads"""
    import torch

    from fastplong_amd import engine

    data = open(a.bam, "rb").read()
    eng = engine.Engine(abi.FplOptions.default(**OPTS), START, END, device=0, max_cycles=1 << 16)
    _, dt, rew, seg = resident(eng, data, a.window_mb << 20, False)
    cuts = stretches(data, a.window_mb << 20)
    n = cuts[1] - cuts[0]
    src = eng.pinned_array(n)
    src[:] = np.frombuffer(data, np.uint8, n, cuts[0])
    dst = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(torch.from_numpy(src), non_blocking=True)
        torch.cuda.synchronize()
        up = time.perf_counter() - t0
    print("window %d MB: %d stretches, first stretch %d compressed bytes copied up in %.1f us (%.1f GB/s; host-timed, through torch); %d segments, %d walked again; "
          "%.3f s wall stats-only" % (a.window_mb, len(cuts) - 1, n, up * 1e6, n / up / 1e9, seg, rew, dt), flush=True)
    eng.close()


def kernels(a, mb, out):
    d = os.path.join(out, "trace_%dmb" % mb)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "walk", "--", sys.executable, os.path.abspath(__file__),
           "--bam", a.bam, "--child", "--window-mb", str(mb)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200)
    lines = [l for l in p.stdout.splitlines() if l.startswith("window ")]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout[-3000:])
        raise SystemExit("the profiled run failed (rc %d)" % p.returncode)
    stats = sorted(os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv"))
    if not stats:
        raise SystemExit("no kernel stats file under %s" % d)
    rows = {k: None for k in KERNELS}
    for row in csv.DictReader(open(stats[-1])):
        for k in KERNELS:
            if row["Name"].startswith(k) or (" " + k + "(") in row["Name"] or row["Name"].split("(")[0].endswith(k):
                rows[k] = row
    with open(os.path.join(out, "kernels_%dmb.txt" % mb), "w") as f:
        for l in lines:
            print(l), f.write(l + "\n")
        walk = 0.0
        for k in KERNELS:
            r = rows[k]
            if r is None:
                raise SystemExit("%s is not in %s" % (k, stats[-1]))
            l = "%-18s %s calls, average %.1f us, fastest %.1f us, slowest %.1f us" % (k, r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                    float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
            print(l), f.write(l + "\n")
            if k.startswith("k_bam_") and k != "k_bam_decode":
                walk += float(r["AverageNs"]) / 1e3
        l = "the five walk kernels together: %.1f us per window on average (compare with the host-timed copy above)" % walk
        print(l), f.write(l + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_resident"))
    ap.add_argument("--windows", default="32,256")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--window-mb", type=int, default=32, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.wall:  # (a child of its own as well: this process stays off the GPU)
        from fastplong_amd import engine

        data = open(a.bam, "rb").read()
        eng = engine.Engine(abi.FplOptions.default(**OPTS), START, END, device=0, max_cycles=1 << 16)
        ref, pool = None, []
        for k in range(a.runs):
            r, dt, rew, seg = resident(eng, data, a.window_mb << 20, True, pool=pool)
            cnt = eng.counters()
            print("resident %d: %.3f s wall, %d reads, %d segments, %d walked again" % (k, dt, len(r), seg, rew), flush=True)
            h, dth, t_read = host_path(eng, a.bam, a.window_mb << 20)
            print("host path %d: %.3f s wall (%.3f s of it BamReader: inflate + walk), %d reads" % (k, dth, t_read, len(h)), flush=True)
            if ref is None:
                ref = h
                if r.tobytes() != h.tobytes() or not np.array_equal(cnt, eng.counters()):
                    raise SystemExit("the two paths disagree")
        eng.close()
        return
    os.makedirs(a.out, exist_ok=True)
    for mb in [int(x) for x in a.windows.split(",")]:
        kernels(a, mb, a.out)
    for mb in [int(x) for x in a.windows.split(",")]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--bam", a.bam, "--wall", "--window-mb", str(mb), "--runs", str(a.runs)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        sys.stdout.write(p.stdout)
        open(os.path.join(a.out, "wall_%dmb.txt" % mb), "w").write(p.stdout)
        if p.returncode != 0:
            raise SystemExit("the wall-time run failed (rc %d)" % p.returncode)


if __name__ == "__main__":
    main()
