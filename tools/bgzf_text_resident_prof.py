"""usage: python tools/bgzf_text_resident_prof.py --fastq FILE [--out profiles/bgzf_text] [--levels 1,6] [--windows 32,256] [--runs 3]
The resident BGZF text path (fpl_process_bgzf_text_async: inflate, the cut at a record's end, the parse and the per-read kernels
chained on the device) on the configs[2] reads as FASTQ (`python tools/bam_e2e.py --keep` leaves them as DIR/twin.fq).  The text is
compressed here, at every level of --levels, into BGZF blocks of 65280 bytes by a pool of at most 16 processes.  For every level
and every window size (MB of TEXT per submission) three measurements, raw lines into --out:

  kernels    a child of this process under `rocprofv3 --kernel-trace --stats` (a run of its own, the program after `--`) submits
             the file window by window, stats only; from the ONE trace the time of k_bgzf_inflate and of every parse kernel
             (k_tw_place_tail, k_tw_count, k_text_scan, k_tw_fill, k_tw_records, k_text_offsets, k_tw_verdict, k_text_gather,
             k_tw_names) per call.
  resident   the wall time of submit_bgzf_text ... wait three deep over the whole file, --runs times.
  host       the same text through the host's inflate (zlib, one process: what a caller without the resident path does per
             window before it can submit) + submit_text, cut at record boundaries on the host, three deep, in the same session,
             --runs times; the records of the two paths are compared once.

No rate is promised and no threshold is set in advance: the per-wave decode rate of k_bgzf_inflate is unmeasured, and this path
rests on it.  State the numbers with the session's run-to-run spread (the --runs lines).  This process never opens the GPU itself."""
import argparse
import csv
import multiprocessing as mp
import os
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastplong_amd import abi, bgzf  # noqa: E402

KERNELS = ["k_bgzf_inflate", "k_tw_place_tail", "k_tw_count", "k_text_scan", "k_tw_fill", "k_tw_records", "k_text_offsets", "k_tw_verdict",
           "k_text_gather", "k_tw_names"]
OPTS = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)
START, END = "AAGGATTCATTCCCACGGTAACAC", "GTGTTACCGTGGGAATGAATCCTT"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


def _blocks(args):
    """(pool worker) text[a:b) of the file -> whole BGZF blocks"""
    path, a, b, level = args
    with open(path, "rb") as f:
        f.seek(a)
        data = f.read(b - a)
    out = []
    for p in range(0, len(data), BLOCK):
        d = data[p:p + BLOCK]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        cd = c.compress(d) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", 12 + 6 + len(cd) + 8 - 1) + cd +
                   struct.pack("<II", zlib.crc32(d) & 0xFFFFFFFF, len(d)))
    return b"".join(out)


def compress(path, level, procs=16):
    n = os.path.getsize(path)
    step = BLOCK * 256
    with mp.get_context("fork").Pool(max(1, min(procs, 16))) as pool:
        parts = pool.map(_blocks, [(path, a, min(n, a + step), level) for a in range(0, n, step)])
    return b"".join(parts) + EOF_BLOCK


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


def resident(eng, data, window, deep=abi.FPL_MAX_IN_FLIGHT):
    """-> (records of the whole file, seconds)"""
    cuts = stretches(data, window)
    parts = []
    for k in range(len(cuts) - 1):
        blk, _ = bgzf.blocks(data, cuts[k], cuts[k + 1])
        comp = eng.pinned_array(cuts[k + 1] - cuts[k])
        comp[:] = np.frombuffer(data, np.uint8, cuts[k + 1] - cuts[k], cuts[k])
        parts.append((comp, blk))
    eng.set_bam_tail(b"")
    eng.reset_counters()
    pending, res = [], []

    def collect():
        h, r = pending.pop(0).wait(False)[:2]
        if h["status"] != abi.FPL_TXTW_OK:
            raise SystemExit("refused: %r" % h)
        res.append(r)

    t0 = time.perf_counter()
    for comp, blk in parts:
        pending.append(eng.submit_bgzf_text(comp, blk))
        if len(pending) == deep:
            collect()
    while pending:
        collect()
    dt = time.perf_counter() - t0
    if eng.bam_tail():
        raise SystemExit("the file does not end with a line break")
    return np.concatenate(res), dt


def host_path(eng, data, window, deep=abi.FPL_MAX_IN_FLIGHT):
    """the same file: every stretch inflated with zlib, cut behind its last whole record on the host, submit_text -> (records,
    seconds, seconds of them in zlib)"""
    cuts = stretches(data, window)
    eng.reset_counters()
    res, inflight, carry, t_inf = [], 0, b"", 0.0
    bufs = [eng.pinned_array(int(window * 1.5) + (1 << 20)) for _ in range(deep + 1)]
    t0 = time.perf_counter()
    for k in range(len(cuts) - 1):
        t1 = time.perf_counter()
        _, offs = bgzf.blocks(data, cuts[k], cuts[k + 1])
        text = carry + b"".join(bgzf.inflate_block(data, o) for o in offs)
        t_inf += time.perf_counter() - t1
        nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
        cut = int(nl[4 * (len(nl) // 4) - 1]) + 1 if len(nl) >= 4 else 0
        carry = text[cut:]
        buf = bufs[k % len(bufs)]
        buf[:cut] = np.frombuffer(text, np.uint8, cut)
        eng.submit_text(buf[:cut])
        inflight += 1
        if inflight == deep:
            res.append(eng.wait_text()[1])
            inflight -= 1
    while inflight:
        res.append(eng.wait_text()[1])
        inflight -= 1
    return np.concatenate(res), time.perf_counter() - t0, t_inf


def new_engine():
    from fastplong_amd import engine

    return engine.Engine(abi.FplOptions.default(**OPTS), START, END, device=0, max_cycles=1 << 16)


def child(a):
    """(under rocprofv3) the file window by window through the resident path, stats only"""
    data = open(a.bgzf, "rb").read()
    eng = new_engine()
    r, dt = resident(eng, data, a.window_mb << 20)
    print("window %d MB: %d stretches, %d reads, %.3f s wall stats-only" % (a.window_mb, len(stretches(data, a.window_mb << 20)) - 1, len(r), dt),
          flush=True)
    eng.close()


def kernels(a, path, tag, mb, out):
    d = os.path.join(out, "trace_%s_%dmb" % (tag, mb))
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "walk", "--", sys.executable, os.path.abspath(__file__),
           "--fastq", a.fastq, "--bgzf", path, "--child", "--window-mb", str(mb)]
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
    with open(os.path.join(out, "kernels_%s_%dmb.txt" % (tag, mb)), "w") as f:
        for l in lines:
            print(l), f.write(l + "\n")
        parse = 0.0
        for k in KERNELS:
            r = rows[k]
            if r is None:
                raise SystemExit("%s is not in %s" % (k, stats[-1]))
            l = "%-16s %s calls, average %.1f us, fastest %.1f us, slowest %.1f us" % (k, r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                                  float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3)
            print(l), f.write(l + "\n")
            if k != "k_bgzf_inflate":
                parse += float(r["AverageNs"]) / 1e3 * (2 if k == "k_text_offsets" else 1)
        l = "the parse kernels together: %.1f us per window on average (k_text_offsets runs twice)" % parse
        print(l), f.write(l + "\n")


def wall(a):
    data = open(a.bgzf, "rb").read()
    eng = new_engine()
    ref = None
    for k in range(a.runs):
        r, dt = resident(eng, data, a.window_mb << 20)
        cnt = eng.counters()
        print("resident %d: %.3f s wall, %d reads" % (k, dt, len(r)), flush=True)
        h, dth, t_inf = host_path(eng, data, a.window_mb << 20)
        print("host inflate + submit_text %d: %.3f s wall (%.3f s of it zlib), %d reads" % (k, dth, t_inf, len(h)), flush=True)
        if ref is None:
            ref = h
            if r.tobytes() != h.tobytes() or not np.array_equal(cnt, eng.counters()):
                raise SystemExit("the two paths disagree")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fastq", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_text"))
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--windows", default="32,256")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--bgzf", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--wall", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--window-mb", type=int, default=32, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.wall:  # (a child of its own as well: this process stays off the GPU)
        return wall(a)
    os.makedirs(a.out, exist_ok=True)
    for level in [int(x) for x in a.levels.split(",")]:
        tag = "l%d" % level
        path = os.path.join(a.out, "reads_%s.fastq.gz" % tag)
        t0 = time.perf_counter()
        comp = compress(a.fastq, level)
        open(path, "wb").write(comp)
        print("level %d: %.2f GB of text -> %.2f GB of BGZF in %.1f s" % (level, os.path.getsize(a.fastq) / 1e9, len(comp) / 1e9, time.perf_counter() - t0),
              flush=True)
        del comp
        for mb in [int(x) for x in a.windows.split(",")]:
            kernels(a, path, tag, mb, a.out)
        for mb in [int(x) for x in a.windows.split(",")]:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fastq", a.fastq, "--bgzf", path, "--wall", "--window-mb", str(mb), "--runs",
                                str(a.runs)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
            sys.stdout.write(p.stdout)
            open(os.path.join(a.out, "wall_%s_%dmb.txt" % (tag, mb)), "w").write(p.stdout)
            if p.returncode != 0:
                raise SystemExit("the wall-time run failed (rc %d)" % p.returncode)
        os.unlink(path)


if __name__ == "__main__":
    main()
