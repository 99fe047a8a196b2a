"""The CLI against the whole reference program (oracle/_ref/fastplong_ref, built by oracle.build() from the reference's own
sources): the inputs, the flag matrix and the comparison shared by tests/test_cli_vs_ref_binary_stub.py (the CLI on the
oracle-backed stub library) and tests/test_gpu_vs_ref_binary.py (the CLI on the real library)."""
import os
import re
import subprocess

import numpy as np

from fastplong_amd import build, synth
from tests import hostio, refjson

PERIODIC_S = "ACACACACACACACACACAC"
HOMOPOLYMER_E = "AAAAAAAAAAAAAAAAAAAAAAAA"
ODD_E = "GTGTNACCgtggGAATNNATCCTTAC"  # -e is not validated by the reference (only -s is): N and lower case reach the trims


def fasta17(path):
    rng = np.random.default_rng(17)
    ads = ["".join("ACGT"[i] for i in rng.integers(0, 4, int(n))) for n in rng.integers(12, 40, 17)]
    ads[3] = "AC" * 10  # periodic
    ads[9] = "T" * 20  # homopolymer
    with open(path, "w") as f:
        for i, a in enumerate(ads):
            f.write(">ad%d\n%s\n" % (i, a))
    return ads


# name -> (input kind, flags); "ADAPTERS.fa" is replaced by the path of fasta17()
CASES = {
    "auto_dna": ("auto_dna", []),
    "auto_rna": ("auto_rna", []),
    "full": ("dna", ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]),
    "s_only": ("dna", ["-s", synth.START_ADAPTER]),
    "periodic": ("periodic", ["-s", PERIODIC_S, "-e", HOMOPOLYMER_E, "-d", "0.25"]),
    "odd_e": ("odd", ["-s", synth.START_ADAPTER, "-e", ODD_E, "-d", "0.5"]),
    "fasta17": ("dna", ["-s", synth.START_ADAPTER, "-a", "ADAPTERS.fa"]),
    "d0_ext0": ("dna", ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "-d", "0", "--trimming_extension", "0"]),
    "d1_ext100": ("periodic", ["-s", PERIODIC_S, "-e", HOMOPOLYMER_E, "-d", "1", "--trimming_extension", "100"]),
    "break_mask": ("dna", ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "-b", "--break_window_size", "40",
                           "--break_mean_quality", "12", "-N", "--mask_window_size", "15", "--mask_mean_quality", "14",
                           "-n", "95", "-u", "90"]),
    "split": ("dna", ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--split", "3"]),
}


def reads(kind, n=240, seed=0, median_len=1500):
    """a CSR batch: ONT-like reads with planted (start, end and 20 % middle) adapters of the case's kind"""
    if kind == "dna":
        seq, qual, off = synth.ont_like(n, seed=100 + seed, median_len=median_len, p_middle=0.2)
    elif kind in ("auto_dna", "auto_rna"):  # enough clean copies near the ends for the evaluator to detect both adapters
        seq, qual, off = synth.ont_like(max(n, 600), seed=400 + seed, median_len=600, p_middle=0.2, err=0.02, lead_max=3)
        if kind == "auto_rna":
            seq = seq.copy()
            seq[seq == ord("T")] = ord("U")
    elif kind == "periodic":
        seq, qual, off = synth.ont_like(n, seed=200 + seed, median_len=median_len, p_middle=0.2, start_adapter=PERIODIC_S,
                                        end_adapter=HOMOPOLYMER_E)
    elif kind == "odd":
        seq, qual, off = synth.ont_like(n, seed=300 + seed, median_len=median_len, p_middle=0.2, end_adapter=ODD_E)
    else:
        raise ValueError(kind)
    return seq, qual, off


def write_input(path, kind, **kw):
    seq, qual, off = reads(kind, **kw)
    text, _, _ = hostio.make_fastq(seq, qual, off)
    with open(path, "wb") as f:
        f.write(text)
    return seq, qual, off


def flags_of(name, workdir):
    fl = list(CASES[name][1])
    if "ADAPTERS.fa" in fl:
        p = os.path.join(str(workdir), "ADAPTERS.fa")
        fasta17(p)
        fl[fl.index("ADAPTERS.fa")] = p
    return fl


def _cmd(exe, inp, outdir, flags, threads):
    os.makedirs(str(outdir), exist_ok=True)
    o = str(outdir)
    return [exe, "-i", str(inp), "-o", os.path.join(o, "out.fq"), "--failed_out", os.path.join(o, "failed.fq"),
            "-j", os.path.join(o, "out.json"), "-h", os.path.join(o, "out.html"), "-w", str(threads)] + list(flags)


def run_ref(inp, outdir, flags, threads=4):
    from oracle import oracle

    p = subprocess.run(_cmd(oracle.REF_BIN, inp, outdir, flags, threads), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, cwd=str(outdir))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


def run_cli(env, inp, outdir, flags, threads=4, extra_env=None, extra_flags=()):
    e = dict(env)
    e.update(extra_env or {})
    p = subprocess.run(_cmd(build.CLI, inp, outdir, list(flags) + list(extra_flags), threads), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, env=e, cwd=str(outdir))
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return p


def outputs(d):
    """every FASTQ the run wrote (--split's numbered files included), fastplong.json without its command line and
    fastplong.html without the command line and the time stamp"""
    d = str(d)
    got = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".fq")}
    got["json"] = [l for l in open(os.path.join(d, "out.json"), "rb").read().split(b"\n") if not l.startswith(b'\t"command":')]
    page = refjson.STAMP.sub(b"<time>", open(os.path.join(d, "out.html"), "rb").read())
    got["html"] = re.sub(rb"<div id='footer'> <p>.*?</p>", b"<div id='footer'> <p></p>", page, flags=re.S)
    return got


def detection_lines(p):
    return [l for l in p.stderr.split(b"\n") if l.startswith((b"Detected", b"Not detected", b"Found possible"))]


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if got[k] != want[k]:
            g, w = got[k], want[k]
            if isinstance(g, bytes):
                i = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
                raise AssertionError("%s differs at byte %d of %d/%d: got %r, want %r" % (k, i, len(g), len(w), g[max(0, i - 80):i + 80],
                                                                                     w[max(0, i - 80):i + 80]))
            diff = [(a, b) for a, b in zip(g, w) if a != b][:5]
            raise AssertionError("%s differs: %r (lines %d/%d)" % (k, diff, len(g), len(w)))
