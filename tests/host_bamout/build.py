"""TEST INFRASTRUCTURE ONLY -- builds tests/host_bamout/host_bamout_run: the host's BAM output unit (fastplong_amd/host/bam_out.cpp)
with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own with its own main (main.cpp)."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(HERE, "host_bamout_run")
SRCS = [os.path.join(HERE, "main.cpp"), os.path.join(ROOT, "fastplong_amd", "host", "bam_out.cpp"),
        os.path.join(ROOT, "fastplong_amd", "host", "bam_out.h"), os.path.join(ROOT, "fastplong_amd", "csrc", "bam_out_rules.h")]


def build():
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in SRCS):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", tmp, SRCS[0], SRCS[1]])
        os.replace(tmp, EXE)
    return EXE


def convert(text):
    """-> (header bytes, record bytes) of the sanitized program; raises with the sanitizer's report when it did not end clean"""
    exe = build()
    with tempfile.TemporaryDirectory(prefix="host_bamout_") as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            f.write(text)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
        if p.returncode != 0:
            raise RuntimeError("host_bamout_run ended with %d:\n%s" % (p.returncode, p.stdout.decode(errors="replace")[-4000:]))
        raw = open(fout, "rb").read()
    from tests.bam_out_cases import HEADER_RAW
    return raw[:len(HEADER_RAW)], raw[len(HEADER_RAW):]
