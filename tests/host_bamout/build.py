"""TEST INFRASTRUCTURE ONLY -- builds tests/host_bamout/host_bamout_run: the host's BAM output unit (fastplong_amd/host/bam_out.cpp)
with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own with its own main (main.cpp)."""
import os

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host_bamout_run")


def build():
    return cbuild.compile(EXE, ["-std=c++17", "-O1", "-g", *cbuild.SANITIZE], ["tests/host_bamout/main.cpp", "fastplong_amd/host/bam_out.cpp"],
                          extra_deps=[__file__])


def convert(text):
    """-> (header bytes, record bytes) of the sanitized program; raises with the sanitizer's report when it did not end clean"""
    raw = emujob.run(build(), lambda f: f.write(text), "host_bamout_", asan_options="detect_leaks=1:abort_on_error=0", timeout=120)
    from tests.bam_out_cases import HEADER_RAW
    return raw[:len(HEADER_RAW)], raw[len(HEADER_RAW):]
