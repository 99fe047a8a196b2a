"""TEST INFRASTRUCTURE ONLY -- builds tests/host_bamcomment/host_bamcomment_run: fmt_float of
fastplong_amd/csrc/bam_comment_rules.h against the libc's "%g", with AddressSanitizer and UndefinedBehaviorSanitizer, as a program
of its own with its own main (main.cpp)."""
import os
import struct

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host_bamcomment_run")


def build():
    return cbuild.compile(EXE, ["-std=c++17", "-O2", "-g", *cbuild.SANITIZE], ["tests/host_bamcomment/main.cpp"], extra_deps=[__file__])


def check(seed):
    """-> (values checked, mismatches, the longest text, a line per mismatch); raises with the sanitizers' report when the run did
    not end clean"""
    raw = emujob.run(build(), lambda f: f.write(struct.pack("<Q", seed)), "host_bamcomment_", timeout=300)
    checked, bad, longest = struct.unpack_from("<QQQ", raw)
    return checked, bad, longest, raw[24:].decode()
