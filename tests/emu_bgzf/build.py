"""TEST INFRASTRUCTURE ONLY -- builds tests/emu_bgzf/emu_bgzf_run: the BGZF inflate kernel (fastplong_amd/csrc/bgzf_inflate.h) on the
host (tests/emu/hip_emu.h), with AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own (a sanitized shared
object cannot be loaded into an unsanitized Python).  A job goes in and comes out as a file:
    in:  u64 comp_bytes, out_bytes, n_blocks, grid (0: the driver picks); n_blocks x fpl_bgzf_block; comp; the initial out
    out: n_blocks x fpl_bgzf_block (status filled in); out
The program poisons every byte of comp and out no descriptor covers, so a kernel that leaves its ranges dies with a report."""
import os

import numpy as np

from tests import cbuild, emujob

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "emu_bgzf_run")
BLOCK_DTYPE = [("comp_off", "<u8"), ("out_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("status", "<u4")]


def build():
    return cbuild.emu_program(EXE, "tests/emu_bgzf/driver.cpp", __file__, main="EMU_BGZF_MAIN")


def start(comp, blocks, out, grid=0):
    """start one sanitized run; finish() collects it"""
    comp = np.ascontiguousarray(comp, np.uint8)
    out = np.ascontiguousarray(out, np.uint8)
    blocks = np.ascontiguousarray(blocks, np.dtype(BLOCK_DTYPE))

    def payload(f):
        f.write(np.array([len(comp), len(out), len(blocks), grid], np.uint64).tobytes())
        f.write(blocks.tobytes())
        f.write(comp.tobytes())
        f.write(out.tobytes())

    return emujob.start(build(), payload, "emu_bgzf_"), len(blocks), len(out)


def finish(job):
    """-> (out, blocks with status); raises with the sanitizer's report when the run did not end clean"""
    run, n, n_out = job
    raw = emujob.finish(run)
    blocks = np.frombuffer(raw[:32 * n], np.dtype(BLOCK_DTYPE)).copy()
    out = np.frombuffer(raw[32 * n:], np.uint8).copy()
    assert len(out) == n_out
    return out, blocks


def inflate(comp, blocks, out, grid=0):
    return finish(start(comp, blocks, out, grid))
