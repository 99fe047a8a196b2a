"""The kernel chain of fpl_set_bam_comments (fastplong_amd/csrc/bam_comments.h) on the CPU emulator: the walk and the plan of the
tagged record form as they are, k_bam_comment_tags, k_bam_comment_len, the layout and the compose kernel with the comments, in front
of the unchanged block kernels in member and BGZF framing, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/emu_bamcomments).

The composed text must be, byte for byte, what the plain-Python model of tests/bam_comment_cases.py and the host form
(host/bam_comments.cpp) make of the same batch; total, CRC, block counts and the output bound hold; every block inflates; the 5x
bound holds for every record of the list; with the switch off the bytes are k_gz_compose_bam's; a batch in which nothing passes gives
nothing.  The list holds regions that do not parse, control bytes, every B subtype at 0 .. 4097 elements and one comment longer
than a deflate block and a stripe together, so the sanitizers see the clamping."""
import gzip
import zlib

import pytest

from tests import bam_comment_cases as cc
from tests import bam_out_cases as bc
from tests.bgzf_out_cases import STRIPE, check_blocks
from tests.emu_bamcomments import build as emu
from tests.test_bam_tags_emu import stream
from tests.test_host_bam_comments import L, cases, host_form  # noqa: F401  (the host library's hooks, the case list)


def deflate_blocks(text):
    """how many deflate blocks the layout cuts this text into: every multiple of 16 384 starts one, and a read whose bases line has
    at least 1 024 bytes starts one at its name line and one at its '+' line -- the comment is part of the name line"""
    starts, o = set(), 0
    lines = text.split(b"\n")
    for k in range(0, len(lines) - 1, 4):
        a, b = len(lines[k]) + 1 + len(lines[k + 1]) + 1, len(lines[k + 2]) + 1 + len(lines[k + 3]) + 1
        if len(lines[k + 1]) + 1 >= bc.GZ_L:
            starts.update((o, o + a))
        o += a + b
    assert o == len(text)
    starts.update(range(0, o, bc.GZ_B))
    return len(starts)


def check(job, want, stats, bgzf, label):
    data, comp, info = emu.finish(job)
    assert info["total"] == len(want) and info["stats"] == stats
    assert comp == want, next(i for i, (a, b) in enumerate(zip(comp, want)) if a != b)
    if not want:
        assert data == b""
        return data
    nb = deflate_blocks(want)
    assert info["n_blocks"] == nb <= info["blk_cap"] and info["crc"] == zlib.crc32(want)
    if bgzf:
        n_bgzf = -(-len(want) // STRIPE)
        blocks = check_blocks(data, want, piece=STRIPE)  # (every block inflates on its own, to its stripe)
        assert len(blocks) == n_bgzf and all(len(b) <= 65536 for b in blocks)
        assert len(data) == info["gz_len"] <= info["out_cap"] == len(want) + 5 * nb + 31 * n_bgzf
    else:
        assert gzip.decompress(data) == want and zlib.decompressobj(31).decompress(data) == want
        assert len(data) == info["gz_len"] <= info["out_cap"] == len(want) + 5 * nb + 23
    print("%s: text %d, output %d in %d deflate blocks" % (label, len(want), len(data), nb))
    return data


@pytest.fixture(scope="module")
def streamed(cases):  # noqa: F811
    return stream(cases[0])


def test_every_selection_equals_the_model_and_the_host_form(L, cases, streamed):  # noqa: F811
    recs, res = cases[0], cases[1]
    raw, starts, off = streamed
    jobs = {}
    for name, sel in cc.SELECTIONS.items():  # (side by side: each is a process of its own)
        jobs[name] = emu.start(raw, starts, off, res, *cc.selection_args(sel), bgzf=name in ("all", "first"))
    jobs["off"] = emu.start(raw, starts, off, res)
    today = None
    for name, job in jobs.items():
        sel = cc.SELECTIONS.get(name)
        want = cc.expected(recs, res, sel)
        host = host_form(L, cases, sel, 4)
        assert host[0] == want[0] and host[2] == want[2]
        data = check(job, want[0], want[2] if sel else [0] * 4, name in ("all", "first"), name)
        if name in ("off", "nothing"):  # the switch off, and a list that matches nothing: the bytes of k_gz_compose_bam
            today = today or data
            assert data == today
    want = cc.expected(recs, res, "*")
    assert max(len(l) for l in want[0].split(b"\n")) > STRIPE + bc.GZ_B and want[2][3] >= 4
    assert cc.bound_holds(recs)


def test_fragment_mode_re_indexes_nothing(cases, streamed):  # noqa: F811
    """(the library's layout reads the per-read records in a --break / --mask context too: every record counts as changed)"""
    recs, res = cases[0][:200], cases[1][:200]
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res, b"", -1, fragment_mode=True)
    out, st = [], [0] * 4
    from fastplong_amd import abi
    from tests import bam_tag_cases as tc
    from tests import bamio
    for (name, flag, codes, qual, enc), r in zip(recs, res):
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        for f in range(0 if r["dropped"] else int(r["n_frag"])):
            if r["code"][f] == abi.FPL_PASS_FILTER:
                a, k = int(r["frag_start"][f]), int(r["frag_len"][f])
                c, n, left = cc.comment(cc.tag_bytes_of(tc.aux_region(enc), codes, flag, a, k, True, True), "*")
                cc.note(st, c, n, left)
                out.append(b"@" + tc.PREFIX[int(r["kind"][f])] + name + c + b"\n" + seq[a:a + k] + b"\n+\n" + q[a:a + k] + b"\n")
    text = b"".join(out)
    assert b"\tMM:Z:" not in text and b"\tRG:Z:" in text
    check(job, text, st, False, "fragment mode")


def test_nothing_passes(cases):  # noqa: F811
    recs, res = cases[0][:40], cases[1][:40].copy()
    res["code"][:] = 16
    raw, starts, off = stream(recs)
    for bgzf in (False, True):
        check(emu.start(raw, starts, off, res, b"", -1, bgzf=bgzf), b"", [0] * 4, bgzf, "nothing passes")
