"""k_bam_tags_mods, k_bam_mods_plan and the re-indexing compose kernel (fpl_set_bam_mods; fastplong_amd/csrc/bam_mods.h) on the CPU
emulator, around the tagged layout kernel and in front of the unchanged BGZF block kernels, as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu_bammods).

The composed bytes must be, byte for byte, what the host form makes of the same batch and what the byte rule of
tests/bam_mod_cases.py makes of it, and every re-indexed record must satisfy the decoder's property; every BGZF block inflates on
its own; the output keeps the size bound of the tagged form; all eight counters are the model's.  The lists hold records that are
not re-indexable and regions that do not parse, so the sanitizers see the clamping."""
import zlib

import numpy as np
import pytest

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests.bgzf_out_cases import STRIPE
from tests.emu_bammods import build as emu
from tests.test_bam_tags_emu import deflate_blocks, stream
from tests.test_host_bam_mods import L, host_form  # noqa: F401  (the host library's hooks)


def check(job, want, stats, mod_stats, label):
    data, comp, info = emu.finish(job)
    assert info["mod_stats"] == mod_stats and info["stats"] == stats and info["total"] == len(want)
    assert comp == want, next(i for i, (a, b) in enumerate(zip(comp, want)) if a != b)
    if not want:
        assert data == b""
        return
    nb, n_bgzf = deflate_blocks(want), -(-len(want) // STRIPE)
    assert info["n_blocks"] == nb and info["crc"] == zlib.crc32(want)
    blocks = bc.check_device_blocks(data, want)
    assert len(blocks) == n_bgzf
    print("%s: records %d, BGZF %d in %d blocks of %d deflate blocks" % (label, len(want), len(data), n_bgzf, nb))
    assert len(data) == info["gz_len"] <= info["out_cap"] == len(want) + 5 * nb + 31 * n_bgzf


def test_case_list_equals_host_form_and_model(L, tmp_path):  # noqa: F811
    recs, res, _ = mc.case_list()
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res)
    want = mc.expected(recs, res)
    host = host_form(L, tmp_path, recs, res, 4)
    assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4]
    for name, region, codes, s, n, t in want[6]:
        mc.check_semantics(region, codes, s, n, t)
    assert want[4][0] >= 40 and want[4][1] >= 10 and len(want[0]) > 2 * STRIPE
    # a record never carries more tag bytes than its input region: the bound of the tagged form stands
    assert all(len(t) <= len(region) for _, region, _, _, _, t in want[6])
    check(job, want[0], want[2], want[4], "case list")


def test_tag_case_list_and_malformed_regions_under_the_switch(L, tmp_path):  # noqa: F811
    """the --keep_tags case list (every kind of region, regions that do not parse, flag 0x10, records without the fields) with
    the switch on, and the regions that do not parse behind their MM field"""
    recs, res = tc.case_list(malformed=True)
    more, mres = mc.malformed_list()
    recs, res = recs + more, np.concatenate([res, mres])
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res)
    want = mc.expected(recs, res)
    host = host_form(L, tmp_path, recs, res, 3)
    assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4]
    assert want[4][0] >= 1 and want[4][1] > 10 and want[2][3] > 5  # (its MN fields say 120: few of its records are re-indexable)
    check(job, want[0], want[2], want[4], "tag case list")


def test_fragment_mode_re_indexes_nothing():
    recs, res, _ = mc.case_list()
    recs, res = recs[:120], res[:120]
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res, fragment_mode=True)
    out, st, n = [], tc.Stats(), 0
    from tests import bamio
    for (name, flag, codes, qual, enc), r in zip(recs, res):  # the layout's reading of the records, every one of them changed
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        for f in range(0 if r["dropped"] else int(r["n_frag"])):
            if r["code"][f] == abi.FPL_PASS_FILTER:
                a, k = int(r["frag_start"][f]), int(r["frag_len"][f])
                t = tc.pick(tc.aux_region(enc), True)
                out.append(tc.with_tags(bc.record(b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq[a:a + k], q[a:a + k]), t))
                st.note(tc.aux_region(enc), True, t)
                n += 1
    check(job, b"".join(out), st.v, [0, n, 0, 0], "fragment mode")


def test_nothing_passes():
    recs, res, _ = mc.case_list()
    recs, res = recs[:40], res[:40].copy()
    res["code"][:] = 16
    raw, starts, off = stream(recs)
    check(emu.start(raw, starts, off, res), b"", [0, 0, 0, 0], [0, 0, 0, 0], "nothing passes")
