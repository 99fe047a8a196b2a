"""k_bam_tags_moves, k_bam_moves_plan and the re-indexing compose kernel (fpl_set_bam_moves; fastplong_amd/csrc/bam_moves.h) on the
CPU emulator, around the tagged layout kernel and in front of the unchanged BGZF block kernels, as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu_bammoves).

The composed bytes must be, byte for byte, what the host form makes of the same batch and what the byte rule of
tests/bam_move_cases.py makes of it, and every re-indexed record must satisfy the decoder's property; every BGZF block inflates on
its own; the output keeps the size bound of the tagged form; all twelve counters are the model's, with --keep_mods beside the
switch and without it.  The lists hold records that are not re-indexable and regions that do not parse, so the sanitizers see the
clamping."""
import zlib

import numpy as np

from fastplong_amd import abi
from tests import bam_mod_cases as mc
from tests import bam_move_cases as vc
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.bgzf_out_cases import STRIPE
from tests.emu_bammoves import build as emu
from tests.test_bam_tags_emu import deflate_blocks, stream
from tests.test_host_bam_moves import L, host_form  # noqa: F401  (the host library's hooks)


def check(job, want, stats, mod_stats, move_stats, label):
    data, comp, info = emu.finish(job)
    assert info["move_stats"] == move_stats and info["mod_stats"] == mod_stats and info["stats"] == stats and info["total"] == len(want)
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
    recs, res, _ = vc.case_list()
    raw, starts, off = stream(recs)
    jobs = {mods: emu.start(raw, starts, off, res, mods=mods) for mods in (False, True)}
    for mods, job in jobs.items():
        want = vc.expected(recs, res, mods=mods)
        host = host_form(L, tmp_path, recs, res, 4, mods=mods)
        assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4] and host[6] == want[6]
        for name, region, s, n, t in want[8]:
            vc.check_semantics(region, s, n, t)
            assert len(t) <= len(region)  # a record never carries more tag bytes than its input region: the bound of the tagged form stands
        assert want[6][0] >= 40 and want[6][1] >= 10 and len(want[0]) > 2 * STRIPE and (want[4][0] >= 8) == mods
        check(job, want[0], want[2], want[4], want[6], "case list, mods %d" % mods)


def test_tag_and_mod_case_lists_and_malformed_regions_under_the_switch(L, tmp_path):  # noqa: F811
    """the --keep_tags case list (every kind of region, regions that do not parse, flag 0x10, tables of 50 000 and 100 000 entries
    that are no move tables), --keep_mods' malformed list and this rule's, with both switches on"""
    recs, res = tc.case_list(malformed=True)
    for more, mres in (mc.malformed_list(), vc.malformed_list()):
        recs, res = recs + more, np.concatenate([res, mres])
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res, mods=True)
    want = vc.expected(recs, res, mods=True)
    host = host_form(L, tmp_path, recs, res, 3, mods=True)
    assert host[0] == want[0] and host[2] == want[2] and host[4] == want[4] and host[6] == want[6]
    assert want[6][0] == 3 and want[6][1] > 10 and want[4][1] > 10 and want[2][3] > 5
    check(job, want[0], want[2], want[4], want[6], "tag case list")


def test_fragment_mode_re_indexes_nothing():
    recs, res, _ = vc.case_list()
    recs, res = recs[:120], res[:120]
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res, fragment_mode=True)
    out, st, n = [], tc.Stats(), 0
    for (name, flag, codes, qual, enc), r in zip(recs, res):  # the layout's reading of the records, every one of them changed
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        for f in range(0 if r["dropped"] else int(r["n_frag"])):
            if r["code"][f] == abi.FPL_PASS_FILTER:
                a, k = int(r["frag_start"][f]), int(r["frag_len"][f])
                t = tc.pick(tc.aux_region(enc), True)
                out.append(tc.with_tags(bc.record(b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq[a:a + k], q[a:a + k]), t))
                st.note(tc.aux_region(enc), True, t)
                n += 1
    check(job, b"".join(out), st.v, [0, 0, 0, 0], [0, n, 0, 0], "fragment mode")


def test_nothing_passes():
    recs, res, _ = vc.case_list()
    recs, res = recs[:40], res[:40].copy()
    res["code"][:] = 16
    raw, starts, off = stream(recs)
    check(emu.start(raw, starts, off, res), b"", [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], "nothing passes")
