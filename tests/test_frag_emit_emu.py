"""The fragment forms of the device output (fpl_set_fragment_output) on the CPU emulator, as a program of its own under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu_frag): csrc/frag_index.h, k_gz_layout_frag / k_gz_compose_frag and
k_emit_count_frag / k_emit_fill_frag / k_emit_mask with the library's launch order and capacities.

The lists are the oracle's, handed over with their entries SHUFFLED by a seeded permutation: the device's list is in whatever
order the waves of k_break_mask got to the counter, and the index must not depend on it.  What is expected never comes from the
kernels: first[] is FragmentList::index restated (frag_cases.first_of), the text is the host formatter's
(fplh_format_batch_fragments), the CSR arrays are Python slices of the same fragments."""
import numpy as np
import pytest

from fastplong_amd import abi, synth
from tests import frag_cases as fc
from tests import gzcheck
from tests.emu_frag import build as emu


@pytest.fixture(scope="module")
def hostlib():
    return fc.load_hostlib()


def oracle_lists(orc, reads, okw):
    seq, qual, off = fc.csr_of(reads)
    cfg = orc.Config(abi.FplOptions.default(**okw), synth.START_ADAPTER, synth.END_ADAPTER)
    res, _, frags, regs = orc.process_batch_ex(cfg, seq, qual, off)
    return res, frags, regs


def shuffled(frags, seed):
    return frags[np.random.default_rng(seed).permutation(len(frags))]


def check(orc, hostlib, tmp_path, reads, okw, seed, bgzf=False, **kw):
    res, frags, regs = oracle_lists(orc, reads, okw)
    text = fc.text_of(reads)
    mixed = shuffled(frags, seed)
    r = emu.run(text, res, mixed, regs, bgzf=bgzf, **kw)
    ix = r["index"]
    assert ix["status"] == 0 and ix["n"] == len(frags)
    assert ix["first"].tolist() == fc.first_of(frags, len(reads)).tolist()
    # order[] names, place by place, the entries of the shuffled list that are the sorted list's
    assert mixed[ix["order"]].tobytes() == frags.tobytes()
    want = fc.host_format(hostlib, tmp_path, text, res, frags, regs)
    g = r["gz"]
    assert g["layout"]["status"] == 0 and g["composed"] == want
    if want:
        assert g["header"]["status"] == 0
        if bgzf:
            fc.inflate_stripes(g["bytes"], want)
        else:
            assert gzcheck.inflate_all(g["bytes"], len(want)) == want
    else:
        assert g["bytes"] == b"" and g["layout"]["total"] == 0
    off, src, kind, brk, seq, qual = fc.csr_slices(reads, res, frags, regs)
    c = r["csr"]
    assert c["status"] == 0 and c["off0"] == 0 and c["n_out"] == len(src) and c["n_bytes"] == len(seq)
    assert c["off"] == off and c["src"].tolist() == src and c["kind"].tolist() == kind and c["break_no"].tolist() == brk
    assert c["seq"] == seq and c["qual"] == qual
    return res, frags, regs, want, r


def test_names(orc, hostlib, tmp_path):
    res, frags, regs, want, _ = check(orc, hostlib, tmp_path, fc.names_case(), fc.BREAK_ONLY, 1)
    ok = frags[frags["code"] == 0]
    assert ok["break_no"].max() >= 10 and b"@r9-nine\n" in want and b"@r10-ten\n" in want
    assert ((ok["kind"] == 1) & (ok["break_no"] > 0)).any() and ((ok["kind"] == 2) & (ok["break_no"] > 0)).any()
    assert b"@r1-\n" in want and b"@r1-twelve stretches\n" in want
    assert b"@r1-split-by-adapter-left-adapter in the middle\n" in want


def test_masks(orc, hostlib, tmp_path):
    reads = fc.masks_case()
    res, frags, regs, want, _ = check(orc, hostlib, tmp_path, reads, fc.BREAK_MASK, 2)
    ok = frags[(frags["code"] == 0) & (frags["region_count"] > 0)]
    assert len(ok) >= 3
    first = [regs[f["region_first"]] for f in ok]
    assert any(int(g["start"]) == int(f["start"]) for f, g in zip(ok, first))  # a masked stretch at output offset 0
    ends = [(f, regs[int(f["region_first"]) + int(f["region_count"]) - 1]) for f in ok]
    assert any(int(g["start"] + g["len"]) == int(f["start"] + f["len"]) for f, g in ends)  # ... and one up to the last base
    b2b = [f for f in ok if f["region_count"] >= 2 and
           int(regs[f["region_first"]]["start"] + regs[f["region_first"]]["len"]) == int(regs[int(f["region_first"]) + 1]["start"])]
    assert b2b
    whole = frags[frags["read"] == 3]
    assert len(whole) == 1 and whole[0]["code"] != 0 and int(regs[whole[0]["region_first"]]["len"]) == int(whole[0]["len"])
    assert b"@whole" not in want and (frags["break_no"] > 0).any()


@pytest.mark.parametrize("lengths", [(1021,), (1022,), (1023,), (1024,), (1025,), (1021, 1022, 1023, 1024, 1025)])
def test_forced_cuts(orc, hostlib, tmp_path, lengths):
    reads = fc.forced_case(lengths)
    res, frags, regs, want, r = check(orc, hostlib, tmp_path, reads, fc.MASK_ONLY, 3)
    assert len(frags) == len(reads) and (frags["code"] == 0).all()
    # a bases line of GZ_L bytes with its line end starts a block at its name line and one at its '+' line
    starts = set(r["gz"]["blk_start"].tolist())
    for f, o in zip(frags, r["gz"]["rec_off"][:-1]):
        name = len(reads[int(f["read"])][0])
        forced = int(f["len"]) + 1 >= 1024
        assert (int(o) in starts or int(o) == 0) == (forced or int(o) == 0)
        assert (int(o) + name + 1 + int(f["len"]) + 1 in starts) == forced


def test_scans_and_stripes(orc, hostlib, tmp_path):
    # more than one 1024-lane step of the layout, more than one block of the count kernel, every fragment broken
    res, frags, regs, want, r = check(orc, hostlib, tmp_path, fc.scan_case(1100), fc.BREAK_ONLY, 4)
    assert len(frags) > 1024 and (frags["break_no"] > 0).all()
    res, frags, regs, want, r = check(orc, hostlib, tmp_path, fc.stripes_case(), fc.BREAK_MASK, 5, bgzf=True)
    assert len(want) > 3 * 49152


def test_nothing(orc, hostlib, tmp_path):
    for reads, okw in (([], fc.BREAK_MASK), (fc.all_fail_case(), fc.MASK_ONLY)):
        res, frags, regs, want, r = check(orc, hostlib, tmp_path, reads, okw, 6)
        assert want == b"" and r["csr"]["n_out"] == 0
    # every read dropped: the records say so, whatever the list holds
    reads = fc.masks_case()
    res, frags, regs = oracle_lists(orc, reads, fc.BREAK_MASK)
    res = res.copy()
    res["dropped"] = 1
    r = emu.run(fc.text_of(reads), res, shuffled(frags, 7), regs)
    assert r["index"]["status"] == 0 and r["gz"]["layout"]["total"] == 0 and r["gz"]["bytes"] == b""
    assert r["csr"]["status"] == 0 and r["csr"]["n_out"] == 0 and r["csr"]["off0"] == 0


def test_status(orc, tmp_path):
    """a list that overflowed, a count beyond the capacity, an entry of no read, a seq_no twice: a status, and nothing is written"""
    reads = fc.masks_case()
    res, frags, regs = oracle_lists(orc, reads, fc.BREAK_MASK)

    def refused(r, bit):
        assert r["index"]["status"] & bit and r["index"]["n"] == 0
        assert r["gz"]["layout"]["status"] & 4 and r["gz"]["layout"]["total"] == 0
        assert r["csr"]["status"] & 4 and r["csr"]["n_out"] == 0 and r["csr"]["off0"] == 0

    text = fc.text_of(reads)
    refused(emu.run(text, res, frags, regs, overflow=True), 1)
    refused(emu.run(text, res, frags, regs, frag_cap=len(frags) - 1), 1)
    bad = frags.copy()
    bad[2]["read"] = len(reads)
    refused(emu.run(text, res, bad, regs), 2)
    bad = frags.copy()
    bad[-1]["seq_no"] = 5
    refused(emu.run(text, res, bad, regs), 2)
    # the CSR capacities are still checked: bit 1, nothing written
    r = emu.run(text, res, frags, regs, cap_reads=1)
    assert r["csr"]["status"] == 2 and r["csr"]["n_out"] == 0
