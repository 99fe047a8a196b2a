"""The BAM record kernels (fpl_set_gzip_records; fastplong_amd/csrc/bam_emit.h: k_bamout_layout, k_bamout_compose and their BAM-source
forms) on the CPU emulator, in front of the unchanged BGZF block kernels, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/emu_bamout).

The composed bytes must be, byte for byte, what the host's converter (fplh::fastq_to_bam_records, pinned against plain Python in
tests/test_host_bam_out.py) makes of the host-formatted text of the same records -- and what tests/bam_out_cases.py's own
restatement of the rule makes of it.  The output must be BGZF blocks of 49 152 record bytes each that gzip takes block by block;
with the header block in front and the EOF block behind, tests/bamio.py reads the file back as the formatted text with names cut
and '+' lines bare.

Size condition: output <= total + 5 * deflate blocks + 31 * ceil(total / 49 152) -- a deflate block grows by at most the five
bytes of a stored block's header, a BGZF block adds 18 + 5 + 8 bytes of frame -- with the deflate blocks counted from the cut rule
in Python (bam_out_cases.deflate_blocks)."""
import ctypes as C
import zlib

import numpy as np
import pytest

from fastplong_amd import abi, synth
from tests import bam_out_cases as bc
from tests import bamio, hostio
from tests.bgzf_out_cases import STRIPE, exact_text, one_long_read_text
from tests.emu_bamout import build as emu
from tests.gzcheck import host_format, load_hostlib
from tests.test_bamgz_emu import made_up, stream, whole

C3 = dict(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5, polyx=1, complexity_filter=1)


@pytest.fixture(scope="module")
def hostlib():
    L = load_hostlib()
    L.fplh_fastq_to_bam_records.restype = C.c_int
    L.fplh_fastq_to_bam_records.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    return L


def host_records(L, text):
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_fastq_to_bam_records(text, len(text), C.byref(out), C.byref(n)) == 0
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    return s


def check_output(hostlib, formatted, data, comp, info, label, readable=True):
    """the checks of the module's docstring; formatted: the host's text for the same records"""
    want = host_records(hostlib, formatted)
    assert want == bc.records(formatted)
    assert info["total"] == len(want)
    assert comp == want, next(i for i, (a, b) in enumerate(zip(comp, want)) if a != b)
    if not want:
        assert data == b"" and info["n_blocks"] == 0
        return
    nb, total = bc.deflate_blocks(formatted)
    n_bgzf = -(-total // STRIPE)
    assert info["n_blocks"] == nb and total == len(want)
    assert info["crc"] == zlib.crc32(want)
    blocks = bc.check_device_blocks(data, want)
    assert len(blocks) == n_bgzf
    print("%s: records %d (text %d), BGZF %d in %d blocks of %d deflate blocks" % (label, total, len(formatted), len(data), n_bgzf, nb))
    assert len(data) == info["gz_len"] <= info["out_cap"] == total + 5 * nb + 31 * n_bgzf
    assert bc.check_fixed_fields(want) == len(bc.fastq_records(formatted))
    if readable:
        assert bamio.bam_to_fastq(bc.file_bytes(data)) == bc.cut_text(formatted)


def text_case(hostlib, tmp_path, text, res, label, readable=True):
    formatted = host_format(hostlib, tmp_path, text, res)
    data, comp, info = emu.finish(emu.start_text(text, res))
    check_output(hostlib, formatted, data, comp, info, label, readable)
    return data, formatted


def test_fragment_lengths_at_every_front_trim(hostlib, tmp_path):
    """0 .. 65 around the lane's 32-base unit and its ragged end, 1 022 .. 1 024 around the forced cut; fragments that start at byte
    0 .. 3 of their read and end two bases before its end"""
    text, plan = bc.lengths_text(extra=2)
    res = whole([fl + trim + 2 for fl, trim in plan])
    res["frag_start"][:, 0] = [trim for fl, trim in plan]
    res["frag_len"][:, 0] = [fl for fl, trim in plan]
    data, formatted = text_case(hostlib, tmp_path, text, res, "lengths")
    assert [len(s) for n, s, q in bc.fastq_records(formatted)] == [fl for fl, trim in plan]
    names = [r[1] for r in bamio.parse(bc.file_bytes(data))]
    assert b"L0.0" in names and b"L1.0" in names and b"L0.3_" + b"n" * 249 in names  # cut at a space, at a tab, at 254 bytes


def test_whole_reads_of_every_length(hostlib, tmp_path):
    text, plan = bc.lengths_text()
    text_case(hostlib, tmp_path, text, whole([fl for fl, trim in plan]), "whole reads")


def test_every_base_value(hostlib, tmp_path):
    """all the bytes a line can hold as bases, at even and odd places, through the 32-base unit and the ragged end"""
    vals = bytes(v for v in range(256) if v not in (10, 13))
    text = b"".join(b"@v%d\n%s\n+\n%s\n" % (k, s, bytes(33 + (i * 7 + k) % 94 for i in range(len(s))))
                    for k, s in enumerate([vals, b"A" + vals, vals[:77], vals[100:133] + b"=acgtn"]))
    lens = [len(l) for l in text.split(b"\n")[1::4]]
    data, formatted = text_case(hostlib, tmp_path, text, whole(lens), "base values", readable=False)
    codes = [r[3] for r in bamio.parse(bc.file_bytes(data))]
    assert [list(c) for c in codes] == [[bc.TABLE[b] for b in l] for l in text.split(b"\n")[1::4]]


def test_quality_values(hostlib, tmp_path):
    q = bytes(v for v in range(256) if v not in (10, 13)) * 2
    text = b"@q\n%s\n+\n%s\n" % (b"A" * len(q), q)
    data, _ = text_case(hostlib, tmp_path, text, whole([len(q)]), "quality values", readable=False)
    (_, _, _, _, got), = bamio.parse(bc.file_bytes(data))
    assert got == bytes(max(v, 33) - 33 for v in q)


def test_splits_dropped_and_failing_reads(hostlib, tmp_path):
    """both fragments of a split read with their prefixes, one of them failing, dropped and failing reads between passing ones"""
    rng = np.random.default_rng(7)
    lens = [int(n) for n in rng.integers(0, 700, 400)]
    text = b"".join(bc.rand_read(rng, n, b"@m%d%s" % (i, bc.NAME_TAILS[i % 4])) for i, n in enumerate(lens))
    res = made_up(rng, lens)
    assert (res["dropped"] == 1).any() and (res["code"][:, 0] != abi.FPL_PASS_FILTER).any() and (res["n_frag"] == 2).any()
    data, formatted = text_case(hostlib, tmp_path, text, res, "made-up records")
    names = [r[1] for r in bamio.parse(bc.file_bytes(data))]
    assert any(n.startswith(b"split-by-adapter-left-m") for n in names) and any(n.startswith(b"split-by-adapter-right-m") for n in names)
    assert any(len(n) == 254 and n.startswith(b"split-by-adapter-right-") for n in names)  # the prefix counts towards the 254


def test_splits_through_the_oracle(orc, hostlib, tmp_path):
    seq, qual, off = synth.ont_like(300, seed=5, median_len=900, p_middle=0.25)
    text, _, _ = hostio.make_fastq(seq, qual, off)
    cfg = orc.Config(abi.FplOptions.default(**C3), synth.START_ADAPTER, synth.END_ADAPTER)
    res, _ = orc.process_batch(cfg, seq, qual, off)
    data, formatted = text_case(hostlib, tmp_path, text, res, "splits")
    assert b"@split-by-adapter-left-" in formatted and b"@split-by-adapter-right-" in formatted


@pytest.mark.parametrize("total", [49151, 49152, 49153])
def test_stripe_edges(hostlib, tmp_path, total):
    text = bc.exact_records_text(total)
    lens = [len(l) for l in text.split(b"\n")[1::4]]
    data, _ = text_case(hostlib, tmp_path, text, whole(lens), "edge %d" % total)
    assert len(bc.check_device_blocks(data, bc.records(text))) == -(-total // STRIPE)


def test_every_part_of_a_record_across_a_block_edge(hostlib, tmp_path):
    text, where = bc.straddle_text()
    assert {t % bc.GZ_B for _, _, _, t in where} == {0} and sum(t % STRIPE == 0 for _, _, _, t in where) == 4
    lens = [len(l) for l in text.split(b"\n")[1::4]]
    text_case(hostlib, tmp_path, text, whole(lens), "straddle")


def test_one_read_of_200_kb(hostlib, tmp_path):
    text = one_long_read_text()
    data, _ = text_case(hostlib, tmp_path, text, whole([200_000]), "one long read")
    assert len(bc.check_device_blocks(data, bc.records(text))) == 7


def test_no_read_passes(hostlib, tmp_path):
    text = exact_text(20000)
    lens = [len(l) for l in text.split(b"\n")[1::4]]
    data, _ = text_case(hostlib, tmp_path, text, whole(lens, code=abi.FPL_FAIL_LENGTH), "nothing passes")
    assert data == b""


@pytest.mark.parametrize("seed", [1, 2])
def test_bam_batches_with_reversed_records(hostlib, tmp_path, seed):
    """the BAM source: names out of the records, bases and qualities out of the decoded arrays (flag 0x10: reverse-complemented)"""
    rng = np.random.default_rng(seed)
    recs = bamio.random_records(rng, 300, max_len=1500, flags=(0, 0x10, 0x4, 0x14),
                                lengths=None if seed == 1 else bc.FRAG_LENGTHS)
    assert any(r[1] & 0x10 for r in recs)
    lens = [len(r[2]) for r in recs]
    raw, starts, off, twin = stream(recs)
    for res in (made_up(rng, lens), whole(lens)):
        formatted = host_format(hostlib, tmp_path, twin, res)
        data, comp, info = emu.finish(emu.start_bam(raw, starts, off, res))
        check_output(hostlib, formatted, data, comp, info, "BAM source %d" % seed)
