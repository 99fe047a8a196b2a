"""k_bam_tags and the tagged BAM-source layout and compose kernels (fpl_set_bam_tags; fastplong_amd/csrc/bam_tags.h) on the CPU
emulator, in front of the unchanged BGZF block kernels, as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/emu_bamtags).

The composed bytes must be, byte for byte, what the host form makes of the same batch and what the plain-Python rule of
tests/bam_tag_cases.py makes of it; every BGZF block inflates on its own; the output is at most total + 5 * deflate blocks + 31 *
ceil(total / 49 152) bytes, the deflate blocks counted from the cut rule in Python; the four counters are the model's.  The case
list holds regions that do not parse to their end, so the sanitizers see the clamping."""
import struct
import zlib

import numpy as np
import pytest

from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio
from tests.bgzf_out_cases import STRIPE
from tests.emu_bamtags import build as emu
from tests.test_host_bam_tags import L, host_form  # noqa: F401  (the host library's hooks)


def stream(recs):
    """-> (uncompressed stream, starts of the records that are not skipped, CSR offsets of their bases)"""
    raw, starts, off = bytearray(bamio.header()), [], [0]
    for name, flag, codes, qual, enc in recs:
        if not flag & 0x900:
            starts.append(len(raw))
            off.append(off[-1] + len(codes))
        raw += enc
    return bytes(raw), np.array(starts, np.uint64), np.array(off, np.uint64)


def deflate_blocks(raw):
    """how many deflate blocks the layout cuts these records into: every multiple of 16 384 starts one, and a record with
    l_seq + 1 >= 1 024 starts one at its first byte and one at its first quality byte (the tags join the qualities' part)"""
    starts, o = set(), 0
    while o < len(raw):
        bs, l_name, l_seq = struct.unpack_from("<I", raw, o)[0], raw[o + 12], struct.unpack_from("<I", raw, o + 20)[0]
        if l_seq + 1 >= bc.GZ_L:
            starts.update((o, o + 36 + l_name + (l_seq + 1) // 2))
        o += 4 + bs
    assert o == len(raw)
    starts.update(range(0, o, bc.GZ_B))
    return len(starts)


def check(job, want, stats, label):
    data, comp, info = emu.finish(job)
    assert info["total"] == len(want) and info["stats"] == stats
    assert comp == want, next(i for i, (a, b) in enumerate(zip(comp, want)) if a != b)
    if not want:
        assert data == b""
        return
    nb, n_bgzf = deflate_blocks(want), -(-len(want) // STRIPE)
    assert info["n_blocks"] == nb and info["crc"] == zlib.crc32(want)
    blocks = bc.check_device_blocks(data, want)  # stripes of 49 152 bytes that gzip takes one by one
    assert len(blocks) == n_bgzf
    print("%s: records %d, BGZF %d in %d blocks of %d deflate blocks" % (label, len(want), len(data), n_bgzf, nb))
    assert len(data) == info["gz_len"] <= info["out_cap"] == len(want) + 5 * nb + 31 * n_bgzf


@pytest.fixture(scope="module")
def cases():
    return tc.case_list(malformed=True)


def test_case_list_equals_host_form_and_model(L, tmp_path, cases):  # noqa: F811
    recs, res = cases
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res)
    want = tc.expected(recs, res)
    host = host_form(L, tmp_path, recs, res, 4)
    assert host[0] == want[0] and host[2] == want[2]
    assert want[2][3] > 5 and len(want[0]) > 5 * STRIPE  # regions that do not parse; regions that cross one stripe and two
    check(job, want[0], want[2], "case list")


def test_fragment_mode_changes_every_record(cases):
    recs, res = cases
    recs = [r for r in recs if len(r[4]) < 20000][:150]
    res = res[:len([r for r in recs if not r[1] & 0x900])]
    raw, starts, off = stream(recs)
    job = emu.start(raw, starts, off, res, fragment_mode=True)
    kept = [r for r in recs if not r[1] & 0x900]
    out, st = [], tc.Stats()
    for (name, flag, codes, qual, enc), r in zip(kept, res):  # the layout's reading of the records, every one of them changed
        _, seq, _, q, _ = bamio.twin_record(name, flag, codes, qual).split(b"\n")
        for f in range(0 if r["dropped"] else int(r["n_frag"])):
            if r["code"][f] == 0:
                a, n = int(r["frag_start"][f]), int(r["frag_len"][f])
                t = tc.pick(tc.aux_region(enc), True)
                out.append(tc.with_tags(bc.record(b"@" + tc.PREFIX[int(r["kind"][f])] + name, seq[a:a + n], q[a:a + n]), t))
                st.note(tc.aux_region(enc), True, t)
    check(job, b"".join(out), st.v, "fragment mode")


def test_a_block_size_that_runs_past_the_buffer_is_clamped():
    """the last record claims more aux bytes than the stream holds: the region ends with the buffer, nothing behind it is read"""
    rng = np.random.default_rng(3)
    recs = []
    for i in range(5):
        codes, qual = rng.integers(1, 16, 50, dtype=np.uint8).tobytes(), bytes([30] * 50)
        recs.append((b"c%d" % i, 4, codes, qual, bamio.encode_record(b"c%d" % i, 4, codes, qual, tags=tc.K1 + tc.K2)))
    n, f, c, q, enc = recs[-1]
    lying = struct.pack("<I", struct.unpack_from("<I", enc)[0] + 100000) + enc[4:]
    raw, starts, off = stream(recs[:-1] + [(n, f, c, q, lying)])
    res = np.array([tc.result_of("whole", 50)] * 5, np.dtype(__import__("fastplong_amd").abi.RESULT_DTYPE))
    want = tc.expected(recs, res)  # (the model sees the honest record: the bytes in the buffer are the same)
    check(emu.start(raw, starts, off, res), want[0], want[2], "clamped")


def test_nothing_passes(cases):
    recs, res = cases
    recs, res = recs[:40], res[:len([r for r in recs[:40] if not r[1] & 0x900])].copy()
    res["code"][:] = 16
    raw, starts, off = stream(recs)
    check(emu.start(raw, starts, off, res), b"", [0, 0, 0, 0], "nothing passes")
