"""The BAM decode kernel (fastplong_amd/csrc/bam_decode.h) on the CPU emulator against bamio's independent twin: every code,
both strands, qualities 0..254 (clamped at 93), lengths 0, 1, odd and even, records with CIGAR operations and tags, and output
offsets that do not start on a 16-byte word."""
import numpy as np
import pytest

from tests import bamio
from tests.emu_bam import build as emu_bam


def _check(recs, n_cigar=0, tags=b"", shift=0):
    data, starts, raw = bamio.bam_bytes(recs, n_cigar=n_cigar, tags=tags)
    keep = [i for i, r in enumerate(recs) if not (r[1] & 0x900)]
    want_seq, want_qual, off, _ = bamio.twin_csr(data)
    off = off + np.uint64(shift)
    got_seq, got_qual = emu_bam.decode(raw, [starts[i] for i in keep], off)
    assert got_seq[shift:].tobytes() == want_seq.tobytes()
    assert got_qual[shift:].tobytes() == want_qual.tobytes()


@pytest.mark.parametrize("seed", [1, 2])
def test_emu_decode_matches_twin(seed):
    rng = np.random.default_rng(seed)
    recs = bamio.random_records(rng, 2500, max_len=120)
    _check(recs)


def test_emu_decode_cigar_tags_and_offset():
    rng = np.random.default_rng(5)
    recs = bamio.random_records(rng, 600, max_len=70)
    _check(recs, n_cigar=3, tags=b"MMZC+m,1,2;", shift=7)


def test_emu_decode_long_reads_both_strands():
    rng = np.random.default_rng(9)
    recs = bamio.random_records(rng, 6, lengths=[5000, 4999, 1, 0, 8191, 33], flags=(0, 0x10))
    _check(recs)
    # every code at every nibble parity, forwards and backwards
    codes = bytes(range(16)) * 3 + bytes([7])
    _check([(b"a", 0, codes, bytes(range(len(codes)))), (b"b", 0x10, codes, bytes(range(90, 90 + len(codes)))),
            (b"c", 0x10, codes[1:], bytes(200 for _ in codes[1:]))])


def test_emu_decode_runs_of_empty_reads():
    """thousands of l_seq == 0 records at one output offset, inside a word and on a word boundary"""
    recs = [(b"a", 0, bytes([1, 2, 4, 8, 15]), bytes([10, 20, 30, 40, 100]))]
    recs += [(b"e%d" % i, 0x4, b"", b"") for i in range(3000)]
    recs += [(b"b", 0x10, bytes(range(16)) * 2, bytes(range(32)))]
    recs += [(b"f%d" % i, 0x4, b"", b"") for i in range(2000)]
    recs += [(b"c", 0, bytes([3] * 11), bytes([94] * 11))]
    _check(recs)
    _check(recs, shift=11)
