"""Test helpers shared by tests/test_emit_emu.py and tests/test_gpu_emit.py: hand-made batches and records for
fpl_emit_batch_device (fastplong_amd/csrc/emit.h), the numpy gather that says what must come out, and the check of a run against
it.  A backend is a function

    run(seq, qual, off, res, cap_bytes, cap_reads, shift) -> (rc, info, seq_out, qual_out, off_out, src, kind)

that runs the kernels with exactly these capacities over outputs pre-filled with PAT / PAT64 / PAT32 and GUARD spare items behind
the capacity, the output byte arrays starting `shift` bytes behind a 16-byte boundary, and returns the WHOLE arrays (capacity +
GUARD items) as numpy arrays."""
import numpy as np

from fastplong_amd import abi

RES = np.dtype(abi.RESULT_DTYPE)
PASS = abi.FPL_PASS_FILTER
PAT, PAT64, PAT32 = 0xA5, 0x5A5A5A5A5A5A5A5A, 0xDEADBEEF
GUARD = 64

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025]


def batch(rng, lens):
    """random bytes (every value: the gather must not care) as a CSR batch"""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    return rng.integers(0, 256, total, dtype=np.uint8), rng.integers(0, 256, total, dtype=np.uint8), off


def records(n):
    return np.zeros(n, RES)


def one_fragment(lens, starts=None, flens=None, kind=0):
    """a passing fragment per read: the window [start, start + flen) (default: the whole read)"""
    lens = np.asarray(lens, np.int64)
    res = records(len(lens))
    res["n_frag"] = 1
    res["frag_start"][:, 0] = 0 if starts is None else starts
    res["frag_len"][:, 0] = lens if flens is None else flens
    res["kind"][:, 0] = kind
    res["code"][:, 0] = PASS
    res["code"][:, 1] = abi.FPL_FAIL_LENGTH  # (beyond n_frag: must not be looked at)
    return res


def reference(seq, qual, off, res):
    """the numpy gather over the records -> (seq_out, qual_out, off_out, src, kind); None when a counted window reaches outside its
    read"""
    n = len(off) - 1
    o = off.astype(np.int64)
    lens = np.diff(o)
    take = [(res["dropped"] == 0) & (res["n_frag"] > f) & (res["code"][:, f] == PASS) for f in range(2)]
    for f in range(2):
        if (res["frag_start"][:, f].astype(np.int64) + res["frag_len"][:, f].astype(np.int64) > lens)[take[f]].any():
            return None
    # input order, fragment 0 before fragment 1: interleave the two columns and keep what is taken
    tk = np.stack(take, axis=1).reshape(-1)
    src = np.repeat(np.arange(n, dtype=np.int64), 2)[tk]
    start = (o[:-1, None] + res["frag_start"].astype(np.int64)).reshape(-1)[tk]
    flen = res["frag_len"].astype(np.int64).reshape(-1)[tk]
    kind = res["kind"].reshape(-1)[tk]
    off_out = np.zeros(len(flen) + 1, np.int64)
    off_out[1:] = np.cumsum(flen)
    idx = np.repeat(start - off_out[:-1], flen) + np.arange(int(off_out[-1]), dtype=np.int64)
    return seq[idx], qual[idx], off_out, src.astype(np.uint32), kind.astype(np.uint8)


def check(run, seq, qual, off, res, shift=0, spare_bytes=0, spare_reads=0):
    """runs with the exact capacities (plus spare_*) and holds everything against reference(); -> (info, want)"""
    want = reference(seq, qual, off, res)
    assert want is not None
    ws, wq, woff, wsrc, wkind = want
    n_out, n_bytes = len(wsrc), len(ws)
    cap_b, cap_r = n_bytes + spare_bytes, n_out + spare_reads
    rc, info, gs, gq, goff, gsrc, gkind = run(seq, qual, off, res, cap_b, cap_r, shift)
    assert rc == 0
    flens = np.diff(woff)
    assert info == dict(n_bytes=n_bytes, n_out=n_out, max_len=int(flens.max()) if n_out else 0, status=0), info
    assert len(gs) == cap_b + GUARD and len(gq) == cap_b + GUARD and len(goff) == cap_r + 1 + GUARD
    assert np.array_equal(gs[:n_bytes], ws) and np.array_equal(gq[:n_bytes], wq)
    assert (gs[n_bytes:] == PAT).all() and (gq[n_bytes:] == PAT).all()  # nothing behind the output, the guard bytes least of all
    assert np.array_equal(goff[:n_out + 1].astype(np.int64), woff)
    assert (goff[n_out + 1:] == np.uint64(PAT64)).all()
    assert np.array_equal(gsrc[:n_out], wsrc) and (gsrc[n_out:] == PAT32).all()
    assert np.array_equal(gkind[:n_out], wkind) and (gkind[n_out:] == PAT).all()
    return info, want


def check_refused(run, seq, qual, off, res, cap_bytes, cap_reads, status, shift=0):
    """a run that must set `status` and leave everything but d_off_out[0] as it was"""
    rc, info, gs, gq, goff, gsrc, gkind = run(seq, qual, off, res, cap_bytes, cap_reads, shift)
    assert rc == 0
    assert info == dict(n_bytes=0, n_out=0, max_len=0, status=status), info
    assert (gs == PAT).all() and (gq == PAT).all()
    assert goff[0] == 0 and (goff[1:] == np.uint64(PAT64)).all()
    assert (gsrc == PAT32).all() and (gkind == PAT).all()


# ---- the cases -------------------------------------------------------------------------------------------------------------------

def case_lengths_and_alignments(tile):
    """every fragment length of the list and the tile size -1 / +0 / +1, each at every source alignment 0..15: read k of a length
    starts its fragment k bytes into a read whose own start wanders (the reads have a tail of k % 3 bytes behind the fragment)"""
    rng = np.random.default_rng(21)
    flens, starts, lens = [], [], []
    for L in LENGTHS + [tile - 1, tile, tile + 1]:
        for a in range(16):
            flens.append(L)
            starts.append(a)
            lens.append(a + L + a % 3)
    seq, qual, off = batch(rng, lens)
    return seq, qual, off, one_fragment(lens, starts, flens)


def alignments(off, res, want):
    """({source alignments}, {destination alignments}) of the non-empty output reads"""
    woff, wsrc = want[2], want[3].astype(np.int64)
    flens = np.diff(woff)
    # (one fragment per read in the cases this is asked of)
    s = (off.astype(np.int64)[wsrc] + res["frag_start"][wsrc, 0].astype(np.int64))[flens > 0] % 16
    d = woff[:-1][flens > 0] % 16
    return set(s.tolist()), set(d.tolist())


def case_tiles(tile):
    """a tile with parts of five reads (the end of a long one, three short ones, the head of the next), a read over more than three
    tiles, and a last tile with the ragged end of the output"""
    rng = np.random.default_rng(22)
    lens = [tile - 10, 2, 0, 3, 1, 3 * tile + 100, 3, 40, 1]
    seq, qual, off = batch(rng, lens)
    return seq, qual, off, one_fragment(lens)


def case_tiny():
    """the whole output is shorter than one lane's 16 bytes"""
    rng = np.random.default_rng(23)
    lens = [30, 0, 9]
    seq, qual, off = batch(rng, lens)
    return seq, qual, off, one_fragment(lens, [27, 0, 2], [3, 0, 4])


def case_record_kinds():
    """dropped, n_frag 0, one fragment passing / failing, two fragments in all four combinations (a failing fragment 0 in front of a
    passing fragment 1 among them), twice over so that the kinds meet in both orders"""
    rng = np.random.default_rng(24)
    F = abi.FPL_FAIL_QUALITY
    rows = [  # dropped, n_frag, (start, len, code, kind) x 2
        (1, 1, (0, 50, PASS, 0), (0, 0, 0, 0)),          # dropped: counts for nothing though the fragment "passes"
        (0, 0, (0, 50, PASS, 0), (60, 20, PASS, 2)),     # no fragment: what lies in the slots is not looked at
        (0, 1, (3, 40, PASS, 0), (50, 30, PASS, 2)),     # one fragment: slot 1 is beyond n_frag
        (0, 1, (3, 40, F, 0), (0, 0, 0, 0)),
        (0, 2, (2, 30, PASS, 1), (45, 33, PASS, 2)),
        (0, 2, (2, 30, PASS, 1), (45, 33, F, 2)),
        (0, 2, (2, 30, F, 1), (45, 33, PASS, 2)),        # a failing fragment 0 in front of a passing fragment 1
        (0, 2, (2, 30, F, 1), (45, 33, abi.FPL_FAIL_LENGTH, 2)),
        (0, 2, (0, 0, PASS, 1), (17, 83, PASS, 2)),      # an empty left part
    ]
    rows = rows + rows[::-1]
    res = records(len(rows))
    for i, (dr, nf, f0, f1) in enumerate(rows):
        res["dropped"][i], res["n_frag"][i] = dr, nf
        for f, (st, ln, code, kind) in enumerate((f0, f1)):
            res["frag_start"][i, f], res["frag_len"][i, f], res["code"][i, f], res["kind"][i, f] = st, ln, code, kind
    seq, qual, off = batch(rng, [100] * len(rows))
    return seq, qual, off, res


def case_all_fail():
    rng = np.random.default_rng(25)
    lens = [40, 0, 1000, 17]
    seq, qual, off = batch(rng, lens)
    res = one_fragment(lens)
    res["code"][:, 0] = abi.FPL_FAIL_LENGTH
    res["dropped"][2] = 1
    return seq, qual, off, res


def case_random(n, seed):
    """n reads of 0..40 bytes with records of every kind: a tenth dropped, 0 / 1 / 2 fragments, two thirds of them passing, windows
    anywhere inside the read, the second behind the first"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 41, n)
    seq, qual, off = batch(rng, lens)
    res = records(n)
    res["dropped"] = rng.random(n) < 0.1
    res["n_frag"] = rng.integers(0, 3, n)
    cut = np.sort(rng.integers(0, lens[:, None] + 1, (n, 4)), axis=1)  # four cuts: [c0, c1) and [c2, c3)
    for f in range(2):
        res["frag_start"][:, f] = cut[:, 2 * f]
        res["frag_len"][:, f] = cut[:, 2 * f + 1] - cut[:, 2 * f]
        res["code"][:, f] = np.where(rng.random(n) < 0.67, PASS, abi.FPL_FAIL_LENGTH)
    two = res["n_frag"] == 2
    res["kind"][two, 0], res["kind"][two, 1] = 1, 2
    return seq, qual, off, res
