"""TEST INFRASTRUCTURE ONLY -- the batches of the fragment-output tests (tests/test_frag_emit_emu.py on the emulator,
tests/test_gpu_frag_out.py on the device) and what they are compared with: the host formatter over the same fragment list.

Qualities are two letters, one far above and one far below the thresholds, so the low-quality regions fall where the
reference's detector (Filter::detectLowQualityRegions) puts them for the construction.  That detector restarts its rolling sum
from zero behind a region: the next region begins at once, and it ends only where a window has gained (33 + quality) * window
over the window it restarted on.  With 'I' and '#' (38 apart) no window of 100 ever gains 4 300, so the second region of a read
runs to the read's end; with '~' and '#' (91 apart) regions end, each adjacent to the one before.  Fragments therefore come
from in front of the first region ("r1-") and from behind the last one ("r<regions + 1>-") only, and a two-digit break_no
needs the '~' / '#' reads of many_regions() below."""
import ctypes as C

import numpy as np

from fastplong_amd import abi, synth

GOOD, BAD, TOP = ord("I"), ord("#"), ord("~")


def read(name, segs, seed, strand=b"+", good=GOOD, adapter_at=None):
    """(name, bases, strand, qualities): segs = [(length, good?)]; adapter_at: where the start adapter is written into the bases"""
    rng = np.random.default_rng(seed)
    n = sum(a for a, _ in segs)
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    if adapter_at is not None:
        ad = np.frombuffer(synth.START_ADAPTER.encode(), np.uint8)
        s[adapter_at:adapter_at + len(ad)] = ad
    q = np.concatenate([np.full(a, good if g else BAD, np.uint8) for a, g in segs]) if segs else np.zeros(0, np.uint8)
    return name, s.tobytes(), strand, q.tobytes()


def many_regions(name, gap, k, seed):
    """a read of '~' and '#' whose break regions (window 100, quality 10) lie back to back: k + 1 bad stretches of 100"""
    segs = [(150, 1), (100, 0), (21, 1)]
    for _ in range(k):
        segs += [(100, 0), (gap, 1)]
    segs[-1] = (150, 1)
    return read(name, segs, seed, good=TOP)


def text_of(reads):
    return b"".join(b"%s\n%s\n%s\n%s\n" % r for r in reads)


def csr_of(reads):
    return synth.pack([(np.frombuffer(r[1], np.uint8), np.frombuffer(r[3], np.uint8)) for r in reads])


BREAK_MASK = dict(break_enabled=1, break_window=100, break_quality=10, mask_enabled=1, mask_window=30, mask_quality=10,
                  unqualified_percent_limit=90, n_base_percent_limit=95)
MASK_ONLY = dict(mask_enabled=1, mask_window=30, mask_quality=10, unqualified_percent_limit=90, n_base_percent_limit=95)
BREAK_ONLY = dict(break_enabled=1, break_window=100, break_quality=10, unqualified_percent_limit=90, n_base_percent_limit=95)


def names_case():
    """break_no of one and two digits, both split kinds with a break_no, a one-byte name, a name with a space"""
    twelve = []
    for i in range(12):
        twelve.append((150, 1))
        if i < 11:
            twelve.append((120, 0))
    return [
        read(b"@twelve stretches", twelve, 1),
        many_regions(b"@nine", 59, 7, 2),   # eight regions: its tail is "r9-"
        many_regions(b"@ten", 62, 8, 3),    # nine regions: "r10-"
        read(b"@", [(400, 1), (120, 0), (300, 1)], 4),
        read(b"@adapter in the middle", [(200, 1), (120, 0), (700, 1), (120, 0), (200, 1)], 5, strand=b"+adapter in the middle",
             adapter_at=650),
        read(b"@plain read/1 with spaces", [(500, 1)], 6),
    ]


def masks_case():
    """mask regions that touch a fragment's first base, its last base, lie back to back, and cover a whole fragment"""
    return [
        read(b"@first", [(40, 0), (25, 1)], 11),             # one region from offset 0; too little left for a second
        read(b"@last", [(400, 1), (40, 0)], 12),             # one region up to the last base
        read(b"@back to back", [(200, 1), (35, 0), (200, 1)], 13),  # the second region begins where the first ends
        read(b"@whole", [(60, 0)], 14),                      # all N: fails
        read(b"@clean", [(333, 1)], 15),
        read(b"@broken and masked", [(300, 1), (120, 0), (200, 1), (40, 0)], 16),
    ]


def forced_case(lengths=(1021, 1022, 1023, 1024, 1025)):
    return [read(b"@len %d" % n, [(n, 1)], 20 + n) for n in lengths]


def scan_case(n=1100):
    """n reads of 300 bases with one break each"""
    return [read(b"@s%d" % i, [(140, 1), (120, 0), (40, 1)], 1000 + i) for i in range(n)]


def stripes_case():
    """more than 3 x 49 152 bytes of output"""
    return [read(b"@stripe %d" % i, [(2500 + 17 * i, 1), (40, 0)], 3000 + i) for i in range(32)]


def all_fail_case():
    return [read(b"@bad %d" % i, [(60 + i, 0)], 40 + i) for i in range(5)]


# ---- the host formatter ----
def load_hostlib():
    from tests import gzcheck

    L = gzcheck.load_hostlib()
    L.fplh_format_batch_fragments.restype = C.c_int
    L.fplh_format_batch_fragments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    return L


def host_format(L, tmp_path, text, res, frags, regs):
    """fplh_format_batch_fragments over the text as the host's reader takes it -> the bytes of --out"""
    if len(res) == 0:
        return b""
    p = tmp_path / "in.fq"
    p.write_bytes(text)
    b = L.fplh_batch_read(str(p).encode(), 2 ** 62, 2 ** 30)
    assert b and L.fplh_batch_n(b) == len(res)
    res, frags, regs = np.ascontiguousarray(res), np.ascontiguousarray(frags), np.ascontiguousarray(regs)
    out, n = C.c_void_p(), C.c_uint64()
    assert L.fplh_format_batch_fragments(b, res.ctypes.data, frags.ctypes.data, len(frags), regs.ctypes.data, len(regs), 1, C.byref(out),
                                         C.byref(n), None, None) == 0
    s = C.string_at(out, n.value)
    L.fplh_free(out)
    L.fplh_batch_free(b)
    return s


def csr_slices(reads, res, frags, regs):
    """the CSR batch fpl_emit_batch_device must make of a sorted fragment list, sliced in Python: offsets, src, kind, break_no,
    bases with their N, qualities"""
    off, src, kind, brk, seq, qual = [0], [], [], [], [], []
    for f in frags:
        r = int(f["read"])
        if f["code"] != abi.FPL_PASS_FILTER or res[r]["dropped"]:
            continue
        a, n = int(f["start"]), int(f["len"])
        s = bytearray(reads[r][1][a:a + n])
        for g in regs[int(f["region_first"]):int(f["region_first"]) + int(f["region_count"])]:
            x = int(g["start"]) - a
            if x < 0 or x >= n:
                continue
            m = min(int(g["len"]), n - x)
            s[x:x + m] = b"N" * m
        seq.append(bytes(s))
        qual.append(reads[r][3][a:a + n])
        off.append(off[-1] + n)
        src.append(r)
        kind.append(int(f["kind"]))
        brk.append(int(f["break_no"]))
    return off, src, kind, brk, b"".join(seq), b"".join(qual)


def first_of(frags, n_reads):
    """FragmentList::index (host/format.cpp): first[r] = fragments of the reads in front of r"""
    first = np.zeros(n_reads + 1, np.int64)
    np.add.at(first, frags["read"][frags["read"] < n_reads].astype(np.int64) + 1, 1)
    return np.cumsum(first)


def inflate_stripes(data, want):
    """BGZF blocks of a batch: every block is a gzip member every inflater takes, holds exactly its stripe of 49 152 bytes of the
    text (the last one what is left), and the concatenation is `want`"""
    from fastplong_amd import bgzf
    from tests import gzcheck

    _, offs = bgzf.blocks(data)
    ends = offs[1:] + [len(data)]
    assert len(offs) == (len(want) + 49151) // 49152
    for k, (a, b) in enumerate(zip(offs, ends)):
        stripe = want[49152 * k:49152 * (k + 1)]
        assert gzcheck.inflate_all(data[a:b], len(stripe)) == stripe, k


def normal(frags, regs):
    """a sorted fragment list without what the order of k_break_mask's waves decides: the records with region_first cleared, and
    the regions in the fragments' order"""
    f = frags.copy()
    f["region_first"] = 0
    r = [regs[int(a):int(a) + int(n)].tobytes() for a, n in zip(frags["region_first"], frags["region_count"])]
    return f.tobytes(), b"".join(r)
