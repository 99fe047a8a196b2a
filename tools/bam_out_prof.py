"""The BAM record kernels (k_bamout_layout / k_bamout_compose, fastplong_amd/csrc/bam_emit.h) and the BGZF block kernels behind them
on one resident text batch, for `rocprofv3 --kernel-trace --stats -- python tools/bam_out_prof.py [Mbases] [--bam]`: reads of 10 kb
with ONT-like qualities, every read passing whole, submitted three times through Engine.submit_text(gzip=True).  Without --bam
the batch is the BGZF FASTQ form (Engine.set_gzip_framing: k_gz_layout / k_gz_compose), the form to compare with IN THE SAME
SESSION; with it the records' form (Engine.set_gzip_records).

Bytes k_bamout_compose moves per base: 2 read (base, quality), 1.5 written = 3.5; the roofline printed is that count at 8 TB/s,
next to the whole design's (compose as above, k_gz_block_bgzf reads the 1.5 and writes the coded block, k_gz_compact reads and
writes that again).  The wall time printed holds the upload, the parse, the per-read kernels and the bytes' way back as well.

`--mods [Mbases]` / `--mods --tags-only [Mbases]`: the --keep_mods leg (fastplong_amd/csrc/bam_mods.h).  A resident BAM batch of
ONT-like reads with adapters (median 5 kb, a middle adapter in three of ten) that carry generated modification calls -- C+mh? at
CpGs, A+a. at every fourth A, a sparse N+n group --, submitted three times through Engine.submit_bam(gzip=True) with set_bam_tags
and set_bam_mods (k_bam_tags_mods, k_bam_mods_plan, k_bamout_compose_bam_mods), or with --tags-only with set_bam_tags alone
(k_bam_tags, k_bamout_compose_bam_tags): the form to compare with in the same session.

`--moves [Mbases]` / `--moves --tags-only [Mbases]`: the --keep_moves leg (fastplong_amd/csrc/bam_moves.h).  The --mods batch shape
with move tables of about 2 entries a base (stride 6, 1 to 3 entries per base), ts and ns in place of the modification calls,
with set_bam_tags and set_bam_moves (k_bam_tags_moves, k_bam_moves_plan, k_bamout_compose_bam_moves) or, with --tags-only, with
set_bam_tags alone.  It prints the table bytes of the candidate records: what k_bam_moves_plan reads once."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastplong_amd import abi, bgzf, engine  # noqa: E402


def main(mbases=1000, L=10_000, bam=False):
    rng = np.random.default_rng(1)
    n = max(1, mbases * 1_000_000 // L)
    pool = 64  # distinct reads; the kernels do not care that reads repeat
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes() for _ in range(pool)]
    quals = [(np.clip(rng.normal(18, 8, L), 1, 60).astype(np.uint8) + 33).tobytes() for _ in range(pool)]
    text = b"".join(b"@read%d runid=abc ch=%d\n%s\n+\n%s\n" % (i, i % 512, seqs[i % pool], quals[i % pool]) for i in range(n))
    eng = engine.Engine(abi.FplOptions.default(adapter_enabled=0, qual_filter=0, length_filter=0), "", "", device=0, max_cycles=L)
    if bam:
        eng.set_gzip_records(True)
    else:
        eng.set_gzip_framing(True)
    buf = eng.pinned_array(len(text))
    buf[:] = np.frombuffer(text, np.uint8)
    for k in range(3):
        t0 = time.time()
        eng.submit_text(buf, gzip=True)
        info, res, lines, out = eng.wait_text()
        dt = time.time() - t0
        print("batch %d: %.3f s wall, %d reads, %.3f Gbases, text %d bytes -> %s in BGZF blocks: %d bytes (%.3f of the text)" % (
            k, dt, info["n_reads"], info["n_bases"] / 1e9, len(text), "BAM records" if bam else "FASTQ", len(out), len(out) / len(text)))
    composed, pos = 0, 0
    while pos < len(out):  # block after block: ISIZE says what went in (the tests inflate; 0.9 GB here would take minutes)
        size = bgzf.block_len(out, pos)
        composed += int.from_bytes(out[pos + size - 4:pos + size], "little")
        pos += size
    n_bases = n * L
    print("composed: %d bytes in front of the block kernels (%.3f per base)" % (composed, composed / n_bases))
    if bam:
        print("k_bamout_compose moves 3.5 bytes a base: at 8 TB/s %.3f ms" % (3.5 * n_bases / 8e12 * 1e3))
        moved = 2 * n_bases + 2 * composed + 4 * len(out)
    else:
        moved = 3 * composed + 4 * len(out)
    print("bytes the design moves: %.2f per base; at 8 TB/s: %.3f ms" % (moved / n_bases, moved / 8e12 * 1e3))
    eng.close()


def mods_main(mbases=100, mods=True, moves=None):
    from fastplong_amd import synth
    from tests import bam_mod_cases as mc
    from tests import bam_move_cases as vc
    from tests import bamio, hostio
    L = 5000
    pool = 256  # distinct reads: generating the calls in Python is the slow part; the kernels do not care that reads repeat
    rng = np.random.default_rng(2)
    seq, qual, off = synth.ont_like(pool, seed=3, median_len=L, p_middle=0.3)
    encoded = []
    for i, (_, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        occ = mc.occurrences(codes, b"C")
        cpg = [k for k, p in enumerate(occ) if p + 1 < len(codes) and codes[p + 1] == 4]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", mc.every(codes, b"A", 4, 3)),
                (b"N+n", mc.every(codes, b"N", 997, 11))]
        tags, table = mc.fields_of(codes, spec, rng) if moves is None else None, 0
        if moves is not None:
            table = int(rng.integers(1, 4, len(codes)).sum()) + 2
            tags = vc.fields_of(vc.table(len(codes), table, rng, lead=2), ts=(b"i", 10 + i))
        encoded.append((len(codes), bamio.encode_record(b"read%d" % i, 4, codes, q, tags=tags), table))
    n = max(1, mbases * 1_000_000 // L)
    raw, starts, offs = bytearray(), [], [0]
    for i in range(n):
        starts.append(len(raw))
        offs.append(offs[-1] + encoded[i % pool][0])
        raw += encoded[i % pool][1]
    starts, offs = np.array(starts, np.uint64), np.array(offs, np.uint64)
    eng = engine.Engine(abi.FplOptions.default(cut_front=1, cut_tail=1, cut_front_window=5, cut_tail_window=5), synth.START_ADAPTER,
                        synth.END_ADAPTER, device=0, max_cycles=int(max(e[0] for e in encoded)) + 64)
    eng.set_gzip_records(True)
    eng.set_bam_tags(True)
    eng.set_bam_mods(mods and moves is None)
    if moves is not None:
        eng.set_bam_moves(moves)
    buf = eng.pinned_array(len(raw))
    buf[:] = np.frombuffer(bytes(raw), np.uint8)
    res = np.zeros(n, abi.RESULT_DTYPE)
    for k in range(3):
        t0 = time.time()
        eng.submit_bam(buf, starts, offs, res=res, gzip=True)
        out = eng.wait()
        print("batch %d (%s): %.3f s wall, %d records of %d bytes, %.3f Gbases -> %d bytes of BGZF blocks; %d split reads" % (
            k, "--keep_moves" if moves else "--keep_mods" if mods and moves is None else "--keep_tags alone", time.time() - t0, n, len(raw), int(offs[-1]) / 1e9, len(out), int((res["n_frag"] == 2).sum())))
    print("tag counts: %s; modification counts: %s" % (eng.bam_tag_stats(), eng.bam_mod_stats()))
    if moves is not None:
        whole = (res["n_frag"] == 1) & (res["code"][:, 0] == 0) & (res["frag_start"][:, 0] == 0) & (res["frag_len"][:, 0] == np.diff(offs.astype(np.int64)))
        cand = ~whole & (res["dropped"] == 0) & ((res["code"][:, 0] == 0) | ((res["n_frag"] == 2) & (res["code"][:, 1] == 0)))
        table_bytes = int(sum(encoded[i % pool][2] for i in np.flatnonzero(cand)))
        print("move counts: %s; %d candidate records, their tables %d bytes: read once at 8 TB/s in %.4f ms" % (
            eng.bam_move_stats(), int(cand.sum()), table_bytes, table_bytes / 8e12 * 1e3))
    eng.close()


if __name__ == "__main__":
    flags = ("--bam", "--mods", "--moves", "--tags-only")
    args = [a for a in sys.argv[1:] if a not in flags]
    if "--moves" in sys.argv[1:]:
        mods_main(*(int(a) for a in args[:1]), mods=False, moves="--tags-only" not in sys.argv[1:])
    elif "--mods" in sys.argv[1:]:
        mods_main(*(int(a) for a in args[:1]), mods="--tags-only" not in sys.argv[1:])
    else:
        main(*(int(a) for a in args[:1]), bam="--bam" in sys.argv[1:])
