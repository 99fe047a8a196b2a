"""The streams of the single-member inflate tests (csrc/gzip_inflate.h), shared by the emulator test and the device test, the
window loop a caller of fpl_inflate_gzip runs, and the rules of the comparison.  The yardstick is Python's zlib, never the code
under test.

A member goes through the call window by window: `window` compressed bytes from the byte of the bit where the call before ended,
the last 32 KiB made so far as the dictionary.  A window must hold at least one whole deflate block, so the parameterised streams
are written with small blocks (memLevel 4: 1024 symbols a block, or flushes every few KB) and go through windows of 16 KiB with
chunks of 1 KiB and 4 KiB; the same levels at zlib's default memLevel (blocks of up to 16384 symbols) go through 64 KiB windows.

  list (a) "zlib writes these": every window status 0, the member's bytes and every window's CRC-32 equal zlib's, nothing refused.
  list (b) "must not be believed": whatever comes back with status 0 is a prefix of what zlib makes of the same bytes, and a
           member reported complete is one zlib takes to its end, with the same bytes.

describe() is a small deflate reader of its own (block types, their distance codes, the largest distance, the 258-at-1 matches):
what a stream's name promises is checked with it on the CPU (tests/test_gzip_inflate_emu.py)."""
import json
import os
import zlib

import numpy as np

from fastplong_amd import synth
from tests import bgzf_cases
from tests.bgzf_cases import (CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LIT, LEN_BASE, LEN_EXTRA, Bits, canonical, dynamic_block,
                              fixed_block, stored_block)

WINDOW = 16384
CHUNKS = (1024, 4096)

_text = {}


def text(n, seed=1):
    """n bytes of FASTQ text of synthetic reads"""
    if seed not in _text:
        seq, qual, off = synth.ont_like(260, seed=seed, median_len=1500)
        _text[seed] = synth.to_fastq(seq, qual, off)
    t = _text[seed]
    assert len(t) >= n, (len(t), n)
    return t[:n]


def raw(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, every=0, flush=zlib.Z_SYNC_FLUSH, end=zlib.Z_FINISH, zdict=None):
    kw = {} if zdict is None else {"zdict": zdict}
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy, **kw)
    if not every:
        return c.compress(data) + c.flush(end)
    out = b""
    for i in range(0, len(data), every):
        out += c.compress(data[i:i + every]) + c.flush(flush)
    return out + c.flush(end)


class Case:
    def __init__(self, name, comp, chunk, window=WINDOW, zdict=b"", out_short=0, must=None):
        self.name, self.comp, self.chunk, self.window, self.zdict, self.out_short = name, comp, chunk, window, zdict, out_short
        self.must = must or {}  # what describe() has to find in it
        self.data, self.whole = zlib_says(comp, zdict)

    def __repr__(self):
        return "Case(%s, %d -> %d, chunk %d, window %d)" % (self.name, len(self.comp), len(self.data), self.chunk, self.window)


def zlib_says(comp, zdict=b""):
    """(what zlib makes of the stream, fed in small pieces so that nothing in front of a fault is lost; did it reach the end)"""
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    out = []
    try:
        for i in range(0, len(comp), 64):
            out.append(d.decompress(comp[i:i + 64]))
            if d.eof:
                break
    except zlib.error:
        return b"".join(out), False
    return b"".join(out), d.eof


# ---------------------------------------------------------------- hand-made blocks (the writers of tests/bgzf_cases.py)
LIT_LENS = [9] * 256 + [5] * 2 + [6] * 28  # a complete code over the 286 symbols
DIST_LENS = [4] * 2 + [5] * 28             # ... and over the 30 distances


def tokens_block(bw, tokens, last=0, dist_lens=DIST_LENS):
    """one dynamic block of literals (bytes) and matches ((length, distance))"""
    c = dynamic_block(bw, LIT_LENS, dist_lens, last=last)
    for t in tokens:
        if isinstance(t, tuple):
            c.match(*t)
        else:
            c.lits(t)
    c.eob()


def far_matches(seed):
    """literal text in small blocks, then matches that reach 20 .. 32 KiB back -- 32768 exactly among them -- in small blocks"""
    rng = np.random.default_rng(seed)
    bw, t = Bits(), text(60000, 2)
    for i in range(0, len(t), 1500):
        tokens_block(bw, [t[i:i + 1500]])
    n_out = len(t)
    while n_out < 260000:
        toks = []
        for _ in range(60):
            dist = 32768 if rng.integers(4) == 0 else int(rng.integers(20480, 32769))
            length = 258 if rng.integers(5) == 0 else int(rng.integers(3, 259))
            toks += [bytes(rng.integers(33, 90, int(rng.integers(0, 4)), dtype=np.uint8)), (length, dist)]
            n_out += len(toks[-2]) + length
        tokens_block(bw, toks)
    tokens_block(bw, [b"end\n"], last=1)
    return bw.done()


def long_run():
    """one byte, then 258-at-distance-1 matches in blocks of 300: the run crosses chunk cuts, markers are copied by overlapping matches"""
    bw = Bits()
    tokens_block(bw, [text(3000, 3)])
    for _ in range(4):
        tokens_block(bw, [b"A"] + [(258, 1)] * 300)
    tokens_block(bw, [text(2000, 3)], last=1)
    return bw.done()


def odd_distance_codes():
    """text; a block whose distance code is a single 1-bit code (distance symbol 9: 25 .. 32); one with no distance code at all"""
    bw, t = Bits(), text(30000, 4)
    for i in range(0, 24000, 1500):
        tokens_block(bw, [t[i:i + 1500]])
    for k in range(8):
        tokens_block(bw, [t[24000 + 300 * k:24300 + 300 * k], (40, 25), b"xy", (7, 32)], dist_lens=[0] * 9 + [1])
        tokens_block(bw, [t[26400 + 300 * k:26700 + 300 * k]], dist_lens=[0])
    tokens_block(bw, [b"end\n"], last=1)
    return bw.done()


def final_in_first_byte(data):
    """zlib's blocks, a stored block as padding, and a final block of ten bits that starts in the last byte of one 4 KiB chunk and
    ends in the first byte of the next (so for 1 KiB chunks too)"""
    z = raw(data, 6, 4, end=zlib.Z_FULL_FLUSH)
    bw = Bits()
    bw.raw(z)
    stored_block(bw, b"p" * ((4096 + 1 - 7 - len(z)) % 4096), last=0)
    fixed_block(bw, last=1).eob()
    out = bw.done()
    assert len(out) % 4096 == 1
    return out


def spliced():
    """dynamic, fixed and stored stretches, each its own compressor closed with Z_FULL_FLUSH (so they concatenate), the fixed and
    stored ones several chunks long and flushed every 3000 bytes: chunks without any dynamic header, and chunks that must run on"""
    t = text(300000, 5)
    parts = [raw(t[:60000], 6, 4, end=zlib.Z_FULL_FLUSH),
             raw(t[60000:90000], 6, 4, zlib.Z_FIXED, every=3000, end=zlib.Z_FULL_FLUSH),
             raw(t[90000:150000], 6, 4, end=zlib.Z_FULL_FLUSH),
             raw(t[150000:175000], 0, 4, every=3000, end=zlib.Z_FULL_FLUSH),
             raw(t[175000:230000], 9, 4, end=zlib.Z_FULL_FLUSH),
             raw(t[230000:245000], 6, 4, zlib.Z_FIXED, every=3000, end=zlib.Z_FULL_FLUSH),
             raw(t[245000:], 6, 4)]
    return b"".join(parts)


_lists = {}


def zlib_cases():
    """list (a)"""
    if "a" in _lists:
        return _lists["a"]
    t = text(300000, 1)
    streams = [("level%d" % lv, raw(t, lv, 4), {"dynamic": 20}) for lv in (1, 6, 9)]
    streams += [("spliced", spliced(), {"dynamic": 20, "fixed": 10, "stored": 8}),
                ("sync_flush", raw(text(250000, 6), 6, 8, every=4000), {"dynamic": 40, "stored": 40}),
                ("far_matches", far_matches(11), {"dynamic": 40, "dist32768": 20, "max_dist": 32768}),
                ("zlib_run", raw(text(80000, 7) + b"A" * 120000 + text(90000, 8), 6, 4), {"dynamic": 10, "run258": 300}),
                ("long_run", long_run(), {"dynamic": 6, "run258": 1200}),
                ("odd_distance_codes", odd_distance_codes(), {"single_dist": 8, "no_dist": 8}),
                ("empty", raw(b""), {}), ("one_byte", raw(b"x"), {}), ("bytes_70000", raw(text(70000, 9), 6, 4), {"dynamic": 4}),
                ("final_in_first_byte", final_in_first_byte(text(200000, 10)), {"dynamic": 10, "fixed": 1, "last_block_bits": 10})]
    cases = [Case("%s/c%d" % (n, ch), comp, ch, must=must) for n, comp, must in streams for ch in CHUNKS]
    cases += [Case("level%d_mem8/c%d" % (lv, ch), raw(t, lv), ch, window=65536, must={"dynamic": 3}) for lv in (1, 6, 9) for ch in CHUNKS]
    for c in cases:
        assert c.whole, c.name
    _lists["a"] = cases
    return cases


def big_case():
    """8 MB of text at the default sizes: chunk_bytes 0, one window"""
    if "big" not in _lists:
        t = text(400000, 1)
        data = b"".join(t[(7919 * i) % 1000:] for i in range(21))[:8 << 20]
        assert len(data) == 8 << 20
        _lists["big"] = Case("big_8MB", raw(data, 6), 0, window=1 << 26)
    return _lists["big"]


def doubt_cases(seed=3):
    """list (b)"""
    if "b" in _lists:
        return _lists["b"]
    rng = np.random.default_rng(seed)
    base = raw(text(70000, 9), 6, 4)
    inner = raw(text(60000, 2), 6, 4)
    embedded = raw(text(20000, 3) + inner + text(20000, 4), 0, 4, every=3000)
    cases = [Case("embedded_stream/c%d" % ch, embedded, ch) for ch in CHUNKS]
    for k in range(24):
        b = bytearray(base)
        at = int(rng.integers(0, 8 * len(b)))
        b[at >> 3] ^= 1 << (at & 7)
        cases.append(Case("flip/%d" % at, bytes(b), CHUNKS[k & 1]))
    cases += [Case("cut/%d" % k, base[:len(base) - k], 1024) for k in range(1, 41)]
    za, zb = text(32768, 5), text(32768, 6)
    with_dict = raw(text(70000, 9), 6, 4, zdict=za)
    cases += [Case("wrong_dict/c%d" % ch, with_dict, ch, zdict=zb) for ch in CHUNKS]
    cases += [Case("right_dict/c%d" % ch, with_dict, ch, zdict=za) for ch in CHUNKS]
    cases += [Case("out_cap_short/c%d" % ch, base, ch, out_short=1) for ch in CHUNKS]
    _lists["b"] = cases
    return cases


# ---------------------------------------------------------------- the caller's loop
class Run:
    def __init__(self, case):
        self.case, self.bit, self.out, self.windows, self.refused, self.final, self.done = case, 0, b"", [], 0, False, False
        self.log = []  # every result that came back, refused ones too: RECORD_FIELDS of each

    def job(self):
        c, at = self.case, self.bit >> 3
        cap = max(0, len(c.data) + 64 - c.out_short - len(self.out)) if not c.out_short else max(0, len(c.data) - c.out_short - len(self.out))
        return dict(comp=c.comp[at:at + c.window], start_bit=self.bit & 7, dict=(c.zdict + self.out)[-32768:], out_cap=cap, chunk_bytes=c.chunk)

    def take(self, r):
        """one result (rc, status, out_bytes, end_bit, crc32, final, data)"""
        self.log.append([int(r[k]) for k in RECORD_FIELDS])
        stuck = r["rc"] == 0 and r["status"] == 0 and not r["final"] and r["end_bit"] <= (self.bit & 7)
        if r["rc"] != 0 or r["status"] != 0 or stuck:
            self.refused, self.done = self.refused + 1, True  # (the caller inflates the rest itself)
            return
        assert len(r["data"]) == r["out_bytes"] and r["crc32"] == zlib.crc32(r["data"]), self.case.name
        self.windows.append(r)
        self.out += r["data"]
        self.bit = 8 * (self.bit >> 3) + r["end_bit"]
        assert self.bit <= 8 * len(self.case.comp), self.case.name
        self.final = self.done = bool(r["final"])


def run_members(cases, batch_call, max_rounds=4000):
    """every case through its windows; batch_call(list of jobs) -> list of results.  The cases advance in rounds, so that an
    emulator that is a program of its own is started once a round, not once a window."""
    runs = [Run(c) for c in cases]
    for _ in range(max_rounds):
        live = [r for r in runs if not r.done]
        if not live:
            break
        jobs = []
        for r in live:
            j = r.job()
            if len(j["comp"]) == 0:  # nothing left to hand over: a stream cut at a block's end
                r.refused, r.done = r.refused + 1, True
            else:
                jobs.append((r, j))
        if jobs:
            for (r, _), res in zip(jobs, batch_call([j for _, j in jobs])):
                r.take(res)
    assert all(r.done for r in runs)
    return runs


def check_zlib_list(runs):
    for r in runs:
        assert r.final and r.refused == 0, (r.case.name, r.refused, len(r.out), len(r.case.data))
        assert r.out == r.case.data, r.case.name
        assert r.bit + 7 >> 3 == len(r.case.comp), r.case.name


def check_doubt_list(runs):
    for r in runs:
        want = r.case.data
        n = min(len(want), len(r.out))
        assert r.out[:n] == want[:n], r.case.name
        if r.final:
            assert r.case.whole and r.out == want, r.case.name
        if r.case.out_short:
            assert len(r.out) <= len(want) - r.case.out_short and not r.final, r.case.name


# ---------------------------------------------------------------- what the decoder answers, pinned
# tests/golden/gzip_window_results.json: the decoder's own answers (this project's code on the emulator, written with
# `python -m tests.gzip_cases --record`), so that a change which moves a check, and with it a status or the end of a window, shows.
# Names and integers only: the streams are rebuilt from their seeds.
RECORD_FIELDS = ("rc", "status", "out_bytes", "end_bit", "crc32", "final", "chunks")
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gzip_window_results.json")


def stream_cases():
    """the hand-made and the refused streams of the BGZF tests (tests/bgzf_cases.py), for this decoder"""
    return bgzf_cases.refuse_cases() + bgzf_cases.hand_cases()


def stream_jobs():
    """... each as one window from bit 0 with no dictionary"""
    return [dict(comp=c.payload, start_bit=0, dict=b"", out_cap=len(c.data) + 64, chunk_bytes=1024) for c in stream_cases()]


def window_results(doubt_runs, stream_res):
    """the runs of doubt_cases() and the results of stream_jobs() in the form of the record"""
    names = [r.case.name for r in doubt_runs]
    assert len(set(names)) == len(names)
    return {"fields": list(RECORD_FIELDS),
            "doubt": {"names": names, "windows": [r.log for r in doubt_runs]},
            "streams": {"names": [c.name for c in stream_cases()], "results": [[int(r[k]) for k in RECORD_FIELDS] for r in stream_res]}}


def check_doubt_record(doubt_runs):
    want = json.load(open(RECORD))
    assert want["fields"] == list(RECORD_FIELDS)
    assert [r.case.name for r in doubt_runs] == want["doubt"]["names"]
    for r, w in zip(doubt_runs, want["doubt"]["windows"]):
        assert r.log == w, (r.case.name, r.log, w)


def check_stream_record(stream_res):
    want = json.load(open(RECORD))
    assert want["fields"] == list(RECORD_FIELDS)
    cases = stream_cases()
    assert [c.name for c in cases] == want["streams"]["names"] and len(stream_res) == len(cases)
    for c, r, w in zip(cases, stream_res, want["streams"]["results"]):
        assert [int(r[k]) for k in RECORD_FIELDS] == w, (c.name, r, w)


def check_stream_rules(stream_res):
    """what holds by rule for the results of stream_jobs(): where this decoder and the BGZF one must differ, and where not"""
    by = {c.name: (c, r) for c, r in zip(stream_cases(), stream_res)}
    c, r = by["refuse/single_distance_code"]  # zlib's incomplete distance set: taken here, refused there
    assert r["rc"] == 0 and r["status"] == 0 and r["final"] and r["data"] == c.data and len(c.data) > 0, r
    c, r = by["refuse/distance_before_start"]  # the marker has nothing to resolve against
    assert r["rc"] == 0 and r["status"] != 0 and r["data"] == b"", r
    hand = [(c, r) for c, r in by.values() if c.name.startswith("hand/")]
    assert len(hand) >= 15
    for c, r in hand:
        assert c.zlib_ok and r["rc"] == 0 and r["status"] == 0 and r["final"] and r["data"] == c.data, (c.name, r["status"])
        assert r["crc32"] == zlib.crc32(c.data) and r["end_bit"] + 7 >> 3 == len(c.payload), c.name


def record(batch_call):
    """writes the record: to be run on the emulator, at a commit whose decoder is the one to hold on to"""
    got = window_results(run_members(doubt_cases(), batch_call), batch_call(stream_jobs()))
    with open(RECORD, "w") as f:
        f.write("{\n \"fields\": %s,\n" % json.dumps(got["fields"]))
        for key, rows in (("doubt", "windows"), ("streams", "results")):
            f.write(" \"%s\": {\n  \"names\": %s,\n  \"%s\": [\n" % (key, json.dumps(got[key]["names"]), rows))
            f.write(",\n".join("   " + json.dumps(v, separators=(",", ":")) for v in got[key][rows]))
            f.write("\n  ]\n }%s\n" % ("," if key == "doubt" else ""))
        f.write("}\n")
    return got


# ---------------------------------------------------------------- a deflate reader of its own
def describe(comp):
    """-> counts: blocks by type, the distance codes of the dynamic ones, the largest distance, matches of 32768, of 258 at 1,
    the bits of the last block and where every block ends"""
    pos = 0

    def take(n):
        nonlocal pos
        v = (int.from_bytes(comp[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):
        return {(l, c): s for s, (c, l) in canonical(lens).items()}

    def sym(tab):
        nonlocal pos
        code = 0
        for l in range(1, 16):
            code = (code << 1) | take(1)
            if (l, code) in tab:
                return tab[(l, code)]
        raise ValueError("no code")

    d = dict(dynamic=0, fixed=0, stored=0, single_dist=0, no_dist=0, max_dist=0, dist32768=0, run258=0, last_block_bits=0, out=0,
             ends=[])  # ends: (the bit behind the block, the bytes made up to there) of every block
    fixed = (table(FIXED_LIT), table(FIXED_DIST))
    while True:
        at = pos
        last, kind = take(1), take(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            assert take(16) == n ^ 0xFFFF
            pos += 8 * n
            d["stored"] += 1
            d["out"] += n
        else:
            if kind == 1:
                lit, dist = fixed
                d["fixed"] += 1
            else:
                assert kind == 2
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = take(3)
                ct, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = sym(ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    elif s == 17:
                        lens += [0] * (3 + take(3))
                    else:
                        lens += [0] * (11 + take(7))
                assert len(lens) == hlit + hdist
                dl = lens[hlit:]
                used = [l for l in dl if l]
                d["dynamic"] += 1
                d["no_dist"] += not used
                d["single_dist"] += used == [1]
                lit, dist = table(lens[:hlit]), table(dl)
            while True:
                s = sym(lit)
                if s < 256:
                    d["out"] += 1
                elif s == 256:
                    break
                else:
                    k = s - 257
                    length = LEN_BASE[k] + take(LEN_EXTRA[k])
                    ds = sym(dist)
                    dd = DIST_BASE[ds] + take(DIST_EXTRA[ds])
                    d["max_dist"] = max(d["max_dist"], dd)
                    d["dist32768"] += dd == 32768
                    d["run258"] += length == 258 and dd == 1
                    d["out"] += length
        d["ends"].append((pos, d["out"]))
        if last:
            d["last_block_bits"] = pos - at
            d["end_bit"] = pos
            return d


if __name__ == "__main__":
    import sys

    from tests.emu_gzip import build as emu

    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.gzip_cases --record")
    emu.build()
    got = record(emu.inflate)
    print("%s: %d windows of %d runs, %d streams" % (RECORD, sum(len(w) for w in got["doubt"]["windows"]), len(got["doubt"]["names"]),
                                                     len(got["streams"]["names"])))
