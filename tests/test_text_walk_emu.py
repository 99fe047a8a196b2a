"""The resident FASTQ text walk (fastplong_amd/csrc/text_walk.h: k_tw_place_tail, k_tw_count, k_tw_fill, k_tw_records,
k_tw_verdict, k_tw_names around k_text_scan / k_text_offsets / k_text_gather) and the six kernels of text_parse.h on the
emulator, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu_textwalk): every buffer has
exactly its promised size, so a run that ends clean also never left one.

What is expected never comes from the kernels: window() below is the model -- split at "\\n", groups of four, the three checks --
over [tail | data] as Python bytes, and the tail is what it leaves behind the last group.  A position p of that stream is byte
lo + p of the slot's buffer (lo = tail capacity - len(tail); the driver reports it)."""
import re

import numpy as np
import pytest

from tests.emu_textwalk import build as emu

OK, BLOCK, IRREGULAR, TAIL_ROOM, TOO_MANY, CHAIN, STRAND = range(7)
NONE = emu.NONE
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 300, 4095, 4096, 4097, 9000]
CAP = 32768  # holds any record of the texts whole (the longest is 2 * 9000 bytes and a name)


# ---- the texts ----
def make_records(seed, eol, n=40, first=(17, 0, 16, 1, 15)):
    """[(four lines, four line ends)]: every length of LENGTHS at least once, `first` in front (a stretch of short records),
    names with spaces, '@' and '+' as first quality bytes"""
    rng = np.random.default_rng(seed)
    rest = [x for x in LENGTHS if x not in first]
    lens = list(first) + [int(x) for x in rng.permutation(rest + [int(v) for v in rng.choice(LENGTHS, n - len(first) - len(rest))])]
    recs = []
    for i, ln in enumerate(lens):
        s = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, ln)].tobytes()
        q = rng.integers(33, 127, ln).astype(np.uint8)
        if ln:
            q[0] = ord("@") if i % 2 else ord("+")
        ends = [{"lf": b"\n", "crlf": b"\r\n", "mixed": b"\r\n" if rng.integers(0, 2) else b"\n"}[eol] for _ in range(4)]
        name = b"@x" if i % 7 == 3 else b"@r %d" % i if i < 3 else b"@read %d  some text len=%d" % (i, ln)
        recs.append(([name, s, b"+", q.tobytes()], ends))
    return recs


def join(recs):
    return b"".join(l + e for lines, ends in recs for l, e in zip(lines, ends))


def rec_bounds(recs):
    """byte offset of every record's start, and of the end"""
    return np.cumsum([0] + [sum(len(l) + len(e) for l, e in zip(*r)) for r in recs])


# ---- the model ----
def window(buf):
    """one submission over buf = tail + data -> status, records [(name, bases, qualities, four line starts)], the cut, and for a
    refusal the failing record's index in buf (None: the structure) and its position"""
    a = np.frombuffer(buf, np.uint8)
    nl = np.flatnonzero(a == 10)
    n = len(nl) // 4
    cut = int(nl[4 * n - 1]) + 1 if n else 0
    cr = [int(i) for i in np.flatnonzero(a[:-1] == 13) if a[i + 1] != 10][:1]
    lone = cr[0] if cr and cr[0] < cut else None
    recs, bad, strand = [], None, None
    starts = [0] + [int(p) + 1 for p in nl[:4 * n]]
    for r in range(n):
        st = starts[4 * r:4 * r + 4]
        four = [buf[starts[4 * r + i]:starts[4 * r + i + 1] - 1] for i in range(4)]
        four = [l[:-1] if l.endswith(b"\r") else l for l in four]
        good = four[0][:1] == b"@" and four[2][:1] == b"+" and len(four[1]) == len(four[3])
        if not good and bad is None:
            bad = r
        if good and len(four[2]) > 1 and strand is None:
            strand = r
        recs.append((four[0], four[1], four[3], st))
    out = dict(n_lines=len(nl), cut=cut, recs=recs, bad=None, pos=None)
    if lone is not None or (bad is not None and (strand is None or bad < strand)):
        pos = [p for p in (lone, starts[4 * bad] if bad is not None else None) if p is not None]
        return dict(out, status=IRREGULAR, bad=bad, pos=min(pos))
    if strand is not None:
        return dict(out, status=STRAND, bad=strand, pos=starts[4 * strand])
    return dict(out, status=OK)


def tolerant(buf):
    """what stands in for the host's reader on a refused stretch: lines that do not start with '@' are skipped where a name is
    expected (the reference's reader does that), the three lines behind a name are taken as they are -> records [(name, bases,
    qualities)], the bytes behind the last whole record"""
    lines = buf.split(b"\n")
    lines.pop()
    at = np.cumsum([0] + [len(l) + 1 for l in lines])
    strip = lambda l: l[:-1] if l.endswith(b"\r") else l
    recs, i = [], 0
    while True:
        while i < len(lines) and not lines[i].startswith(b"@"):
            i += 1
        if i + 4 > len(lines):
            break
        recs.append((strip(lines[i]), strip(lines[i + 1]), strip(lines[i + 3])))
        i += 4
    return recs, buf[int(at[min(i, len(lines))]):]


def check_ok(r, m, tail, data, seen_before, what):
    """an accepted submission against the model's window over tail + data"""
    assert r["rc"] == 0 and r["status"] == OK and m["status"] == OK, (what, {k: v for k, v in r.items() if not hasattr(v, "__len__")}, m["status"])
    n = len(m["recs"])
    assert r["n_reads"] == n and r["n_lines"] == m["n_lines"] and r["records_seen"] == seen_before + n, what
    assert r["tail_bytes"] == len(tail) + len(data) - m["cut"], what
    assert r["line"].tolist() == [[r["lo"] + p for p in rec[3]] for rec in m["recs"]], what
    assert r["len"].tolist() == [len(rec[1]) for rec in m["recs"]], what
    assert r["off"].tolist() == np.cumsum([0] + [len(rec[1]) for rec in m["recs"]]).tolist(), what
    assert r["name_off"].tolist() == np.cumsum([0] + [len(rec[0]) for rec in m["recs"]]).tolist(), what
    assert r["names"] == b"".join(rec[0] for rec in m["recs"]) and r["name_bytes"] == len(r["names"]), what
    assert r["seq"] == b"".join(rec[1] for rec in m["recs"]) and r["qual"] == b"".join(rec[2] for rec in m["recs"]), what
    assert r["n_bases"] == len(r["seq"]) and r["max_read_len"] == max([len(rec[1]) for rec in m["recs"]] + [0]), what


def stream_ops(pieces, cap=CAP):
    ops = [emu.new(cap)]
    for p in pieces:
        ops += [emu.submit(p), ("tail_get",)]
    return ops


def check_stream(res, text, pieces, what):
    """the results of stream_ops for regular text: every step against the model, the union against the model of the whole"""
    tail, seen, got = b"", 0, []
    for k, p in enumerate(pieces):
        r, t = res[2 * k], res[2 * k + 1]
        m = window(tail + p)
        check_ok(r, m, tail, p, seen, (what, k))
        seen += len(m["recs"])
        got += [rec[:3] for rec in m["recs"]]
        tail = (tail + p)[m["cut"]:]
        assert t == tail, (what, k)
    whole = window(text)
    assert whole["status"] == OK and got == [rec[:3] for rec in whole["recs"]] and tail == text[whole["cut"]:], what
    return tail


TEXTS = {eol: make_records(11 + i, eol) for i, eol in enumerate(("lf", "crlf", "mixed"))}


def run_batches(batches):
    """[(ops, check)] -> one run of the program for all of them"""
    ops = [op for b in batches for op in b[0]]
    res = emu.run(ops)
    at = 0
    for b_ops, check in batches:
        k = sum(1 for op in b_ops if op[0] in ("submit", "whole", "tail_get"))
        check(res[at:at + k])
        at += k
    assert at == len(res)


# ---- case 1 ----
def test_two_submissions_cut_at_every_byte_of_three_records():
    """records 1 .. 3 (0, 16 and 1 bases, short names: every cut costs two submissions) of the text with both kinds of line ends:
    every cut from the last byte of record 0 to the first byte of record 4 -- between '\\r' and '\\n', right behind a record's
    last '\\n', inside each of the four lines"""
    recs = TEXTS["mixed"]
    text, b = join(recs), rec_bounds(recs)
    assert b"\r\n" in text[b[1]:b[4]] and re.search(rb"[^\r]\n", text[b[1]:b[4]])
    batches = []
    for c in range(int(b[1]) - 1, int(b[4]) + 2):
        pieces = [text[:c], text[c:]]
        batches.append((stream_ops(pieces), lambda res, pieces=pieces, c=c: check_stream(res, text, pieces, ("cut", c)) == b"" or pytest.fail("tail")))
    run_batches(batches)


# ---- case 2 ----
def test_tail_lengths_put_the_text_at_every_alignment():
    """the first k bytes of the text as the tail, set from outside, in front of a submission of the rest: lo = CAP - k is at every
    alignment within 16 bytes and on both sides of a 4 KiB block"""
    recs = make_records(5, "mixed", n=16, first=(4097, 17))
    text = join(recs)
    batches = []
    for k in list(range(0, 18)) + [4095, 4096, 4097]:
        def check(res, k=k):
            m = window(text)
            check_ok(res[0], m, text[:k], text[k:], 0, ("tail", k))
            assert res[0]["lo"] == CAP - k and res[1] == b""
        batches.append(([emu.new(CAP), ("tail_set", text[:k]), emu.submit(text[k:]), ("tail_get",)], check))
    run_batches(batches)


# ---- case 3 ----
def test_one_record_across_three_submissions():
    recs = make_records(6, "crlf", n=15, first=(16, 9000, 1))
    text, b = join(recs), rec_bounds(recs)
    c1, c2 = int(b[1]) + 3000, int(b[1]) + 12000  # inside the bases, inside the qualities of the 9000-base record
    pieces = [text[:c1], text[c1:c2], text[c2:]]

    def check(res):
        check_stream(res, text, pieces, "long record")
        assert res[0]["n_reads"] == 1 and res[0]["tail_bytes"] == 3000
        assert res[2]["status"] == OK and res[2]["n_reads"] == 0 and res[2]["tail_bytes"] == 12000 and len(res[3]) == 12000
        assert res[4]["n_reads"] == 14 and res[5] == b""
    run_batches([(stream_ops(pieces), check)])


# ---- case 4 ----
def test_carriage_return_as_a_submissions_last_byte():
    recs = TEXTS["crlf"]
    text, b = join(recs), rec_bounds(recs)
    c = text.index(b"\r\n", int(b[5])) + 1  # between the two
    regular = [text[:c], text[c:]]
    odd = text[:c] + b"A" + text[c:]  # the '\r' now stands inside the name line of record 5, followed by 'A'
    pieces = [odd[:c], odd[c:]]

    def check_odd(res):
        m = window(pieces[0])
        check_ok(res[0], m, b"", pieces[0], 0, "first")  # the '\r' is its last byte: not judged yet
        tail = pieces[0][m["cut"]:]
        assert res[1] == tail and tail.endswith(b"\r")
        m2 = window(tail + pieces[1])
        assert m2["status"] == IRREGULAR and m2["pos"] == len(tail) - 1
        r = res[2]
        assert r["status"] == IRREGULAR and r["n_reads"] == 0 and r["bad_pos"] == m2["pos"], r
        assert r["bad_index"] == (NONE if m2["bad"] is None else 5 + m2["bad"])
        assert res[3] == tail  # the tail is as it was
    run_batches([(stream_ops(regular), lambda res: check_stream(res, text, regular, "cr|lf")), (stream_ops(pieces), check_odd)])


# ---- case 5 ----
def plant(recs, r, kind):
    out = [([*lines], [*ends]) for lines, ends in recs]
    lines, ends = out[r]
    if kind == "blank":
        out.insert(r, ([b""], [b"\n"]))
    elif kind == "cr":
        lines[0] = lines[0][:1] + b"\r" + lines[0][1:]
    elif kind == "plus":
        lines[2] = b"-"
    elif kind == "unequal":
        lines[3] = lines[3] + b"I"
    elif kind == "strand":
        lines[2] = b"+" + lines[0][1:]
    return out


def refusal_script(text, c1, c2, cap, want_status, what, block_status=(), reserve=0):
    """three submissions text[:c1], [c1:c2], [c2:]; the second is refused with want_status.  Then the way on: reserve + resume and
    the two again (reserve > 0), or the refused stretch through tolerant(), the rest resident.  The whole file's records are
    tolerant(text)'s."""
    s1, s2, s3 = text[:c1], text[c1:c2], text[c2:]
    ops = [emu.new(cap), emu.submit(s1), ("tail_get",), emu.submit(s2, block_status), ("tail_get",), emu.submit(s3), ("tail_get",)]
    m1 = window(s1)
    tail = s1[m1["cut"]:]
    if reserve:
        ops += [("reserve", reserve), ("resume",), emu.submit(s2), ("tail_get",), emu.submit(s3), ("tail_get",)]
    else:
        host_recs, rest = tolerant(tail + s2)
        ops += [("tail_set", rest), emu.submit(s3), ("tail_get",)]

    def check(res):
        check_ok(res[0], m1, b"", s1, 0, (what, "first"))
        assert res[1] == tail
        r, m2 = res[2], window(tail + s2)
        assert r["rc"] == 0 and r["status"] == want_status and r["n_reads"] == 0 and r["n_bases"] == 0, (what, r)
        assert r["records_seen"] == len(m1["recs"]), what
        if want_status in (IRREGULAR, STRAND):
            assert m2["status"] == want_status, (what, m2["status"])
            assert r["bad_index"] == (NONE if m2["bad"] is None else len(m1["recs"]) + m2["bad"]) and r["bad_pos"] == m2["pos"], (what, r, m2["bad"], m2["pos"])
        if want_status == BLOCK:
            assert r["bad_index"] == list(block_status).index(3), what
        if want_status == TAIL_ROOM:
            assert r["tail_bytes"] == len(tail + s2) - m2["cut"] > cap, what
        assert res[3] == tail, what  # the tail is as it was
        assert res[4]["status"] == CHAIN and res[4]["n_reads"] == 0 and res[5] == tail, what
        want_all, end = tolerant(text)
        got = [rec[:3] for rec in m1["recs"]]
        if reserve:
            check_ok(res[6], m2, tail, s2, len(m1["recs"]), (what, "again"))
            t2 = (tail + s2)[m2["cut"]:]
            assert res[7] == t2
            m3 = window(t2 + s3)
            check_ok(res[8], m3, t2, s3, len(m1["recs"]) + len(m2["recs"]), (what, "third"))
            got += [rec[:3] for rec in m2["recs"]] + [rec[:3] for rec in m3["recs"]]
            assert res[9] == end == b""
        else:
            m3 = window(rest + s3)
            check_ok(res[6], m3, rest, s3, len(m1["recs"]), (what, "third"))  # (records_seen: the refused stretch went round the device)
            got += host_recs + [rec[:3] for rec in m3["recs"]]
            assert res[7] == end == b""
        assert got == want_all, what
    return ops, check


def test_every_refusal_and_the_way_on():
    recs = TEXTS["mixed"]
    b0 = rec_bounds(recs)
    batches = []
    for kind, status in (("blank", IRREGULAR), ("cr", IRREGULAR), ("plus", IRREGULAR), ("unequal", IRREGULAR), ("strand", STRAND)):
        for r in (10, 20, 29):  # the first, a middle and the last record in front of the second submission's cut
            text = join(plant(recs, r, kind))
            # (the cuts lie inside records 10 and 30, three bytes behind their starts: '@re|ad ...'; a plant moves the second)
            c1, c2 = int(b0[10]) + 3, int(b0[30]) + 3 + len(text) - int(b0[-1])
            batches.append(refusal_script(text, c1, c2, CAP, status, (kind, r)))
    text = join(recs)
    c1, c2 = int(b0[10]) + 3, int(b0[30]) + 3
    for k in range(3):
        batches.append(refusal_script(text, c1, c2, CAP, BLOCK, ("block", k), block_status=[3 if i == k else 0 for i in range(3)]))
    tiny = [([b"@a", b"A", b"+", b"I"], [b"\n"] * 4)] * 2000  # 9 bytes a record: more than one per 64 bytes and 16
    many = recs[:11] + tiny + recs[30:]
    bm = rec_bounds(many)
    batches.append(refusal_script(join(many), int(bm[10]) + 3, int(bm[11 + 2000]) + 3, 4096, TOO_MANY, "too many"))
    long_at = next(i for i in range(11, 40) if len(recs[i][0][1]) == 9000)
    short = [r for r in recs if len(r[0][1]) < 1000]  # (a 4096-byte tail holds any of them)
    room = short[:12] + [recs[long_at]] + short[12:]
    br = rec_bounds(room)
    batches.append(refusal_script(join(room), int(br[5]) + 3, int(br[12]) + 5000, 4096, TAIL_ROOM, "tail room", reserve=CAP))
    run_batches(batches)


# ---- case 6 ----
def whole_model(text):
    """fpl_process_text_async's verdict for a whole chunk: the window's, and nothing may be left behind the cut"""
    m = window(text)
    lone = [i for i in range(len(text) - 1) if text[i] == 13 and text[i + 1] != 10] + ([len(text) - 1] if text.endswith(b"\r") else [])
    irregular = m["status"] == IRREGULAR or bool(lone) or m["n_lines"] % 4 != 0 or not text.endswith(b"\n")
    bad = next((r for r, rec in enumerate(m["recs"]) if not (rec[0][:1] == b"@" and len(rec[1]) == len(rec[2]) and _plus(text, rec))), None)
    return m, irregular, bad


def _plus(text, rec):
    return text[rec[3][2]:rec[3][2] + 1] == b"+"


def test_the_six_kernels_of_text_parse():
    """whole chunks through k_text_count .. k_text_gather: the three texts, a text with name-repeating third lines (regular
    there), and the eight irregular forms tests/test_gpu_text.py lists"""
    batches = []
    for eol, recs in TEXTS.items():
        text = join(recs)

        def check(res, text=text, eol=eol):
            m, irregular, _ = whole_model(text)
            r = res[0]
            assert not irregular and r["status"] == 0 and r["n_records"] == len(m["recs"]) and r["n_lines"] == m["n_lines"], (eol, r["status"])
            assert r["line"].tolist() == [rec[3] for rec in m["recs"]] and r["len"].tolist() == [len(rec[1]) for rec in m["recs"]]
            assert r["seq"] == b"".join(rec[1] for rec in m["recs"]) and r["qual"] == b"".join(rec[2] for rec in m["recs"])
            assert r["n_bases"] == len(r["seq"]) and r["max_len"] == 9000 and r["bad_record"] == NONE
            assert r["off"].tolist() == np.cumsum([0] + [len(rec[1]) for rec in m["recs"]]).tolist()
        batches.append(([emu.whole(text)], check))
    recs = TEXTS["lf"]
    good = join(recs)
    strand = join(plant(recs, 8, "strand"))
    batches.append(([emu.whole(strand)], lambda res: res[0]["status"] == 0 and res[0]["n_records"] == 40 or pytest.fail("strand")))
    cases = {
        "no final line break": good[:-1],
        "blank line between records": join(plant(recs, 10, "blank")),
        "lone carriage return": good.replace(b"\n", b"\r", 1),
        "carriage return inside a line": good[:40] + b"\r" + good[40:],
        "third line does not start with +": join(plant(recs, 7, "plus")),
        "fewer qualities than bases": join([(l[:3] + [l[3][:-1]], e) if i == 20 else (l, e) for i, (l, e) in enumerate(recs)]),
        "header without @": join([([b"read0 without the at sign"] + l[1:], e) if i == 0 else (l, e) for i, (l, e) in enumerate(recs)]),
        "a record of three lines": join([(l[:1] + l[2:], e[:3]) if i == 30 else (l, e) for i, (l, e) in enumerate(recs)]),
    }
    for name, text in cases.items():
        def check(res, name=name, text=text):
            _, irregular, bad = whole_model(text)
            assert irregular and (res[0]["status"] & 1) and not (res[0]["status"] & 2), name
            assert res[0]["bad_record"] == (NONE if bad is None else bad), (name, res[0]["bad_record"], bad)
        batches.append(([emu.whole(text)], check))
    many = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(2000))
    batches.append(([emu.whole(many)], lambda res: res[0]["status"] == 2 or pytest.fail("too many: %r" % res[0]["status"])))
    run_batches(batches)
