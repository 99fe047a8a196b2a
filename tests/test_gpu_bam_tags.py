"""-m gpu: the auxiliary fields of a BAM input's records in the BAM records the device composes (fpl_set_bam_tags; csrc/bam_tags.h:
k_bam_tags, k_bamout_layout_bam_tags, k_bamout_compose_bam_tags) through Engine.submit_bam, Engine.submit_bgzf and the CLI on the
real library.

The per-read records are the device's own; what the output must hold for them is the plain-Python rule's answer
(tests/bam_tag_cases.py) and the host form's (tests/test_host_bam_tags.py), byte for byte.  Every BGZF block inflates on its own,
by gzip and by the device's Inflater with status 0; bam_tag_stats() is the model's; with the switch off the bytes are those of a
library that never heard of tags."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import abi, bgzf, build, synth
from tests import bam_out_cases as bc
from tests import bam_tag_cases as tc
from tests import bamio, hostio
from tests.gzcheck import host_format
from tests.test_bam_tags_emu import deflate_blocks, stream
from tests.test_gpu_bam_out import C3, PLAIN, check_device_bytes, engine_mod, hostlib, inflater, new_engine, pinned  # noqa: F401
from tests.test_host_bam_tags import L, host_form  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recs():
    """the case list's records (regions that do not parse included) and reads with adapters, so that the device's own records
    hold whole, trimmed, split and failing reads; every third of the latter stored reversed"""
    out, _ = tc.case_list(malformed=True)
    seq, qual, off = synth.ont_like(160, seed=8, median_len=700, p_middle=0.3)
    keys = [k for k in sorted(tc.REGIONS) if len(tc.REGIONS[k]) < 2000]
    for i, (name, _, codes, q) in enumerate(bamio.fastq_to_records(hostio.make_fastq(seq, qual, off)[0])):
        name = b"ont%d" % i
        n, f, c, q = bamio.reverse_record(name, codes, q) if i % 3 == 1 else (name, 0, codes, q)
        out.append((n, f, c, q, bamio.encode_record(n, f, c, q, tags=tc.REGIONS[keys[(7 * i) % len(keys)]])))
    return out


def check_tagged(inflater, data, want, label):  # noqa: F811
    blocks = bc.check_device_blocks(data, want)  # stripes of 49 152 bytes, each a gzip member of its own
    desc, _ = bgzf.blocks(data)
    out, status = inflater.inflate(np.frombuffer(data, np.uint8), desc)
    assert len(status) == len(blocks) and (status == 0).all(), status
    assert out.tobytes() == want
    nb = deflate_blocks(want)
    print("%s: records %d, BGZF %d in %d blocks of %d deflate blocks" % (label, len(want), len(data), len(blocks), nb))
    assert len(data) <= len(want) + 5 * nb + 31 * len(blocks)


@pytest.mark.parametrize("opts", ["plain", "c3"])
def test_submit_bam_equals_host_form_and_model(engine_mod, L, inflater, tmp_path, recs, opts):  # noqa: F811
    raw, starts, off = stream(recs)
    eng = new_engine(engine_mod, PLAIN if opts == "plain" else C3, True, C=65536)
    eng.set_bam_tags(True)
    assert eng.bam_tag_stats() == (0, 0, 0, 0)
    res = np.zeros(len(starts), abi.RESULT_DTYPE)
    eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
    data = eng.wait()
    stats = eng.bam_tag_stats()
    eng.close()
    want = tc.expected(recs, res)
    if opts == "plain":  # every read passes whole: records of forward reads keep their positional fields, 100 000 bytes of mv included
        assert want[2][0] > 300 and tc.REGIONS["mv_100000"] in want[0]
    else:
        assert (res["n_frag"] == 2).any() and (res["code"][:, 0] != 0).any() and want[2][1] > 50
    assert want[2][3] > 5
    check_tagged(inflater, data, want[0], "submit_bam " + opts)
    assert list(stats) == want[2]
    host = host_form(L, tmp_path, recs, res, 3)
    assert host[0] == want[0] and host[2] == want[2]


def test_submit_bgzf_equals_the_model(engine_mod, inflater, recs):  # noqa: F811
    file = tc.input_bam(recs, header_text=tc.RG_HEADER)
    eng = new_engine(engine_mod, C3, True, C=65536)
    eng.set_bam_tags(True)
    desc, _ = bgzf.blocks(file)
    h, res, names, seq, qual, data = eng.submit_bgzf(pinned(eng, file), desc, skip=bgzf.header_len(file), gzip=True).wait()
    stats = eng.bam_tag_stats()
    eng.close()
    assert h["status"] == abi.FPL_BAMW_OK and h["n_reads"] == len([r for r in recs if not r[1] & 0x900])
    want = tc.expected(recs, res)
    check_tagged(inflater, data, want[0], "submit_bgzf")
    assert list(stats) == want[2]
    # a library caller's file: the header with the input's read groups, the batch, the EOF block
    out = bgzf.bam_header(read_groups=bgzf.read_group_lines(tc.RG_HEADER)) + data + bgzf.eof()
    assert gzip.decompress(out) == tc.header_raw(tc.RG_HEADER) + want[0]


def test_switch_off_gives_todays_bytes_and_text_batches_ignore_it(engine_mod, hostlib, inflater, tmp_path, recs):  # noqa: F811
    small = [r for r in recs if len(r[4]) < 20000]
    raw, starts, off = stream(small)
    twin = b"".join(bamio.twin_record(*r[:4]) for r in small if not r[1] & 0x900)
    outs = []
    for switch in (None, False, True):
        eng = new_engine(engine_mod, C3, True, C=65536)
        if switch is not None:
            eng.set_bam_tags(True)  # (on, then off again before the submission: the next submission decides)
            eng.set_bam_tags(switch)
        res = np.zeros(len(starts), abi.RESULT_DTYPE)
        eng.submit_bam(pinned(eng, raw), starts, off, res=res, gzip=True)
        outs.append((eng.wait(), res.copy(), eng.bam_tag_stats()))
        eng.close()
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2] == (0, 0, 0, 0) and outs[2][0] != outs[0][0]
    assert outs[0][1].tobytes() == outs[2][1].tobytes()
    check_device_bytes(hostlib, inflater, outs[0][0], host_format(hostlib, tmp_path, twin, outs[0][1]), "switch off")
    # a text batch: its gzip bytes are BAM records of FASTQ text, which has no tags to keep
    text = twin[:40000].rsplit(b"\n@", 1)[0] + b"\n"
    both = []
    for switch in (False, True):
        eng = new_engine(engine_mod, PLAIN, True)
        eng.set_bam_tags(switch)
        eng.submit_text(pinned(eng, text), gzip=True)
        both.append(eng.wait_text()[3])
        assert eng.bam_tag_stats() == (0, 0, 0, 0)
        eng.close()
    assert both[0] == both[1] and len(both[0]) > 1000


def test_cli_device_form_equals_host_form(engine_mod, tmp_path, recs):  # noqa: F811
    build.build_all()
    small = [r for r in recs if len(r[4]) < 20000 and not r[0].startswith(b"bad.")]  # (the CLI's reader refuses fields that do not parse)
    (tmp_path / "tagged.bam").write_bytes(tc.input_bam(small, header_text=tc.RG_HEADER))
    flags = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]
    got = {}
    for name, extra in (("dev", ["--device_gzip"]), ("host", [])):
        d = tmp_path / name
        d.mkdir()
        p = subprocess.run([build.CLI, "-i", str(tmp_path / "tagged.bam"), "-o", str(d / "out.bam"), "--keep_tags", "-V", "-j", str(d / "o.json"),
                            "-h", str(d / "o.html")] + flags + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, FPLH_CHUNK_BYTES="60000"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        n_dev = int(p.stderr.split(b"BAM records: BGZF blocks framed on the device: ")[1].split()[0])
        line = [l for l in p.stderr.split(b"\n") if l.startswith(b"BAM tags: ")]
        assert len(line) == 1 and (n_dev > 0) == bool(extra)
        got[name] = (gzip.decompress((d / "out.bam").read_bytes()), line[0])
    assert got["dev"] == got["host"]
    raw = got["dev"][0]
    assert raw.startswith(tc.header_raw(tc.RG_HEADER)) and raw.count(tc.K2) > 20
    kept, lost, nbytes = (int(x) for x in __import__("re").findall(rb"\d+", got["dev"][1].replace(b"MM, ML, MN, B", b""))[:3])
    assert kept > 0 and lost > 0 and nbytes > 1000
