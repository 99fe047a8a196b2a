"""-m gpu: --reindex_comments through the CLI on the real library.  There is no device form of the flag: what is pinned here is
that a run whose chunks ARE parsed and trimmed on the device (text-backed batches: the name lines and bases the host rewrites from
lie in the chunk's raw text) writes what the plain-Python model (tests/fq_comment_cases.py) makes of the same run's text without the
flag; that --device_gzip changes nothing under the flag -- the device deflates no member of such a run --; and that without the flag
the same input still takes the device's gzip form."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from fastplong_amd import build, synth
from tests import fq_comment_cases as fc
from tests.test_cli_fq_comments_stub import V_LINE, model, v_line
from tests.test_gpu_bam_out import engine_mod  # noqa: F401

pytestmark = pytest.mark.gpu

FLAGS = ["-s", synth.START_ADAPTER, "-e", synth.END_ADAPTER, "--cut_front", "--cut_tail", "-W", "5", "-x", "-y"]


def make_reads():
    """about 160 ONT-like reads of median 700 with adapters, so that the device's own results hold split and front-trimmed reads;
    every one carries generated calls as comments (C+mh? at CpGs, A+a. at every fourth A, a sparse N+n group), every fourth a move
    table beside them, every eleventh an ML one value short"""
    rng = np.random.default_rng(12)
    seq, qual, off = synth.ont_like(160, seed=8, median_len=700, p_middle=0.3)
    out = []
    for i in range(len(off) - 1):
        s, q = seq[int(off[i]):int(off[i + 1])].tobytes(), qual[int(off[i]):int(off[i + 1])].tobytes()
        occ = fc.occurrences(s, b"C")
        cpg = [k for k, p in enumerate(occ) if s[p + 1:p + 2] == b"G"]
        spec = [(b"C+mh?", [m - (cpg[j - 1] + 1 if j else 0) for j, m in enumerate(cpg)]), (b"A+a.", fc.every(s, b"A", 4, 3)), (b"N+n", fc.every(s, b"N", 97, 11))]
        fields = fc.mods(s, spec, rng)
        if i % 11 == 7:
            fields[1] = fields[1][:fields[1].rindex(b",")]
        fields = fc.KEPT[:1] + fields[:1] + ([b"mv:B:c,5,1,0,1,1,0"] if i % 4 == 1 else fc.KEPT[1:2]) + fields[1:] + fc.KEPT[2:]
        out.append((b"@ont%d" % i + b"".join(b"\t" + f for f in fields), s, q))
    return out


@pytest.fixture(scope="module")
def reads():
    return make_reads()


def run(tmp_path, name, inp, extra):
    d = tmp_path / name
    d.mkdir()
    p = subprocess.run([build.CLI, "-i", str(inp), "-o", str(d / "out.fastq.gz"), "-V", "-j", str(d / "o.json"), "-h", str(d / "o.html")] + FLAGS + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, FPLH_CHUNK_BYTES="60000"))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    n_dev = int(p.stderr.split(b"device gzip: ")[1].split()[0]) if b"device gzip: " in p.stderr else 0
    n_parsed = int(p.stderr.split(b"device parse: ")[1].split()[0]) if b"device parse: " in p.stderr else 0
    return gzip.decompress((d / "out.fastq.gz").read_bytes()), p, n_dev, n_parsed


def test_cli_on_the_real_library_equals_the_model_with_and_without_device_gzip(engine_mod, tmp_path, reads):  # noqa: F811
    build.build_all()
    inp = tmp_path / "in.fq"
    inp.write_bytes(fc.fastq(reads))
    by_name = {l.split(b"\t")[0][1:]: (l, s, q) for l, s, q in reads}
    base, _, n_dev, n_parsed = run(tmp_path, "base", inp, [])
    assert n_dev >= 3 and n_parsed >= 3  # (without the flag: chunks parsed on the device, members deflated there)
    want, st, seen = model(base, by_name)
    assert st[0] > 100 and st[1] > 5 and st[2] > 10000 and st[3] > 500 and st[4] == 0
    assert sum(1 for s, ch, kept in seen if s > 0 and kept > 0) > 50 and want.count(b"@split-by-adapter-right-") > 10
    for name, extra in (("host", []), ("dev", ["--device_gzip"])):
        got, p, n_dev, n_parsed = run(tmp_path, name, inp, ["--reindex_comments"] + extra)
        assert got == want, name
        assert n_dev == 0 and n_parsed >= 3  # (parsed and trimmed on the device, formatted and deflated by the host)
        assert v_line(p) == [(V_LINE % tuple(st)).encode()]

