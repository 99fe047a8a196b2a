"""Seeded generators of adapter cases shared by tests/test_second_reading.py and tests/test_adaptertrimmer_vs_ref.py: adapters
of the shapes where a window search goes wrong (empty, short, homopolymer, short-period, N-bearing, long) and reads holding
noisy / truncated / exact copies of them."""
import numpy as np

from fastplong_amd import synth


def rnd(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), int(n))])


def mutated(rng, ad, err):
    return bytes(synth._mutate(rng, np.frombuffer(ad, np.uint8), err)) if len(ad) else b""


def adapter(rng):
    k = int(rng.integers(0, 10))
    if k == 0:
        return b""
    if k == 1:
        return rnd(rng, rng.integers(1, 8))
    if k == 2:
        return rnd(rng, 1) * int(rng.integers(4, 40))  # homopolymer: every window ties
    if k == 3:
        return rnd(rng, rng.integers(2, 5)) * int(rng.integers(3, 12))  # short period: ties between shifted windows
    if k == 4:
        return rnd(rng, rng.integers(16, 70), b"ACGTN")
    if k == 5:
        return rnd(rng, rng.integers(60, 260))
    return rnd(rng, rng.choice([15, 16, 17, 24, 24, 31, 32, 33, 45, 64]))


def read_with(rng, ad, rlen_max=700):
    """a read that holds 0..3 noisy / truncated / exact copies of `ad` (so that several windows tie), N runs, lower case"""
    L = int(rng.choice([0, 1, 5, 15, 16, 17, 31, 40, 199, 200, 201, 216, 217])) if rng.random() < 0.3 else int(rng.integers(0, rlen_max))
    if rng.random() < 0.15 and len(ad):
        L = int(rng.integers(0, len(ad) + 2))  # around alen: alen > rlen, alen == rlen, alen == rlen - 1
    body = bytearray(rnd(rng, L))
    if rng.random() < 0.15 and len(ad):
        unit = ad[:max(1, len(ad) // 2)]
        body = bytearray((unit * (L // len(unit) + 1))[:L])  # the adapter's own period all over the read
    for _ in range(int(rng.integers(0, 4))):
        if not len(ad) or not L:
            break
        c = mutated(rng, ad, float(rng.choice([0.0, 0.0, 0.05, 0.1, 0.2, 0.35])))
        if rng.random() < 0.35 and len(c) > 2:
            cut = int(rng.integers(1, len(c)))
            c = c[cut:] if rng.random() < 0.5 else c[:cut]
        where = rng.random()
        at = int(rng.integers(0, 30)) if where < 0.35 else (max(0, L - len(c) - int(rng.integers(0, 30))) if where < 0.7 else int(rng.integers(0, L)))
        body[at:at + len(c)] = c
        body = body[:L] if rng.random() < 0.8 else body
    if rng.random() < 0.1 and len(body):
        a = int(rng.integers(0, len(body)))
        body[a:a + int(rng.integers(1, 20))] = b"N" * min(len(body) - a, int(rng.integers(1, 20)))
    if rng.random() < 0.05 and len(body):
        a = int(rng.integers(0, len(body)))
        body[a:a + 10] = bytes(body[a:a + 10]).lower()
    return bytes(body)
