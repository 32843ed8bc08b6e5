"""The GPU aligner (mhap_align_pairs, align_kernels.hip) against its CPU restatement (tests/align_ref.py), field by field."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import align_ref  # noqa: E402

pytestmark = pytest.mark.gpu

R = 8             # rows per lane (AL_R)
ONE_WAVE = 64 * R # s1 rows of the one-wave kernel
PASS = 256 * R    # s1 rows of one pass of the four-wave kernel


def _mutate(rng, s, div):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < div / 3:
            continue
        if u < 2 * div / 3:
            out.append(c)
            out.append(int(rng.choice(list(b"ACGT"))))
            continue
        out.append(int(rng.choice(list(b"ACGT"))) if u < div else c)
    return bytes(out)


def _batch(segs):
    """(bases, pairs) of (s1, s2, b_rc) triples; s2 is stored as given (the aligner reverse-complements it when b_rc)."""
    bases, pairs, off = bytearray(), [], 0
    for s1, s2, rc in segs:
        bases += s1
        bases += s2
        pairs.append((off, len(s1), off + len(s1), len(s2), rc))
        off += len(s1) + len(s2)
    return np.frombuffer(bytes(bases) or b"\0", np.uint8), np.array(pairs, np.int64).reshape(-1, 5)


def _check(segs):
    bases, pairs = _batch(segs)
    got = mhap_amd.align_pairs(bases, pairs)
    want = align_ref.align_pairs(bases, pairs)
    for q in range(len(pairs)):
        assert got[q].tolist() == want[q].tolist(), (q, pairs[q].tolist(), got[q].tolist(), want[q].tolist())
    return got


def test_random_divergent_pairs():
    rng = np.random.default_rng(1)
    segs = []
    for k in range(14):
        n = int(rng.integers(0, 3001)) if k > 1 else k * 5
        s = bytes(rng.choice(list(b"ACGT"), n).tolist())
        t = _mutate(rng, s[int(rng.integers(0, max(1, n // 4))):], rng.uniform(0, 0.2))
        rc = int(rng.integers(0, 2))
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc))
    got = _check(segs)
    assert (got[2:, 0] > 0).all()


@pytest.mark.parametrize("m", [R - 1, R, R + 1, ONE_WAVE - 1, ONE_WAVE, ONE_WAVE + 1, PASS - 1, PASS, PASS + 1,
                               2 * PASS - 1, 2 * PASS, 2 * PASS + 1, 3 * PASS + 5])
def test_strip_and_pass_boundaries(m):
    rng = np.random.default_rng(m)
    g = bytes(rng.choice(list(b"ACGT"), m + 400).tolist())
    s1 = g[:m]
    s2 = _mutate(rng, g[max(0, m - 250):m + 150], 0.1)     # the alignment ends near the last rows of s1
    s3 = _mutate(rng, g[:300], 0.1)                        # ... and near the first
    _check([(s1, s2, 0), (s1, s3, 0), (s2, s1, 0)])


def test_special_bytes_and_ties():
    segs = [(b"ACGT" * 10, b"TGCA" * 10, 0),              # all mismatch but for accidental matches
            (b"AAAAAAAA", b"CCCCCCCC", 0),                # no positive cell
            (b"NNNNNACGTNNNN", b"NNNNNN", 0),             # N runs match N
            (b"ACGTRYKMBVDHWSN", b"ACGTRYKMBVDHWSN", 1),  # IUPAC bytes under b_rc
            (b"acgt", b"ACGT", 0),                        # bytes are compared as they are
            (b"ACG", b"ACGTTACG", 0),                     # end-cell tie: smallest j
            (b"ACGACG", b"ACG", 0),                       # end-cell tie: smallest i
            (b"ACGTTTTACGT", b"ACGTACGT", 0),             # gap placement: E/F/diagonal priority
            (b"ACGTACGT", b"ACGTTTTACGT", 0),
            (b"AAAAAA", b"AAA", 1),                       # rc of TTT
            (b"", b"ACGT", 0), (b"ACGT", b"", 0)]
    got = _check(segs)
    assert got[1].tolist() == [0, -1, -1, -1, -1, 0, 0] and got[10].tolist() == got[1].tolist()
    assert got[5, 3:5].tolist() == [0, 2]


def test_batch_equals_single_calls_permuted_and_split():
    rng = np.random.default_rng(7)
    segs = []
    for m in (0, 5, 100, 600, 1500, 2100, 4500, 30, 900):
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        segs.append((s, _mutate(rng, s, 0.12), int(rng.integers(0, 2))))
    bases, pairs = _batch(segs)
    whole = mhap_amd.align_pairs(bases, pairs)
    single = np.concatenate([mhap_amd.align_pairs(bases, pairs[q:q + 1]) for q in range(len(pairs))])
    perm = rng.permutation(len(pairs))
    permuted = mhap_amd.align_pairs(bases, pairs[perm])
    split = np.concatenate([mhap_amd.align_pairs(bases, pairs[:4]), mhap_amd.align_pairs(bases, pairs[4:])])
    assert (whole == single).all() and (whole[perm] == permuted).all() and (whole == split).all()
    assert (whole == align_ref.align_pairs(bases, pairs)).all()


def test_scores_past_int16():
    rng = np.random.default_rng(3)
    s = bytes(rng.choice(list(b"ACGT"), 20000).tolist())
    d = s[:10000] + s[10007:]                             # one 7-base deletion: 2 * 19993 - (2 + 6)
    bases, pairs = _batch([(s, s, 0), (d, s, 0)])
    got = mhap_amd.align_pairs(bases, pairs)
    assert got[0].tolist() == [40000, 0, 19999, 0, 19999, 20000, 0]
    assert got[1].tolist() == [39978, 0, 19992, 0, 19999, 20000, 7]


_BIG = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import mhap_amd
rng = np.random.default_rng(4)
s = rng.choice(np.frombuffer(b"ACGT", np.uint8), 100000)
t = s.copy(); t[50000] = ord("A") if s[50000] != ord("A") else ord("C")
bases = np.concatenate([s, t])
got = mhap_amd.align_pairs(bases, np.array([[0, 100000, 0, 100000, 0], [0, 100000, 100000, 100000, 0]]))
assert got[0].tolist() == [200000, 0, 99999, 0, 99999, 100000, 0], got[0]
assert got[1].tolist() == [199996, 0, 99999, 0, 99999, 100000, 1], got[1]
print("ok")
"""


def test_100kb_pair_under_its_own_timeout():
    p = subprocess.run([sys.executable, "-c", _BIG, ROOT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ok" in p.stdout, p.stderr[-2000:]
