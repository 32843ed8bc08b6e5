"""Sequence assessment, the parts that need no GPU: the count histogram's valley (mhap_kmer_histogram_valley), the QV arithmetic
(mhap_kmer_qv) against the restatement's expression, the restatement itself (tests/kmer_qv_ref.py) on an example worked by hand, and
the refusals of both tools' options."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_qv_ref as R
import mhap_amd
from mhap_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMERS_CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip-kmers")


def _valley(hist):
    counts = sorted(hist)
    return api.kmer_histogram_valley(np.array(counts, dtype=np.uint32), np.array([hist[c] for c in counts], dtype=np.uint64))


@pytest.mark.parametrize("hist,want", [
    ({1: 900, 2: 300, 3: 40, 4: 7, 5: 1}, 6),                           # monotone decreasing: the largest count + 1
    ({1: 5000, 2: 700, 3: 90, 4: 30, 5: 45, 6: 200, 7: 650, 8: 400}, 4),  # errors, then the coverage peak: the bottom between them
    ({1: 10, 3: 5, 4: 9}, 2),                                             # a gap: n[2] = 0 and n[3] >= 0
    ({1: 10, 2: 10, 3: 1}, 1),                                            # a tie is a valley (n[c + 1] >= n[c])
    ({1: 7}, 2),                                                          # a single entry at 1
    ({5: 3}, 1),                                                          # a single entry elsewhere: n[1] = 0
    ({}, 1),                                                              # empty
    ({1: 3, 2: 2, 3: 1, 2 ** 32 - 1: 1}, 4),
])
def test_valley(hist, want):
    assert R.valley(hist) == want
    assert _valley(hist) == want


def test_valley_refuses_unordered_counts():
    for counts in ([2, 1], [1, 1], [0, 1]):
        with pytest.raises(mhap_amd.MhapError):
            api.kmer_histogram_valley(np.array(counts, dtype=np.uint32), np.ones(len(counts), dtype=np.uint64))


@pytest.mark.parametrize("k", [1, 2, 9, 16])
def test_qv_matches_the_expression(k):
    cases = [(1, 1), (23, 5), (1000, 1), (10 ** 6, 192), (5 * 10 ** 9, 12345), (2 ** 40, 2 ** 39), (77, 76), (77, 77), (10 ** 12, 1)]
    for windows, missing in cases:
        e, q = api.kmer_qv(windows, missing, k)
        we, wq = R.qv(windows, missing, k)
        # relative 1e-9: far above any difference of one ulp between two libm, far below what a QV of two decimals shows
        assert e == pytest.approx(we, rel=1e-9, abs=0.0), (windows, missing, k)
        assert q == pytest.approx(wq, rel=1e-9, abs=1e-12), (windows, missing, k)
    e, q = api.kmer_qv(0, 0, k)
    assert math.isnan(e) and math.isnan(q)
    assert api.kmer_qv(500, 0, k) == (0.0, math.inf)
    e, q = api.kmer_qv(500, 500, k)                  # every window missing: error 1, QV 0 (and not -0)
    assert (e, q) == (1.0, 0.0) and math.copysign(1.0, q) == 1.0
    for bad in ((-1, 0), (5, -1), (5, 6)):
        with pytest.raises(mhap_amd.MhapError):
            api.kmer_qv(bad[0], bad[1], k)
    with pytest.raises(mhap_amd.MhapError):
        api.kmer_qv(5, 1, 0)


def test_restatement_on_an_example_worked_by_hand():
    """k = 4, not canonical.  The set is the 27 windows of
        truth  ACGTTGCATGGCCAATCGATTACGGATCCA     (30 bases, all 27 windows distinct)
        seq    ACGTTGCAAGGCCAATCNATTACGGATCCG     (T -> A at 8, G -> N at 17, A -> G at 29)
    Windows of seq (27 starts, 0..26):
      * the N at 17 lies in windows 14..17 (ATCN TCNA CNAT NATT): invalid.  windows = 27 - 4 = 23.
      * the substitution at 8 lies in windows 5..8 (GCAA CAAG AAGG AGGC), none of them in the set: missing, one run (5..8); window 4
        (TGCA) and window 9 (GGCC) are present and end it.
      * the substitution at 29 lies in window 26 alone (TCCG), the last one: missing, a run that ends with the sequence.
      missing = 4 + 1 = 5, runs = 2.
    Unsupported positions:
      * 8 is contained in windows 5..8 only, all missing: unsupported.  7 is also in window 4 and 9 also in window 9, both present.
      * 29 is contained in window 26 only: unsupported.  28 is also in window 25 (ATCC, present).
      * 14, 15 and 16 are also in window 13 (AATC, present).  17 is in windows 14..17 only, all invalid, so "some valid window
        contains it" fails: an N alone is not an unsupported base.
      unsupported = 2, intervals [8, 9) and [29, 30).
    error = 1 - (1 - 5/23)^(1/4) = 0.0594407..., qv = -10 log10 of it = 12.26."""
    truth = "ACGTTGCATGGCCAATCGATTACGGATCCA"
    seq = "ACGTTGCAAGGCCAATCNATTACGGATCCG"
    cnt = R.count([truth], 4, False)
    assert len(cnt) == 27 and set(cnt.values()) == {1}
    kset, used = R.solid(cnt, 1)
    assert used == 1 and len(kset) == 27
    row, ivs = R.evaluate(seq, kset, 4, False)
    assert row == [30, 23, 5, 2, 2]
    assert ivs == [(8, 9), (29, 30)]
    assert R.table([row], 4) == "seq1\t30\t23\t5\t2\t2\t5.944073e-02\t12.26\ntotal\t30\t23\t5\t2\t2\t5.944073e-02\t12.26\n"
    assert R.bed([(0, b, e) for b, e in ivs], 1, ["contig"]) == "contig\t8\t9\ncontig\t29\t30\n"
    # the same sequence against itself, against nothing, and short ones
    assert R.evaluate(truth, kset, 4, False) == ([30, 27, 0, 0, 0], [])
    assert R.evaluate(truth, set(), 4, False) == ([30, 27, 27, 1, 30], [(0, 30)])
    assert R.evaluate("ACG", kset, 4, False) == ([3, 0, 0, 0, 0], []) and R.evaluate("", kset, 4, False) == ([0, 0, 0, 0, 0], [])
    assert R.evaluate("NNNNNNNN", kset, 4, False) == ([8, 0, 0, 0, 0], [])
    # canonical: a window is named by the smaller of itself and its reverse complement (ACGT is its own)
    assert R.window_key("ACGT", 0, 4, True) == "ACGT" and R.window_key("TTGC", 0, 4, True) == "GCAA" and R.key_value("GCAA") == 0b10010000
    assert R.qv(0, 0, 4)[0] != R.qv(0, 0, 4)[0] and R.qv(9, 0, 4) == (0.0, math.inf)
    assert R.compare({"A", "C"}, {"C", "G", "T"}) == (2, 3, 1)
    assert R.solid({"A": 50, "C": 1, "G": 1, "T": 2}, 0) == ({"A"}, 3)   # histogram {1: 2, 2: 1, 50: 1}: n[2] < n[1], n[3] < n[2], n[4] >= n[3]


def _kmers(*args):
    return subprocess.run([KMERS_CLI, *args], capture_output=True, text=True, timeout=60)


def test_the_counter_tool_refuses_bad_assess_options_on_the_host():
    mhap_amd.load_library()
    r = _kmers("x.fasta")                                           # unchanged: without --assess, -o is required
    assert r.returncode == 1 and "no output file (-o)" in r.stderr
    r = _kmers("-o", "/dev/null", "-k", "17", "x.fasta")
    assert r.returncode == 1 and "from 1 to 16" in r.stderr
    for opts in (["--assess-min-count", "3"], ["--assess-table", "t.tsv"], ["--assess-bed", "b.bed"]):
        r = _kmers("-o", "/dev/null", *opts, "x.fasta")
        assert r.returncode == 1 and "go with --assess" in r.stderr, opts
    for bad in ("abc", "-1", "2.5", ""):
        r = _kmers("--assess", "a.fasta", "--assess-min-count", bad, "x.fasta")
        assert r.returncode == 1 and "--assess-min-count takes an integer" in r.stderr, bad
    r = _kmers("--assess", "a.fasta", "--assess-table")
    assert r.returncode == 1 and "requires a value" in r.stderr
    r = _kmers("--assess", "a.fasta", "-k", "0", "x.fasta")
    assert r.returncode == 1 and "from 1 to 16" in r.stderr
    r = _kmers("--assess", "a.fasta")
    assert r.returncode == 1 and "no input file" in r.stderr
    r = _kmers("--assess", "a.fasta", "--histogram", "h.txt", "x.fasta")
    assert r.returncode == 1 and "--histogram goes with -o" in r.stderr
    for r in (_kmers("--assess"), _kmers("--assess", "a.fasta", "--assess-nothing", "x.fasta")):
        assert r.returncode == 1 and "Usage: mhap-hip-kmers" in r.stderr


def _tool(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "mhap_amd.kmer_qv", *args], capture_output=True, text=True, env=env, timeout=120)


def test_the_python_tool_refuses_bad_options_before_it_opens_a_device():
    for args, msg in ((["reads.fasta"], "two input files"), (["a.fasta", "b.fasta", "c.fasta"], "two input files"),
                      (["a.fasta", "b.fasta", "-k", "17"], "from 1 to 16"), (["a.fasta", "b.fasta", "-k", "0"], "from 1 to 16"),
                      (["a.fasta", "b.fasta", "-k", "x"], "-k takes an integer"), (["a.fasta", "b.fasta", "--min-count", "-2"], "not negative"),
                      (["a.fasta", "b.fasta", "--min-count"], "requires a value"), (["a.fasta", "b.fasta", "--bogus"], "unknown option --bogus")):
        r = _tool(*args)
        assert r.returncode == 1 and msg in r.stderr and "Usage: python -m mhap_amd.kmer_qv" in r.stderr, (args, r.stderr)
        assert r.stdout == ""
    r = _tool("--help")
    assert r.returncode == 0 and "--min-count" in r.stdout


def test_public_names():
    assert mhap_amd.KmerSet is api.KmerSet and mhap_amd.KmerEval is api.KmerEval
    from mhap_amd import kmer_qv
    assert mhap_amd.assess is kmer_qv.assess
    for name in ("kmer_count_finish_set", "kmer_set_eval", "kmer_set_compare", "kmer_set_contains"):
        assert callable(getattr(mhap_amd.MinHashSearch, name))
    lib = mhap_amd.load_library()
    out = C.c_uint64()
    assert lib.mhap_kmer_histogram_valley(None, None, C.c_int64(0), C.byref(out)) == 0 and out.value == 1


# ---- the evaluation kernel's lane arithmetic, run on the host (mhap_selftest_kmer_eval) ---------------------------------------------
TILE, LANE = 4032, 64   # kmer_kernels.hip KE_TILE (63 lanes of KE_LANE positions; the 64th walks the next tile's first 64 for the 63rd)


def _bitmap(kset, k):
    bits = np.zeros(max(4 ** k // 32, 4), dtype=np.uint32)
    for key in kset:
        v = R.key_value(key)
        bits[v >> 5] |= np.uint32(1 << (v & 31))
    return bits


def _host_eval(seq, bits, k, canonical):
    lib = mhap_amd.load_library()
    b = seq.encode("latin-1")
    ntiles = (len(b) + TILE - 1) // TILE
    row, um = np.zeros(4, dtype=np.int64), np.zeros(max(ntiles * 63, 1), dtype=np.uint64)
    assert lib.mhap_selftest_kmer_eval(b, C.c_int32(len(b)), C.c_int32(k), C.c_int32(1 if canonical else 0), api._ptr(bits), api._ptr(row), api._ptr(um)) == 0
    pos = [w * 64 + j for w in range(ntiles * 63 if len(b) >= k else 0) for j in range(64) if (int(um[w]) >> j) & 1]
    ivs = []
    for p in pos:
        if ivs and ivs[-1][1] == p:
            ivs[-1][1] = p + 1
        else:
            ivs.append([p, p + 1])
    return [len(b)] + row.tolist(), [tuple(i) for i in ivs]


def _edited(genome, rnd, n, edits):
    """genome[:n] with the edits {position: byte}"""
    s = list(genome[:n])
    for p, c in edits.items():
        if 0 <= p < n:
            s[p] = c if c != "x" else "ACGT"[("ACGT".index(s[p]) + 1 + rnd.randrange(3)) % 4]
    return "".join(s)


@pytest.mark.parametrize("k", [1, 2, 9, 12, 16])
def test_lane_arithmetic_on_the_host_matches_the_restatement(k):
    import random
    rnd = random.Random(1000 + k)
    genome = "".join(rnd.choice("ACGT") for _ in range(2 * TILE + 200))
    for canonical in (True, False):
        cnt = R.count([genome], k, canonical)
        if k <= 2:   # every k-mer occurs: keep a set that lacks some
            kset = set(sorted(cnt)[::2])
        else:
            kset = set(cnt)
        bits = _bitmap(kset, k)
        cases = [genome[:n] for n in (0, k - 1, k, k + 1, LANE - 1, LANE, LANE + 1, LANE + k - 2, LANE + k - 1, LANE + k, TILE - 1, TILE, TILE + 1,
                                      TILE + k - 2, TILE + k - 1, TILE + k)]
        n = 2 * TILE + k
        for at in (0, n - 1, LANE - 1, LANE, LANE + k - 1, TILE - k, TILE - 1, TILE, TILE + k - 1, 2 * TILE - 1, 2 * TILE):
            cases.append(_edited(genome, rnd, n, {at: "x"}))                         # runs that begin, end or straddle the lane and tile edges
            cases.append(_edited(genome, rnd, n, {at: "x", at + k - 1: "x"}))        # two substitutions fewer than k apart: one run
            cases.append(_edited(genome, rnd, n, {at: "N"}))
            cases.append(_edited(genome, rnd, n, {at + j: "N" for j in range(k + 3)}))
            cases.append(_edited(genome, rnd, n, {at: "R", at + 2 * k: "a", at + 4 * k: "x"}))   # raw bytes: IUPAC, lower case
        for seq in cases:
            want = R.evaluate(seq, kset, k, canonical)
            assert _host_eval(seq, bits, k, canonical) == want, (k, canonical, len(seq))
        empty = np.zeros_like(bits)
        seq = cases[-1]
        assert _host_eval(seq, empty, k, canonical) == R.evaluate(seq, set(), k, canonical)
