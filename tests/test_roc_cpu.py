"""EstimateROC restated (mhap_amd/roc.py), the synthetic reads' truth (mhap_synth_truth, workloads.write_truth_m4) and the CPU
reference of the GPU aligner (tests/align_ref.py).  No GPU: the aligner is injected."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import roc, workloads  # noqa: E402
import align_ref  # noqa: E402


# ---- java.util.Random --------------------------------------------------------------------------------------------------------
def test_java_random_kat():
    assert roc.JavaRandom(0).next_int() == -1155484576
    r = roc.JavaRandom(0)
    assert [r.next_int(100) for _ in range(5)] == [60, 48, 29, 47, 15]


def test_java_random_next_int_branches():
    # power of two: (bound * next(31)) >> 31, one draw
    a, b = roc.JavaRandom(5), roc.JavaRandom(5)
    for _ in range(100):
        assert a.next_int(16) == (16 * b.next(31)) >> 31
        assert a.seed == b.seed
    # rejection: bound 3 * 2^29 rejects every u >= bound (u - r + m overflows int); some draw must take more than one next(31)
    a, b = roc.JavaRandom(1), roc.JavaRandom(1)
    bound, rejected = 3 << 29, 0
    for _ in range(200):
        v = a.next_int(bound)
        assert 0 <= v < bound
        u = b.next(31)
        while u >= bound:
            rejected += 1
            u = b.next(31)
        assert v == u % bound and a.seed == b.seed
    assert rejected > 0


# ---- DecimalFormat("############.########") ---------------------------------------------------------------------------------
@pytest.mark.parametrize("x,want", [(0.0, "0"), (1.0, "1"), (0.5, ".5"), (1 / 3, ".33333333"), (2 / 3, ".66666667"),
                                    (2.0 ** -9, ".00195312"), (3 * 2.0 ** -9, ".00585938"),        # exact ties: to even
                                    (0.123456785, ".12345678"), (0.100000005, ".10000001"),         # binary value just below / above ...5
                                    (float("nan"), "�"), (float("inf"), "∞"), (12.25, "12.25")])
def test_decimal_format(x, want):
    assert roc.decimal_format(x) == want


# ---- parsers -----------------------------------------------------------------------------------------------------------------
LENS = {0: 1000, 1: 2000, 2: 3000}


def _len(k):
    return LENS[k]


def test_overlap_info_four_forms():
    o = roc.get_overlap_info("1 2 N 100 -50 1.5", _len)                                       # CA, 6 columns
    assert (o.id1, o.id2, o.isFwd, o.afirst, o.asecond, o.bfirst, o.bsecond) == ("1", "2", True, 100, 950, 0, 2000)
    o = roc.get_overlap_info("1 2 I -100 50 1.5 0", _len)                                     # CA, 7 columns, aoffset < 0
    assert (o.isFwd, o.afirst, o.asecond, o.bfirst, o.bsecond) == (False, 0, 1000, 100, 1950)
    o = roc.get_overlap_info("2 3 0.1 50 0 10 1990 2000 1 5 3500 3000", _len)                # MHAP, clamped to the lengths
    assert (o.id1, o.id2, o.isFwd, o.afirst, o.asecond, o.bfirst, o.bsecond) == ("2", "3", False, 10, 1990, 5, 3000)
    o = roc.get_overlap_info("m/1/0_5 x,3 -100 90.5 0 10 500 1000 0 20 510 3000 254", _len)  # blasr forward; id at / and ,
    assert (o.id1, o.id2, o.isFwd, o.afirst, o.asecond, o.bfirst, o.bsecond) == ("m", "3", True, 10, 500, 20, 510)
    o = roc.get_overlap_info("1 3 -100 90.5 0 10 500 1000 1 20 510 3000 254", _len)          # blasr reverse: flipped by the length
    assert (o.isFwd, o.bfirst, o.bsecond) == (False, 2490, 2980)
    line = "         1      3 c   [ 4,746.. 8,108] x [     0.. 2,896] :   <    982 diffs  ( 34 trace pts)"
    o = roc.get_overlap_info(line, _len)                                                      # daligner LAshow, complement
    assert (o.id1, o.id2, o.isFwd, o.afirst, o.asecond, o.bfirst, o.bsecond) == ("1", "3", False, 4746, 8108, 104, 3000)
    assert roc.get_overlap_info("a b c", _len).id1 is None
    o = roc.get_overlap_info("1 2 N x -50 1.5", _len)                                         # NumberFormatException: ids kept
    assert (o.id1, o.id2, o.afirst) == ("1", "2", 0)


def test_overlap_size_and_ovl_name():
    o = roc.Overlap()
    o.afirst, o.asecond, o.bfirst, o.bsecond = 0, 101, 10, 10
    assert o.get_size() == 51                                  # Math.round(50.5) = 51
    assert roc.ovl_name("10", "9") == "10_9" and roc.ovl_name("9", "10") == "10_9"
    assert roc.get_range_overlap(0, 10, 10, 20) == 1 and roc.get_range_overlap(0, 5, 10, 20) == -4


def _write(path, lines):
    with open(path, "w") as fh:
        fh.write("".join(line + "\n" for line in lines))
    return str(path)


def test_reference_and_dedup(tmp_path):
    fa = mhap_amd.FastaData.from_strings(["A" * 1000, "C" * 1000, "G" * 1000])
    m4 = _write(tmp_path / "t.m4", [
        "1 chrA -900 95.0 0 0 1000 1000 0 100 1100 50000",
        "2/0_1000 chrA -950 95.0 0 0 1000 1000 1 47000 48000 50000",     # reverse: [2000, 3000)
        "3 chrA -500 70.0 0 0 1000 1000 0 0 1000 50000",                 # idy below 80: skipped
        "1 chrA -990 95.0 0 0 1000 1000 0 200 1200 50000",               # lower score replaces
        "1 chrA -100 95.0 0 0 1000 1000 0 900 1900 50000",               # higher score does not
        "x,3 chrA -100 95.0 0 0 500 1000 0 0 1000 50000"])               # span ratio 0.5 < 0.8: skipped
    g = roc.EstimateROC(min_ovl=10, trials=0)
    g.process_reference(m4)
    assert g.seq_to_name == ["1", "2"]
    assert g.pos.tolist() == [[200, 1200], [2000, 3000]]
    g.load_fasta(fa)
    ovl = _write(tmp_path / "o.txt", [
        "1 2 0.1 50 0 0 500 1000 0 0 500 1000",
        "2 1 0.1 50 0 0 800 1000 0 0 800 1000",      # longer: replaces, keeps the first index
        "1 2 0.1 50 0 0 100 1000 0 0 100 1000",      # shorter: dropped
        "1 1 0.1 50 0 0 100 1000 0 0 100 1000",      # self
        "1 3 0.1 50 0 0 100 1000 0 0 100 1000"])     # 3 is not in the truth
    g.process_overlaps(ovl)
    assert g.ovl_to_name == ["1_2"] and g.ovl_names == {"1_2": 800} and g.ovl_info["1_2"].id1 == "2"
    g2 = roc.EstimateROC(min_ovl=10, trials=0, load_all=True)
    g2.process_reference(m4)
    g2.load_fasta(fa)
    g2.process_overlaps(ovl)
    assert g2.ovl_to_name == ["1_2", "1_3"]


# ---- the interval tree -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_interval_pairs_equal_literal_tree(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 120))
    grid = int(rng.integers(3, 40))            # few distinct endpoints: touching intervals and duplicates
    s = rng.integers(0, grid, n)
    e = s + rng.integers(0, 6, n)
    # (no reversed interval: IntervalNode sends one to the left forever, a StackOverflowError in Java as in the restatement)
    tree = roc.IntervalTree()
    for k in range(n):
        tree.add_interval(int(s[k]), int(e[k]), k)
    lit = set()
    for k in range(n):
        for j in tree.get(int(s[k]), int(e[k])):
            if j != k:
                lit.add((min(j, k), max(j, k)))
    a, b = roc.intersecting_pairs(s, e)
    vec = set(zip(a.tolist(), b.tolist()))
    assert vec == lit
    # a self-hit is what the tree gives for a non-degenerate interval and not for the others
    for k in range(n):
        assert (k in tree.get(int(s[k]), int(e[k]))) == (e[k] > s[k])


# ---- the synthetic truth -----------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _genome_of_reads(n, length, seed, coverage):
    """The genome is not exported: at error rate 0 every read is a genome window, so the reads rebuild it."""
    t, G = mhap_amd.synth_truth(n, length, seed=seed, coverage=coverage, error_rate=0.0)
    fa = mhap_amd.synth_reads(n, length, seed=seed, coverage=coverage, error_rate=0.0)
    return t, G, fa


def test_truth_error_free_reads_are_genome_windows():
    n, L, seed, cov = 400, 300, 11, 8.0
    t, G, fa = _genome_of_reads(n, L, seed, cov)
    assert (t["span"] == L).all() and (t["ins"] == 0).all() and (t["dels"] == 0).all() and (t["subs"] == 0).all()
    genome = bytearray(b"?" * G)
    for q in range(n):
        s = fa.sequence(q).encode()
        fwd = s.translate(_COMP)[::-1] if t["strand"][q] else s
        for k in range(L):
            p = (int(t["start"][q]) + k) % G
            assert genome[p] in (ord("?"), fwd[k]), (q, k)   # every read agrees with every other on the genome
            genome[p] = fwd[k]
    assert 0 < t["strand"].sum() < n


def test_truth_with_errors_and_wraps(tmp_path):
    n, L, seed, cov = 2000, 1000, 3, 5.0
    t, G = mhap_amd.synth_truth(n, L, seed=seed, coverage=cov, error_rate=0.15)
    assert (t["length"] == t["span"] + t["ins"] - t["dels"]).all()
    assert t["ins"].sum() > t["dels"].sum() > 0 and t["subs"].sum() > 0
    wraps = int((t["start"] + t["span"] > G).sum())
    assert wraps > 0
    path = tmp_path / "truth.m4"
    assert workloads.write_truth_m4(path, t, G) == wraps
    g = roc.EstimateROC()
    g.process_reference(str(path))
    keep = np.nonzero(t["start"] + t["span"] <= G)[0]
    assert g.seq_to_name == [str(q + 1) for q in keep]
    assert g.pos.tolist() == [[int(t["start"][q]), int(t["start"][q] + t["span"][q])] for q in keep]
    # shards and the genome form
    ts, Gs = mhap_amd.synth_truth(n, L, seed=seed, coverage=cov, error_rate=0.15, shard=1, nshards=3)
    assert Gs == G and (ts == t[1::3]).all()
    lens = np.array([500, 0, 700, 1200], np.int32)
    tg, _ = mhap_amd.synth_truth(4, seed=seed, lengths=lens, genome_len=5000, error_rate=0.1)
    assert tg["start"][1] == -1 and (tg["length"] == tg["span"] + tg["ins"] - tg["dels"])[[0, 2, 3]].all()


def test_truth_export_leaves_reads_unchanged():
    before = mhap_amd.synth_reads(300, 800, seed=5, coverage=6.0, repeats=(100, 400, 0.02))
    g = np.random.default_rng(1).integers(0, 4, 20000).astype(np.uint8)
    lens = np.full(50, 900, np.int32)
    gb = mhap_amd.synth_reads_from_genome(g, lens, seed=9)
    mhap_amd.synth_truth(300, 800, seed=5, coverage=6.0)
    mhap_amd.synth_truth(50, seed=9, lengths=lens, genome_len=len(g))
    after = mhap_amd.synth_reads(300, 800, seed=5, coverage=6.0, repeats=(100, 400, 0.02))
    assert before.bases.tobytes() == after.bases.tobytes()
    assert gb.bases.tobytes() == mhap_amd.synth_reads_from_genome(g, lens, seed=9).bases.tobytes()
    # the genome form's truth explains its reads: at error rate 0 each read is its genome window
    t0, _ = mhap_amd.synth_truth(50, seed=9, lengths=lens, genome_len=len(g), error_rate=0.0)
    r0 = mhap_amd.synth_reads_from_genome(g, lens, seed=9, error_rate=0.0)
    for q in range(50):
        idx = (int(t0["start"][q]) + np.arange(900)) % len(g)
        w = np.frombuffer(b"ACGT", np.uint8)[g[idx]].tobytes()
        want = w.translate(_COMP)[::-1] if t0["strand"][q] else w
        assert r0.sequence(q).encode() == want


# ---- the aligner reference against brute force ----------------------------------------------------------------------------
def _brute(s1, s2):
    """H of every end cell and, per end cell, every (begin cell, columns, errors) of a path scoring H: all local alignments."""
    m, n = len(s1), len(s2)
    best = {}
    for i0 in range(m):
        for j0 in range(n):
            # paths from (i0, j0) onward; state (i, j, last) -> set of (score, cols, errs); last in "MID" or "" at the start
            states = {(i0, j0, ""): {(0, 0, 0)}}
            order = sorted(((i, j) for i in range(i0, m + 1) for j in range(j0, n + 1)))
            for (i, j) in order:
                for last in ("", "M", "I", "D"):
                    cur = states.get((i, j, last))
                    if not cur:
                        continue
                    for sc, c, e in cur:
                        if i < m and j < n:
                            mis = s1[i] != s2[j]
                            states.setdefault((i + 1, j + 1, "M"), set()).add((sc + (-2 if mis else 2), c + 1, e + int(mis)))
                        if i < m:
                            states.setdefault((i + 1, j, "I"), set()).add((sc - (1 if last == "I" else 2), c + 1, e + 1))
                        if j < n:
                            states.setdefault((i, j + 1, "D"), set()).add((sc - (1 if last == "D" else 2), c + 1, e + 1))
            for (i, j, last), vals in states.items():
                if last == "":
                    continue
                for sc, c, e in vals:
                    best.setdefault((i - 1, j - 1), []).append((sc, i0, j0, c, e))
    return best


@pytest.mark.parametrize("seed", range(40))
def test_align_ref_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    alpha = b"AC" if seed % 2 else b"ACGTN"
    s1 = bytes(rng.choice(list(alpha), int(rng.integers(0, 7))).tolist())
    s2 = bytes(rng.choice(list(alpha), int(rng.integers(0, 7))).tolist())
    got = align_ref.align(s1, s2)
    br = _brute(s1, s2)
    top = max([v[0] for vals in br.values() for v in vals] + [0])
    assert got[0] == top
    if top == 0:
        assert got == (0, -1, -1, -1, -1, 0, 0)
        return
    ends = sorted((j, i) for (i, j), vals in br.items() if max(v[0] for v in vals) == top)
    assert (got[4], got[2]) == ends[0]                            # smallest j, then smallest i
    paths = {(b1, b2, c, e) for sc, b1, b2, c, e in br[(got[2], got[4])] if sc == top}
    assert (got[1], got[3], got[5], got[6]) in paths              # the carried begin, columns and errors are those of an optimal path


def test_align_ref_priority_rules():
    assert align_ref.align(b"ACGT", b"ACGT") == (8, 0, 3, 0, 3, 4, 0)
    assert align_ref.align(b"AAAA", b"CCCC") == (0, -1, -1, -1, -1, 0, 0)
    assert align_ref.align(b"NN", b"NN")[0] == 4                  # N against N matches
    # two equal-scoring copies of the match in s2: the one ending first in s2 wins
    assert align_ref.align(b"ACG", b"ACGTTACG")[3:5] == (0, 2)
    # 7-base deletion in s2: 2*20 - (2 + 6) + 2*20
    s = b"ACGTTGCAAGCTAGCTAGGA" + b"TTTTTTT" + b"CATGCATCGATCGGATCCAA"
    assert align_ref.align(s[:20] + s[27:], s) == (72, 0, 39, 0, 46, 47, 7)
    assert align_ref.rc_bytes(b"ACGTNRYKMBVDHWSX") == b"XSWDHBVKMRYNACGT"


# ---- full and sampled mode against literal transcriptions --------------------------------------------------------------------
def fake_aligner(bases, pairs):
    """Deterministic stand-in for the GPU aligner: good alignments for some pairs, poor ones for others."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 5)
    out = np.zeros((len(pairs), 7), np.int32)
    for q, (ao, al, bo, bl, rc) in enumerate(pairs.tolist()):
        c = min(al, bl)
        good = (ao // 7 + bo // 11 + rc) % 3 != 0
        out[q] = (2 * c, 0, al - 1, 0, bl - 1, c, c // 10 if good else c // 2)
    return out


class Literal:
    """fullEstimate (:886-914), estimateSensitivity / Specificity / PPV (:802-883) as written, over a loaded EstimateROC."""

    def __init__(self, g):
        self.g = g
        self.trees = {}
        for k, n in enumerate(g.seq_to_name):
            self.trees.setdefault(g.chr[k], roc.IntervalTree()).add_interval(int(g.pos[k, 0]), int(g.pos[k, 1]), k)
        self.rand = roc.JavaRandom(0)

    def matches(self, id_, mn):
        k = self.g.index.get(id_)
        if k is None:
            return None
        p1 = self.g.pos[k]
        res = set()
        for k2 in self.trees[self.g.chr[k]].get(int(p1[0]), int(p1[1])):
            id2 = self.g.seq_to_name[k2]
            p2 = self.g.pos[k2]
            if roc.get_range_overlap(int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])) >= mn and id_.lower() != id2.lower():
                res.add(id2)
        return res

    def size(self, a, b):
        p, q = self.g.pos[self.g.index[a]], self.g.pos[self.g.index[b]]
        return roc.get_range_overlap(int(p[0]), int(p[1]), int(q[0]), int(q[1]))

    def overlap_matches(self, a, b):
        ref = self.size(a, b)
        o = self.g.ovl_info.get(roc.ovl_name(a, b))
        if o is None:
            return False
        diff = abs(o.get_size() - ref)
        pct = diff / ref if ref else (math.nan if diff == 0 else math.inf)
        return not (pct > self.g.max_diff)

    def dp(self, a, b):
        return self.g._compute_dp([roc.ovl_name(a, b)])[roc.ovl_name(a, b)]

    def full(self):
        g, names = self.g, self.g.seq_to_name
        tp = fn = tn = fp = 0
        cache = {}
        for i in range(len(names)):
            a = names[i]
            m = cache.setdefault(a, self.matches(a, 0))
            for j in range(i + 1, len(names)):
                b = names[j]
                if not self.overlap_matches(a, b):
                    if b not in m:
                        tn += 1
                    elif self.size(a, b) > g.min_ovl:
                        fn += 1
                elif b in m:
                    tp += 1
                elif self.dp(a, b):
                    tp += 1
                else:
                    fp += 1
        return tp, fn, tn, fp

    def sampled(self):
        g, names, r = self.g, self.g.seq_to_name, self.rand
        tp = fn = tn = fp = 0
        for _ in range(g.trials):
            m = None
            while not m:
                a = names[r.next_int(len(names))]
                m = self.matches(a, g.min_ovl)
            for b in m:
                if self.overlap_matches(a, b):
                    tp += 1
                else:
                    fn += 1
        for _ in range(g.trials):
            a = names[r.next_int(len(names))]
            b = names[r.next_int(len(names))]
            while a.lower() == b.lower():
                b = names[r.next_int(len(names))]
            m = self.matches(a, 0)
            if b not in m:
                if roc.ovl_name(a, b) in g.ovl_names:
                    fp += 1
                else:
                    tn += 1
        ntp = 0
        for _ in range(g.trials):
            ln = 0
            while ln < g.min_ovl:
                name = g.ovl_to_name[r.next_int(len(g.ovl_to_name))]
                o = g.ovl_info[name]
                ln = roc.get_range_overlap(o.afirst, o.asecond, o.bfirst, o.bsecond)
            a, b = name.split("_")[:2]
            m = self.matches(a, 0)
            if m is not None and b in m:
                ntp += 1
            elif self.dp(a, b):
                ntp += 1
        return tp, fn, tn, fp, ntp / g.trials


def _fixture(tmp_path, n=400, L=2000, seed=21, cov=10.0):
    fa = mhap_amd.synth_reads(n, L, seed=seed, coverage=cov, error_rate=0.15)
    t, G = mhap_amd.synth_truth(n, L, seed=seed, coverage=cov, error_rate=0.15)
    m4 = tmp_path / "truth.m4"
    workloads.write_truth_m4(m4, t, G)
    fasta = tmp_path / "reads.fasta"
    workloads.write_fasta(fa, fasta, prefix="")
    rng = np.random.default_rng(seed)
    s, e = t["start"], t["start"] + t["span"]
    lines = []

    def rec(a, b, a1, a2, b1, b2, rc):
        lines.append(f"{a + 1} {b + 1} 0.2 100 0 {a1} {a2} {L} {rc} {b1} {b2} {L}")

    for a in range(n):
        for b in range(a + 1, n):
            lo, hi = max(s[a], s[b]), min(e[a], e[b])
            if hi - lo <= 0 or e[a] > G or e[b] > G:
                continue
            f = rng.choice([1.0, 1.0, 0.6, 1.5, 1.2])        # size noise: under and over 30 %
            ln = int(min(L, (hi - lo) * f))
            if rng.random() < 0.15:
                continue                                      # missed
            rc = int(t["strand"][a] != t["strand"][b])
            rec(a, b, 0, ln, 0, ln, rc)
            if rng.random() < 0.05:
                rec(b, a, 0, max(1, ln - 50), 0, max(1, ln - 50), rc)   # duplicate pair, shorter
    for _ in range(300):                                      # false records
        a, b = rng.integers(0, n, 2)
        if a != b:
            ln = int(rng.integers(100, L))
            rec(int(a), int(b), 0, ln, L - ln, L, int(rng.integers(0, 2)))
    wrapped = np.nonzero(e > G)[0]
    for a in wrapped[:3]:                                     # reads outside the truth
        rec(int(a), int((a + 1) % n), 0, 1500, 0, 1500, 0)
    ovl = tmp_path / "ovl.txt"
    _write(ovl, lines)
    return fa, t, G, str(m4), str(ovl), str(fasta)


@pytest.mark.parametrize("load_all,dp", [(False, True), (True, True), (True, False)])
def test_full_mode_matches_literal(tmp_path, load_all, dp):
    fa, t, G, m4, ovl, fasta = _fixture(tmp_path)
    r = roc.estimate_roc(m4, ovl, fasta, min_ovl=500, trials=0, dp=dp, load_all=load_all, aligner=fake_aligner)
    g = roc.EstimateROC(500, 0, dp, load_all=load_all, aligner=fake_aligner)
    g.process_reference(m4)
    g.load_fasta(fasta)
    g.process_overlaps(ovl)
    lit = Literal(g).full()
    assert (r.tp, r.fn, r.tn, r.fp) == lit
    assert r.tp > 0 and r.fn > 0 and r.tn > 0 and r.fp > 0
    assert r.ppv == r.tp / (r.tp + r.fp)
    assert r.lines[2] == "Estimated PPV:\t " + roc.decimal_format(r.ppv)


def test_full_mode_negative_reference_overlap(tmp_path):
    fa = mhap_amd.FastaData.from_strings(["ACGT" * 300] * 3)
    m4 = _write(tmp_path / "t.m4", ["1 c -1 99 0 0 1200 1200 0 0 1200 9000", "2 c -1 99 0 0 1200 1200 0 3000 4200 9000",
                                    "3 c -1 99 0 0 1200 1200 0 600 1800 9000"])
    ovl = _write(tmp_path / "o.txt", ["1 2 0.1 10 0 0 5 1200 0 0 5 1200",      # reference overlap -1799: diff% < 0 accepts
                                      "1 3 0.1 10 0 0 600 1200 0 0 600 1200"])
    r = roc.estimate_roc(m4, ovl, fasta=fa, min_ovl=100, trials=0, dp=True, aligner=fake_aligner)
    g = roc.EstimateROC(100, 0, True, aligner=fake_aligner)
    g.process_reference(m4)
    g.load_fasta(fa)
    g.process_overlaps(ovl)
    assert (r.tp, r.fn, r.tn, r.fp) == Literal(g).full()
    assert r.fp + r.tp == 2


@pytest.mark.parametrize("load_all", [False, True])
def test_sampled_mode_matches_literal(tmp_path, load_all):
    fa, t, G, m4, ovl, fasta = _fixture(tmp_path, seed=22)
    r = roc.estimate_roc(m4, ovl, fasta, min_ovl=500, trials=700, dp=True, load_all=load_all, aligner=fake_aligner)
    g = roc.EstimateROC(500, 700, True, load_all=load_all, aligner=fake_aligner)
    g.process_reference(m4)
    g.load_fasta(fasta)
    g.process_overlaps(ovl)
    tp, fn, tn, fp, ppv = Literal(g).sampled()
    assert (r.tp, r.fn, r.tn, r.fp, r.ppv) == (tp, fn, tn, fp, ppv)
    assert r.lines[0] == "Estimated sensitivity:\t" + roc.decimal_format(tp / (tp + fn))


def test_error_paths(tmp_path):
    fa = mhap_amd.FastaData.from_strings(["ACGT" * 300] * 2)
    m4 = _write(tmp_path / "t.m4", ["1 c -1 99 0 0 1200 1200 0 0 1200 9000", "2 c -1 99 0 0 1200 1200 0 5000 6200 9000"])
    ovl = _write(tmp_path / "o.txt", ["1 2 0.1 10 0 0 100 1200 0 0 100 1200"])
    with pytest.raises(roc.RocError, match="estimateSensitivity would loop forever"):
        roc.estimate_roc(m4, ovl, fa, min_ovl=100, trials=10, aligner=fake_aligner)
    m4b = _write(tmp_path / "t2.m4", ["1 c -1 99 0 0 1200 1200 0 0 1200 9000", "2 c -1 99 0 0 1200 1200 0 500 1700 9000"])
    with pytest.raises(roc.RocError, match="estimatePPV would loop forever"):
        roc.estimate_roc(m4b, ovl, fa, min_ovl=500, trials=10, aligner=fake_aligner)
    m4c = _write(tmp_path / "t3.m4", ["1 c -1 99 0 0 1200 1200 0 0 1200 9000", "2 d -1 99 0 0 1200 1200 0 500 1700 9000"])
    with pytest.raises(roc.RocError, match="comparing wrong chromosomes betweeen sequences 1 and sequence 2"):
        roc.estimate_roc(m4c, ovl, fa, min_ovl=100, trials=0)
    bad = _write(tmp_path / "bad.txt", ["1 2 0.1 10 0 700 100 1200 0 0 100 1200"])
    with pytest.raises(roc.RocError, match="begin 700, end 100, length 1200"):
        roc.estimate_roc(m4, bad, fa, min_ovl=10, trials=0, dp=True, aligner=fake_aligner)   # negative reference overlap: DP
    with pytest.raises(roc.RocError, match="No sequence matches"):
        roc.estimate_roc(m4b, _write(tmp_path / "e.txt", [""]), fa, trials=0)


def test_cli_usage_and_lines(tmp_path):
    fa, t, G, m4, ovl, fasta = _fixture(tmp_path, n=120, seed=5)
    p = subprocess.run([sys.executable, "-m", "mhap_amd.roc", m4], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 1 and "Minimum overlap length" in p.stderr
    p = subprocess.run([sys.executable, "-m", "mhap_amd.roc", m4, ovl, fasta, "500", "0", "false"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = roc.estimate_roc(m4, ovl, fasta, min_ovl=500, trials=0)
    assert p.stdout == "".join(x + "\n" for x in r.lines)
    assert "Computing full statistics" in p.stderr and "Total time" in p.stderr
