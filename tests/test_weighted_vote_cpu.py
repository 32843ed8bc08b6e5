"""The quality-weighted votes without a GPU: the restatement (tests/weighted_vote_ref.py) worked by hand clause by clause of the
"quality-weighted votes" section of include/mhap_hip.h, the identity with the unweighted restatements when every quality lies in the
middle class, and the wrong bytes of the weighted workload against the unweighted call on the same reads and paths."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_paths_ref as apr  # noqa: E402
import consensus_ref as cref  # noqa: E402
import quality_ref as qref  # noqa: E402
import weighted_vote_ref as wref  # noqa: E402

A, C, G, T, N = b"ACGTN"
LO, HI = 7, 20          # the thresholds of the hand-made cases: Q5 weighs 1, Q14 weighs 2, Q30 weighs 3
Q1, Q2, Q3 = 5, 14, 30


def row(base=(0, 0, 0, 0), dele=0, span=0, ins=()):
    r = np.zeros(24, np.int64)
    r[0:4] = base
    r[4], r[5] = dele, span
    for k, v in enumerate(ins):
        r[6 + 4 * k:10 + 4 * k] = v
    return r


def one(r, own, own_w=2, t=0, L=3, min_cov=4, per_vote=30, cap=60):
    out = wref.position(r, own, own_w, t, L, min_cov)
    return bytes(e for e, _ in out), [0 if m is None else wref.q_of(m, per_vote, cap) for _, m in out]


# ---- the weight and the votes -----------------------------------------------------------------------------------------------------------

def test_the_weight_of_a_base():
    assert [wref.weight(q, 7, 20) for q in (0, 6, 7, 19, 20, 93)] == [1, 1, 2, 2, 3, 3]
    assert [wref.weight(q, 0, 0) for q in (0, 93)] == [3, 3] and [wref.weight(q, 0, 93) for q in (0, 92, 93)] == [2, 2, 3]
    assert [wref.weight(q, 93, 93) for q in (92, 93)] == [1, 3]
    for lo, hi in ((-1, 5), (6, 5), (0, 94)):
        with pytest.raises(ValueError):
            wref.check_weights(lo, hi)
    assert wref.CAP == 21845 and wref.NEUTRAL == 2
    assert (wref.DEFAULT_Q_LO, wref.DEFAULT_Q_HI) in wref.CANDIDATES


def test_the_votes_of_a_view():
    # M adds w(q_e); Del and span add 2; the k-th inserted byte adds w(q_e) to its slot; N votes nothing but takes its slot
    view = [("M", 3, A, Q1), ("M", 4, C, Q3), ("Ins", G, Q3), ("Ins", N, Q3), ("Ins", T, Q1), ("Del", 5), ("M", 6, N, Q3), ("M", 7, T, Q2)]
    assert wref.tally_weighted(view, LO, HI) == [
        (3, 0, 1), (3, cref.SPAN, 2), (4, 1, 3), (4, cref.INS0 + 2, 3), (4, cref.INS0 + 8 + 3, 1), (4, cref.SPAN, 2), (5, cref.DEL, 2),
        (5, cref.SPAN, 2), (6, cref.SPAN, 2), (7, 3, 2)]
    # a fifth inserted byte votes nothing
    view = [("M", 0, A, Q2)] + [("Ins", C, Q3)] * 5 + [("M", 1, A, Q2)]
    got = wref.tally_weighted(view, LO, HI)
    assert [c for _, c, _ in got] == [0, cref.INS0 + 1, cref.INS0 + 5, cref.INS0 + 9, cref.INS0 + 13, cref.SPAN, 0]


@pytest.mark.parametrize("to_rc", [0, 1])
def test_the_quality_is_that_of_the_stored_byte(to_rc):
    """One record, both views: every evidence quality is the one stored with the byte the evidence came from."""
    s1, sb = b"ACGTACGGTA", b"TTACGTCGGTC"
    q1, qb = np.arange(10, 20), np.arange(40, 51)
    s2 = cref.rc_bytes(sb) if to_rc else sb
    runs = [(3 << 4) | 7, (1 << 4) | 2, (2 << 4) | 8, (1 << 4) | 1, (2 << 4) | 7]      # 3=, 1D, 2X, 1I, 2=: rows 1 .. 8, columns 2 .. 9
    va, vb = wref.views_with_qualities(s1, q1, sb, qb, 1, 2, runs, to_rc)
    for col in va:
        if col[0] != "Del":
            e, q = col[-2], col[-1]
            at = int(q) - 40                                  # the stored position in B that the quality names
            assert (cref.complement(sb[at]) if to_rc else sb[at]) == e
    assert [c[-1] for c in va if c[0] != "Del"] == ([48 - x for x in range(8)] if to_rc else [42 + x for x in range(8)])
    for col in vb:
        if col[0] != "Del":
            e, q = col[-2], col[-1]
            assert (cref.complement(s1[int(q) - 10]) if to_rc else s1[int(q) - 10]) == e
    plain_a, plain_b = cref.views_of(s1, s2, 1, 2, runs, to_rc, len(sb))
    assert [c[:3] if c[0] == "M" else c[:2] for c in va] == plain_a and [c[:3] if c[0] == "M" else c[:2] for c in vb] == plain_b
    # the weighted tally casts consensus_ref.tally's votes, in its order
    for view, plain in ((va, plain_a), (vb, plain_b)):
        assert [(t, c) for t, c, _ in wref.tally_weighted(view, LO, HI)] == cref.tally(plain)


# ---- the call, clause by clause ---------------------------------------------------------------------------------------------------------

def test_low_is_twice_min_cov():
    assert one(row((0, 0, 7, 0), span=8), A) == (b"A", [0])              # d = 7 < 8: own stays; s = 2 of n = 9
    assert one(row((0, 0, 8, 0), span=8), A)[0] == b"G"                   # d = 8: called


def test_own_votes_with_its_weight():
    # 3 for G against own = T: a Q5 own (1) loses, a Q14 own (2) loses, a Q30 own (3) ties and stays
    r = row((0, 0, 3, 5), span=8)
    assert one(r, T, 1)[0] == b"T"
    r = row((0, 0, 8, 5), span=12)
    assert one(r, T, 1)[0] == b"G" and one(r, T, 2)[0] == b"G" and one(r, T, 3)[0] == b"T"
    # the margin's own term is the weight: s = 5 + 3 of n = 16
    assert one(r, T, 3) == (b"T", [0])
    assert one(row((0, 0, 0, 9), span=12), T, 3) == (b"T", [18])          # s = 12 of n = 12: m = 12, 30 * 12 / 20 (m_stop = 14)
    assert one(row((0, 0, 0, 9), span=12), T, 1) == (b"T", [15])          # s = 10 of n = 10


def test_a_deletion_needs_more_than_half_of_the_total():
    # del 6 of d = 10: total 12 with a neutral own: 12 > 12 fails; total 11 with a weak own: called
    r = row((0, 0, 4, 0), dele=6, span=10)
    assert one(r, G, 2)[0] == b"G" and one(r, G, 1) == (b"", [])


def test_the_junction():
    # span 7 < 8: no insertion however many votes; span 8: 2 m > span + 2 needs m >= 6
    assert one(row((0, 0, 8, 0), span=7, ins=[(7, 0, 0, 0)]), G)[0] == b"G"
    assert one(row((0, 0, 8, 0), span=8, ins=[(5, 0, 0, 0)]), G)[0] == b"G"
    assert one(row((0, 0, 8, 0), span=8, ins=[(6, 0, 0, 0)]), G) == (b"GA", [15, 3])      # base m = 10; ins m = 12 - 10 = 2; m_stop = 10
    # the stop margin is span + 2 - 2 top: 4 votes in the next slot leave 10 - 8 = 2 on the inserted byte, 5 leave 0
    assert one(row((0, 0, 8, 0), span=8, ins=[(8, 0, 0, 0), (0, 4, 0, 0)]), G) == (b"GA", [15, 3])
    assert one(row((0, 0, 8, 0), span=8, ins=[(8, 0, 0, 0), (0, 5, 0, 0)]), G) == (b"GA", [15, 0])
    assert one(row((0, 0, 8, 0), span=8, ins=[(0, 0, 0, 4)]), G) == (b"G", [3])           # not called, but wanted: m_stop = 2
    assert one(row((0, 0, 8, 0), span=8, ins=[(0, 0, 0, 4)]), G, t=2, L=3) == (b"G", [15])  # the last position has no junction


def test_n_and_the_fixed_zero():
    assert one(row((0, 0, 8, 0), span=8), N) == (b"G", [9])               # N outvoted: s = 8 of n = 10, m = 6
    assert one(row(dele=2, span=2), N, min_cov=1) == (b"N", [0])          # total = 4, 2 del = 4: not deleted; own stays, fixed 0
    assert one(row(), N) == (b"N", [0])


def test_q_is_per_vote_over_twenty():
    assert [wref.q_of(m, 15, 60) for m in (-2, 0, 1, 2, 3, 40, 80, 200)] == [0, 0, 0, 1, 2, 30, 60, 60]
    assert [wref.q_of(2 * m, 15, 60) for m in range(0, 50)] == [qref.q_of(m, 15, 60) for m in range(0, 50)]


# ---- the middle class is the unweighted rule ------------------------------------------------------------------------------------------------

def test_middle_class_identity_on_random_counters():
    """Doubled counters and a neutral own: the bytes, the four counts and the qualities of consensus_ref and quality_ref."""
    rng = np.random.default_rng(5)
    L = 600
    v = np.zeros((L, 24), np.int64)
    v[:, 0:4] = rng.integers(0, 4, (L, 4)) * rng.integers(0, 3, (L, 1))
    v[:, 4] = rng.integers(0, 8, L) * (rng.random(L) < 0.3)
    v[:, 5] = rng.integers(0, 9, L)
    v[:, 6:22] = rng.integers(0, 6, (L, 16)) * (rng.random((L, 1)) < 0.4)
    own = bytes(rng.choice(list(b"ACGTN"), L, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tolist())
    ref = cref.Consensus([own], [1])
    ref.votes[0][:] = v
    mid = np.full(L, Q2, np.uint8)
    for min_cov in (1, 4, 7):
        for per_vote, cap in ((15, 60), (7, 93), (1000, 1)):
            seq, quals = qref.call(own, v, min_cov, per_vote, cap)
            want, st = ref.call_read(0, min_cov)
            for own_q in (mid, None):
                got, gq, counts = wref.call(own, own_q, 2 * v, min_cov, per_vote, cap, LO, HI)
                assert got == seq == want and gq.tolist() == quals.tolist() and counts == tuple(st[2:6])


def test_middle_class_identity_on_the_quality_workload():
    """quality_workload(7) with every quality in [q_lo, q_hi): each counter is twice consensus_ref's, and the call is the same."""
    reads, truths, bases, pairs, meta = cref.quality_workload(7)
    results, offsets, ops = apr.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    ids = range(1, len(reads) + 1)
    ref = cref.Consensus(reads, ids)
    ref.add(recs, offsets, ops)
    rng = np.random.default_rng(1)
    w = wref.WeightedConsensus(reads, [rng.integers(LO, HI, len(r)) for r in reads], ids, LO, HI)
    w.add(recs, offsets, ops)
    for r in range(len(reads)):
        assert np.array_equal(w.votes[r], 2 * ref.votes[r])
        seq, st, quals = w.call_read(r, 4)
        assert (seq, st) == ref.call_read(r, 4) and quals.tolist() == qref.call(reads[r], ref.votes[r], 4)[1].tolist()


# ---- the weighted workload --------------------------------------------------------------------------------------------------------------------

# Measured on this restatement with the defaults (7, 20), seeds 11 .. 15, wrong bytes unweighted -> weighted:
#   1001 -> 704, 991 -> 667, 868 -> 588, 1024 -> 736, 938 -> 603; summed 4822 -> 3298, a relative reduction g = 0.316.
# The tests here and on the GPU's own paths (tests/test_weighted_vote_gpu.py) ask for at least g / 2.
SEEDS = (11, 12, 13, 14, 15)
G_MEASURED = (4822 - 3298) / 4822


def workload_wrong_bytes(seed, paths_of):
    """(wrong bytes unweighted, wrong bytes weighted with the defaults) of weighted_workload(seed), min_cov 4, the same reads and paths."""
    reads, quals, truths, bases, pairs, meta = wref.weighted_workload(seed)
    results, offsets, ops = paths_of(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    ids = range(1, len(reads) + 1)
    ref = cref.Consensus(reads, ids)
    ref.add(recs, offsets, ops)
    w = wref.WeightedConsensus(reads, quals, ids)
    w.add(recs, offsets, ops)
    plain = sum(int(qref.wrong_bytes(ref.call_read(r, 4)[0], truths[r]).sum()) for r in range(len(reads)))
    weighted = sum(int(qref.wrong_bytes(w.call_read(r, 4)[0], truths[r]).sum()) for r in range(len(reads)))
    return plain, weighted


_counts = {}


@pytest.mark.parametrize("seed", SEEDS)
def test_weighted_workload_seed(seed):
    """One seed with the CPU aligner's paths: both counts are printed; weighting does not leave more wrong bytes on any seed."""
    _counts[seed] = workload_wrong_bytes(seed, apr.align_pairs_banded_paths)
    print(f"seed {seed}: wrong bytes {_counts[seed][0]} unweighted, {_counts[seed][1]} weighted")
    assert _counts[seed][1] <= _counts[seed][0]


def test_weighted_workload_reduction():
    """Summed over the five seeds, the relative reduction of wrong bytes is at least half of the measured g."""
    for seed in SEEDS:
        if seed not in _counts:
            _counts[seed] = workload_wrong_bytes(seed, apr.align_pairs_banded_paths)
    plain, weighted = (sum(_counts[s][k] for s in SEEDS) for k in (0, 1))
    print(f"wrong bytes over seeds {SEEDS}: {plain} unweighted, {weighted} weighted, reduction {(plain - weighted) / plain:.3f}")
    assert (plain - weighted) / plain >= G_MEASURED / 2


# ---- the tools' switches ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv,word", [(["--weight-q-lo", "5"], "need --weigh-qualities"), (["--weight-q-hi", "30"], "need --weigh-qualities"),
                                       (["--weigh-qualities", "--weight-q-lo", "30", "--weight-q-hi", "20"], "0 <= --weight-q-lo"),
                                       (["--weigh-qualities", "--weight-q-hi", "94"], "0 <= --weight-q-lo")])
def test_tools_refuse_the_thresholds(argv, word, capsys):
    from mhap_amd import correct, graph
    for tool, extra in ((correct, []), (graph, ["--unitigs", "u.gfa", "--consensus"])):
        with pytest.raises(SystemExit) as e:
            tool.main(["overlaps.txt", "reads.fastq"] + extra + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_graph_tool_wants_a_stage_that_votes(capsys):
    from mhap_amd import graph
    assert graph.main(["overlaps.txt", "reads.fastq", "--weigh-qualities"]) == 1
    assert capsys.readouterr().out == "--weigh-qualities weighs the votes of --consensus: give --consensus too.\n"


def test_the_header_has_the_sections():
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = fh.read()
    assert "quality-weighted votes" in text and "FASTQ input" in text and "#define MHAP_WEIGHTED_VIEW_CAP 21845\n" in text
    for name in ("mhap_weight_default_params", "mhap_correct_begin_weighted", "mhap_consensus_begin_weighted", "mhap_fasta_read_qualities",
                 "mhap_fasta_scan_has_qualities", "mhap_fasta_scan_qualities", "mhap_qualities_free"):
        assert name + "(" in text
