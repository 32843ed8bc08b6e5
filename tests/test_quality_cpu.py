"""Base qualities without a GPU: the restatement (tests/quality_ref.py) worked by hand clause by clause of the "base qualities"
paragraph of include/mhap_hip.h, its bytes against the two call restatements, the FASTQ formatter, the tools' flag checks, and the
ranking condition on the quality workload with the CPU aligner's paths."""
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
import unitig_consensus_ref as ucr  # noqa: E402
from mhap_amd import correct, fastq, graph  # noqa: E402

A, C, G, T, N = b"ACGTN"


def row(base=(0, 0, 0, 0), dele=0, span=0, ins=()):
    """One position's 24 counters; ins: up to four (A, C, G, T) tuples."""
    r = np.zeros(24, np.int64)
    r[0:4] = base
    r[4], r[5] = dele, span
    for k, v in enumerate(ins):
        r[6 + 4 * k:10 + 4 * k] = v
    return r


def one(r, own, t=0, L=3, min_cov=4, per_vote=30, cap=60):
    """(bytes, qualities) of one position."""
    out = qref.position(r, own, t, L, min_cov)
    return bytes(e for e, _ in out), [0 if m is None else qref.q_of(m, per_vote, cap) for _, m in out]


# ---- the rule, clause by clause ---------------------------------------------------------------------------------------------------------

def test_own_agrees_and_own_disagrees():
    # 6 for G and own = G: s = 7 of n = 7, m = 7: 21.  span 6 and no insertion: m_stop = 7, not smaller
    assert one(row((0, 0, 6, 0), span=6), G) == (b"G", [21])
    # 5 for G, 1 for T, own = G: s = 6 of n = 7, m = 5
    assert one(row((0, 0, 5, 1), span=6), G) == (b"G", [15])
    # own = T against 2 for G and 3 for T: T stays with s = 4 of n = 6, m = 2
    assert one(row((0, 0, 2, 3), span=5), T) == (b"T", [6])


def test_a_substituted_byte():
    # own = A, 5 for G: G wins with s = 5 (own does not count for it) of n = 6, m = 4
    assert one(row((0, 0, 5, 0), span=5), A) == (b"G", [12])
    # own = A, 3 for G, 2 for C: G with s = 3 of n = 6, m = 0
    assert one(row((0, 2, 3, 0), span=5), A) == (b"G", [0])


def test_low_coverage():
    # d = 3 < 4: own stays; s = base[own] + 1
    assert one(row((0, 0, 3, 0), span=3), G) == (b"G", [12])          # s = 4 of n = 4
    assert one(row((0, 0, 3, 0), span=3), A) == (b"A", [0])           # s = 1 of n = 4: m = -2
    assert one(row(), C) == (b"C", [3])                                # nobody voted: m = 1
    assert one(row(), C, min_cov=1) == (b"C", [3])                     # the same through the other branch


def test_own_n_gives_zero():
    assert one(row(), N) == (b"N", [0])
    assert one(row((0, 0, 3, 0), span=3), N) == (b"N", [0])           # low coverage keeps N
    assert one(row((0, 0, 0, 0), dele=4, span=4), N, min_cov=9) == (b"N", [0])
    # N outvoted is a substituted byte like any other: s = 5 of n = 6
    assert one(row((0, 0, 5, 0), span=5), N) == (b"G", [12])
    # every base count 0 and enough depth (all deletions would delete; 1 del of d = 1 with min_cov 1 does not): own = N stays, fixed 0
    assert one(row(dele=1, span=1), N, min_cov=1) == (b"N", [0])


def test_one_byte_insertion_whose_stop_margin_is_smaller():
    # base: 6 for G, own G: m = 7.  ins[0] T = 5 of span 6: m = 3.  ins[1] A = 3: m_stop = 7 - 6 = 1 on the inserted byte
    r = row((0, 0, 6, 0), span=6, ins=[(0, 0, 0, 5), (3, 0, 0, 0)])
    assert one(r, G) == (b"GT", [21, 3])
    # without a second-slot vote the stop margin is 7 and the inserted byte keeps its own 3
    r = row((0, 0, 6, 0), span=6, ins=[(0, 0, 0, 5)])
    assert one(r, G) == (b"GT", [21, 9])
    # no insertion called, but 3 of span 6 wanted one: the base byte's margin becomes 7 - 6 = 1
    r = row((0, 0, 6, 0), span=6, ins=[(0, 0, 0, 3)])
    assert one(r, G) == (b"G", [3])


def test_four_byte_insertion_has_no_stop_margin():
    r = row((0, 0, 6, 0), span=6, ins=[(6, 0, 0, 0), (0, 5, 0, 0), (0, 0, 4, 0), (0, 0, 0, 6)])
    assert one(r, G) == (b"GACGT", [21, 15, 9, 3, 15])
    # three bytes: the fourth slot's 3 votes stop the junction with 7 - 6 = 1 on the third
    r = row((0, 0, 6, 0), span=6, ins=[(6, 0, 0, 0), (0, 5, 0, 0), (0, 0, 4, 0), (0, 0, 0, 3)])
    assert one(r, G) == (b"GACG", [21, 15, 9, 3])


def test_the_last_position_has_no_stop_margin():
    r = row((0, 0, 6, 0), span=0, ins=[(0, 0, 0, 3)])               # (no view continues past L - 1; the counters are taken as they are)
    assert one(r, G, t=2, L=3) == (b"G", [21])
    assert one(r, G, t=1, L=3) == (b"G", [0])                        # m_stop = 1 - 6
    assert one(row(), G, t=0, L=1) == (b"G", [3])


def test_span_below_min_cov_with_an_insertion_majority_gives_zero():
    # span 3 < 4: decide() calls no insertion, but 3 of 3 voted for one: m_stop = 4 - 6 = -2
    r = row((0, 0, 6, 0), span=3, ins=[(0, 0, 0, 3)])
    assert one(r, G) == (b"G", [0])
    assert one(r, G, min_cov=3) == (b"GT", [21, 6])                   # with enough span it is called: m = 6 - 4, m_stop = 4


def test_a_called_deletion_emits_nothing():
    assert one(row((0, 0, 1, 0), dele=5, span=6), G) == (b"", [])
    # ... and with an insertion the inserted byte is the only one, and takes the stop margin
    r = row((0, 0, 1, 0), dele=5, span=6, ins=[(0, 0, 0, 6), (2, 0, 0, 0)])
    assert one(r, G) == (b"T", [9])                                    # min(12 - 7, 7 - 4) = 3
    s, q = qref.call(b"GGG", np.array([row((0, 0, 6, 0), span=6), row((0, 0, 1, 0), dele=5, span=6), row((0, 0, 6, 0))]), per_vote=30)
    assert s == b"GG" and q.tolist() == [21, 21] and q.dtype == np.uint8


def test_the_cap_is_reached():
    r = row((0, 0, 30, 0), span=30)
    assert one(r, G) == (b"G", [60])                                   # m = 31: 93 capped
    assert one(r, G, cap=93) == (b"G", [93])
    assert one(r, G, cap=1) == (b"G", [1])
    assert one(row((0, 0, 19, 0), span=19), G) == (b"G", [60])        # m = 20: exactly 60


@pytest.mark.parametrize("per_vote,want", [(1, [0, 0, 0, 1, 1, 2, 6]), (7, [0, 0, 0, 7, 13, 14, 44]), (1000, [0, 0, 60, 60, 60, 60, 60])])
def test_rule_variants(per_vote, want):
    """Q over the margins -3, 0, 1, 10, 19, 20, 63: C integer division, the cap at 60."""
    assert [qref.q_of(m, per_vote, 60) for m in (-3, 0, 1, 10, 19, 20, 63)] == want
    assert qref.q_of(63, per_vote, 93) == min(93, per_vote * 63 // 10)


def test_parameters_out_of_range():
    for pv, cap in ((0, 60), (1001, 60), (30, 0), (30, 94), (-1, -1)):
        with pytest.raises(ValueError):
            qref.call(b"A", np.zeros((1, 24), np.int64), per_vote=pv, cap=cap)
    qref.call(b"A", np.zeros((1, 24), np.int64), per_vote=1000, cap=93)


# ---- the bytes are the call's ------------------------------------------------------------------------------------------------------------

def test_sequence_agreement_on_random_counters():
    """Random counter rows that reach every branch: the restated bytes are consensus_ref's and unitig_consensus_ref's."""
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
    for min_cov in (1, 4, 7):
        seq, quals = qref.call(own, v, min_cov)
        want, st = ref.call_read(0, min_cov)
        assert seq == want and len(quals) == len(seq)
        assert st[2] > 0 and st[3] > 0 and st[4] > 0 and (min_cov == 1 or st[5] > 0)
        assert ucr.call_unitig(own, v, min_cov)[0] == seq
        assert qref.histogram([quals]).sum() == len(seq) and int(quals.max()) <= 60 and quals.tolist() == qref.call(own, v, min_cov, 15, 60)[1].tolist()


# ---- FASTQ ------------------------------------------------------------------------------------------------------------------------------

def test_fastq_formatter():
    text = fastq.format_record("7 len=4 sub=0 del=0 ins=0 low=4", b"ACGT", np.array([0, 9, 60, 93], np.uint8))
    assert text == "@7 len=4 sub=0 del=0 ins=0 low=4\nACGT\n+\n!*]~\n"
    seq_line, qual_line = text.split("\n")[1], text.split("\n")[3]
    assert len(seq_line) == len(qual_line)
    assert fastq.quality_string([93]) == "~" and fastq.quality_string([0]) == "!"
    assert fastq.format_record("e", b"", np.zeros(0, np.uint8)) == "@e\n\n+\n\n"
    assert fastq.format_fastq(["a", "b"], [b"A", b""], [[1], []]) == "@a\nA\n+\n\"\n@b\n\n+\n\n"
    with pytest.raises(ValueError):
        fastq.format_record("x", b"AC", [1])
    with pytest.raises(ValueError):
        fastq.quality_string([94])


def test_the_tools_share_the_header_fields_and_the_line():
    stats = np.array([[5, 4, 1, 1, 0, 2]], np.int32)
    assert correct.format_fasta([9], [b"ACGT"], stats) == ">9 len=4 sub=1 del=1 ins=0 low=2\nACGT\n"
    assert correct.header_fields([9], stats) == ["9 len=4 sub=1 del=1 ins=0 low=2"]
    assert graph.consensus_names([0, 1]) == ["utg000001l", "utg000002c"]
    from mhap_amd import api
    h = np.zeros(94, np.int64)
    h[3], h[12], h[60] = 5, 2, 3
    assert api.quality_counts_line(h) == qref.counts_line(h) == "Qualities: 10 bytes, 5 below Q10, 7 below Q20, mean 21.9"
    assert api.quality_counts_line(np.zeros(94, np.int64)) == "Qualities: 0 bytes, 0 below Q10, 0 below Q20, mean 0.0"
    assert api.QUALITY_BINS == qref.BINS == 94
    p = api.QualityParams()
    assert (p.per_vote, p.cap) == (qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP)


@pytest.mark.parametrize("argv", [["--quality-per-vote", "20"], ["--quality-cap", "40"], ["--fastq", "c.fq", "--quality-per-vote", "0"],
                                  ["--fastq", "c.fq", "--quality-per-vote", "1001"], ["--fastq", "c.fq", "--quality-cap", "94"],
                                  ["--fastq", "c.fq", "--quality-cap", "0"]])
def test_correct_tool_refuses_flags(argv, capsys):
    with pytest.raises(SystemExit) as e:
        correct.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and "--quality-" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--unitigs", "u.gfa", "--consensus-fastq", "c.fq"], ["--unitigs", "u.gfa", "--consensus", "--quality-cap", "40"],
                                  ["--unitigs", "u.gfa", "--consensus", "--consensus-fastq", "c.fq", "--quality-per-vote", "0"],
                                  ["--unitigs", "u.gfa", "--consensus", "--consensus-fastq", "c.fq", "--quality-cap", "94"]])
def test_graph_tool_refuses_flags(argv, capsys):
    with pytest.raises(SystemExit) as e:
        graph.main(["overlaps.txt", "reads.fasta"] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and ("--quality-" in err or "--consensus-fastq" in err)


def test_the_header_has_the_paragraph():
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = fh.read()
    assert "base qualities" in text and "#define MHAP_QUALITY_BINS 94\n" in text and "no quality values" not in text
    for name in ("mhap_quality_default_params", "mhap_correct_quality", "mhap_consensus_quality"):
        assert name + "(" in text


# ---- ranking on the reference alone ----------------------------------------------------------------------------------------------------

def test_ranking_on_the_quality_workload():
    """quality_workload(7), paths from align_paths_ref, min_cov 4, the defaults: the wrong-byte share among bytes at or above the
    median quality is below one quarter of the share among bytes below it.  Measured: 35 of 15 955 (0.22 %) against 774 of 14 267
    (5.4 %); the median is 16 (a net vote of 11; 33 under the slope of 30 the rule was first tried with, the same split)."""
    reads, truths, bases, pairs, meta = cref.quality_workload(7)
    results, offsets, ops = apr.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    ref = cref.Consensus(reads, range(1, len(reads) + 1))
    ref.add(recs, offsets, ops)
    quals, wrongs = [], []
    for r in range(len(reads)):
        seq, q = qref.call(reads[r], ref.votes[r], 4)
        assert seq == ref.call_read(r, 4)[0]
        quals.append(q)
        wrongs.append(qref.wrong_bytes(seq, truths[r]))
    med, (w_lo, n_lo), (w_hi, n_hi) = qref.ranking(quals, wrongs)
    print(f"median {med}: below {w_lo} wrong of {n_lo}, at or above {w_hi} wrong of {n_hi}")
    assert n_lo > 0 and n_hi > 0 and w_hi / n_hi < 0.25 * (w_lo / n_lo)
