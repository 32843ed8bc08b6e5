"""The read-correction contract on the CPU (tests/consensus_ref.py, written from include/mhap_hip.h): hand-made views with the expected
bytes and counts written out, the reversed view of a to_rc record against the same votes cast on the reverse-complemented read, the
quality condition of the plain rule on synthetic reads, and the FASTA writer of `python -m mhap_amd.correct`.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_paths_ref as pref  # noqa: E402
import consensus_ref as cref  # noqa: E402
import handmade_paths as hp  # noqa: E402
from align_ref import rc_bytes  # noqa: E402

A, C, G, T, N = b"ACGTN"
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")


def _m(evidence, start=0):
    """A view of M columns: evidence byte k on target position start + k."""
    return [("M", start + k, e) for k, e in enumerate(evidence)]


def _call(read, views, min_cov=4):
    c = cref.Consensus([read], [1])
    for v in views:
        c.add_view(0, v)
    seq, st = c.call_read(0, min_cov)
    return seq, st, c.votes[0]


def test_substitution_outvoted_three_to_one_plus_own():
    seq, st, votes = _call(b"ACGTA", [_m(b"ACTTA")] * 3 + [_m(b"ACGTA")])
    assert seq == b"ACTTA" and st == (5, 5, 1, 0, 0, 0)            # T 3 against G 1 + own
    assert votes[2, :6].tolist() == [0, 0, 1, 3, 0, 4] and votes[4, 5] == 0     # span: every view continues past 2, none past 4
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 2 + [_m(b"ACGTA")] * 2)
    assert seq == b"ACGTA" and st == (5, 5, 0, 0, 0, 0)            # T 2 against G 2 + own


def _with_del(n_views, n_del):
    """n_views views over ACGTA, n_del of them with position 2 deleted."""
    dele = [("M", 0, A), ("M", 1, C), ("Del", 2), ("M", 3, T), ("M", 4, A)]
    return [dele] * n_del + [_m(b"ACGTA")] * (n_views - n_del)


@pytest.mark.parametrize("n_views,n_del,deleted", [(5, 3, False), (5, 4, True), (6, 3, False), (6, 4, True)])
def test_deletion_boundary(n_views, n_del, deleted):
    """2 del > total with total = d + 1: 6 > 6 no, 8 > 6 yes, 6 > 7 no, 8 > 7 yes."""
    seq, st, votes = _call(b"ACGTA", _with_del(n_views, n_del))
    assert votes[2, cref.DEL] == n_del and votes[2, :4].sum() == n_views - n_del
    assert seq == (b"ACTA" if deleted else b"ACGTA") and st == (5, 4 if deleted else 5, 0, int(deleted), 0, 0)


def _with_ins(n_views, n_ins, ins=b"T"):
    """n_views views over ACGTA, n_ins of them with `ins` inserted after position 1."""
    iv = [("M", 0, A), ("M", 1, C)] + [("Ins", e) for e in ins] + [("M", 2, G), ("M", 3, T), ("M", 4, A)]
    return [iv] * n_ins + [_m(b"ACGTA")] * (n_views - n_ins)


@pytest.mark.parametrize("n_views,n_ins,inserted", [(4, 2, False), (4, 3, True), (5, 3, False), (5, 4, True)])
def test_insertion_boundary(n_views, n_ins, inserted):
    """2 m > span + 1: 4 > 5 no, 6 > 5 yes, 6 > 6 no, 8 > 6 yes."""
    seq, st, votes = _call(b"ACGTA", _with_ins(n_views, n_ins))
    assert votes[1, cref.SPAN] == n_views and votes[1, cref.INS0 + 3] == n_ins
    assert seq == (b"ACTGTA" if inserted else b"ACGTA") and st == (5, 6 if inserted else 5, 0, 0, int(inserted), 0)


def test_minimum_coverage_boundary():
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 3)
    assert seq == b"ACGTA" and st == (5, 5, 0, 0, 0, 5)            # d = min_cov - 1: every position is low and keeps its byte
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 4)
    assert seq == b"ACTTA" and st == (5, 5, 1, 0, 0, 0)            # d = min_cov
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 3, min_cov=3)
    assert seq == b"ACTTA" and st == (5, 5, 1, 0, 0, 0)
    # a view that covers only a part: the rest is low; an insertion needs span >= min_cov as well
    seq, st, _ = _call(b"ACGTA", [_m(b"GT", 2)] * 4)
    assert seq == b"ACGTA" and st == (5, 5, 0, 0, 0, 3)
    seq, st, _ = _call(b"ACGTA", _with_ins(3, 3))
    assert seq == b"ACGTA" and st[4] == 0 and st[5] == 5


def test_tie_rules():
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 2 + [_m(b"ACCTA")] * 2 + [_m(b"ACGTA")])
    assert seq == b"ACGTA" and st[2] == 0                          # G 1 + own = C 2 = T 2: own is among the tied
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 2 + [_m(b"ACCTA")] * 2)
    assert seq == b"ACCTA" and st[2] == 1                          # C 2 = T 2 > G 0 + own: the first of A, C, G, T
    seq, st, _ = _call(b"ACGTA", [_m(b"ACTTA")] * 2 + [_m(b"ACATA")] * 2)
    assert seq == b"ACATA" and st[2] == 1
    # every base count 0: only with own not A, C, G or T, and a deletion that does not win (min_cov 1: 2 > 2 is false)
    seq, st, _ = _call(b"ANA", [[("M", 0, A), ("Del", 1), ("M", 2, A)]], min_cov=1)
    assert seq == b"ANA" and st == (3, 3, 0, 0, 0, 0)
    # an insertion's tie: the first of A, C, G, T
    seq, st, _ = _call(b"ACGTA", _with_ins(3, 3, b"G") + _with_ins(3, 3, b"C"))
    assert seq == b"ACGTA"                                          # 2 * 3 > 6 + 1 is false
    seq, st, _ = _call(b"ACGTA", _with_ins(2, 2, b"G") + _with_ins(2, 2, b"C"), min_cov=1)
    assert seq == b"ACGTA"                                          # 2 * 2 > 4 + 1 is false: a tie can never win


@pytest.mark.parametrize("ins,emitted", [(b"T", b"T"), (b"GATC", b"GATC"), (b"GATCAG", b"GATC")])
def test_insertions_of_one_four_and_six(ins, emitted):
    seq, st, votes = _call(b"ACGTA", _with_ins(4, 4, ins))
    assert seq == b"AC" + emitted + b"GTA" and st == (5, 5 + len(emitted), 0, 0, len(emitted), 0)
    assert votes[1, cref.INS0:cref.INS0 + 16].sum() == 4 * len(emitted) and votes[:, 22:].sum() == 0    # slots beyond 4 vote nowhere
    assert votes[0, cref.INS0:].sum() == 0 and votes[2, cref.INS0:].sum() == 0


def test_insertion_stops_at_the_first_slot_without_a_majority():
    views = _with_ins(4, 4, b"GA")[:2] + _with_ins(4, 4, b"G")[:2]      # slot 0: G 4; slot 1: A 2
    seq, st, _ = _call(b"ACGTA", views)
    assert seq == b"ACGGTA" and st[4] == 1
    views = _with_ins(4, 4, b"GTA")[:3] + _with_ins(4, 4, b"G")[:1]      # slot 0: G 4; slots 1 and 2: 3 of span 4
    seq, st, _ = _call(b"ACGTA", views)
    assert seq == b"ACGTAGTA" and st[4] == 3


def test_n_in_the_target_in_an_m_column_and_inside_an_insertion():
    seq, st, votes = _call(b"ACNTA", [_m(b"ACGTA")] * 4)
    assert seq == b"ACGTA" and st == (5, 5, 1, 0, 0, 0)            # own N casts no vote for itself
    seq, st, votes = _call(b"ACGTA", [_m(b"ACNTA")] * 4)
    assert votes[2, :5].sum() == 0 and votes[2, cref.SPAN] == 4     # an N in an M column votes nothing, the view still spans it
    assert seq == b"ACGTA" and st == (5, 5, 0, 0, 0, 1)            # ... so d = 0 there: low
    seq, st, votes = _call(b"ACGTA", [_m(b"ACTTA")] * 3 + [_m(b"ACNTA")] * 2)
    assert seq == b"ACGTA" and st[5] == 1                          # d = 3 of 5 views
    seq, st, votes = _call(b"ACGTA", _with_ins(4, 4, b"ANG"))
    assert votes[1, cref.INS0 + 0] == 4 and votes[1, cref.INS0 + 4:cref.INS0 + 8].sum() == 0 and votes[1, cref.INS0 + 8 + 2] == 4
    assert seq == b"ACAGTA" and st[4] == 1                         # the N takes slot 1: the call stops there, the G behind it is lost


def test_views_of_a_record_and_the_span_rule():
    # s1 = ACGTTACG, s2 = ACGACCG: 3=, 2I (TT), 1=, 1D (C), 2=
    s1, s2 = b"ACGTTACG", b"ACGACCG"
    runs = [3 << 4 | 7, 2 << 4 | 1, 1 << 4 | 7, 1 << 4 | 2, 2 << 4 | 7]
    va, vb = cref.views_of(s1, s2, 0, 0, runs, False, len(s2))
    assert va == [("M", 0, A), ("M", 1, C), ("M", 2, G), ("Del", 3), ("Del", 4), ("M", 5, A), ("Ins", C), ("M", 6, C), ("M", 7, G)]
    assert vb == [("M", 0, A), ("M", 1, C), ("M", 2, G), ("Ins", T), ("Ins", T), ("M", 3, A), ("Del", 4), ("M", 5, C), ("M", 6, G)]
    ta = cref.tally(va)
    assert sorted(t for t, c in ta if c == cref.SPAN) == [0, 1, 2, 3, 4, 5, 6]
    assert (5, cref.INS0 + 1) in ta and (3, cref.DEL) in ta and (4, cref.DEL) in ta
    tb = cref.tally(vb)
    assert (2, cref.INS0 + 3) in tb and (2, cref.INS0 + 4 + 3) in tb and (4, cref.DEL) in tb


def _record(fid, tid, alen, blen, rc, i0, j0, runs):
    rows = sum(r >> 4 for r in runs if r & 15 != pref.OP_D)
    cols = sum(r >> 4 for r in runs if r & 15 != pref.OP_I)
    n = sum(r >> 4 for r in runs)
    errs = sum(r >> 4 for r in runs if r & 15 != pref.OP_EQ)
    return cref.records_from_results([fid], [tid], [alen], [blen], [rc], [(1, i0, i0 + rows - 1, j0, j0 + cols - 1, n, errs)])


def test_reversed_view_equals_voting_on_the_reverse_complemented_read():
    """An asymmetric path (an insertion group of 2, a mismatch, a deletion group of 3, unequal ends inside both reads) on a to_rc
    record: read B's votes are those of the same path cast on rc(B) as a forward target, turned round — position blen - 1 - t, bases
    complemented, the span of t on the column before it, an insertion group on the other side of its junction with k counted back."""
    rng = np.random.default_rng(5)
    s2 = bytes(rng.choice(list(b"ACGT"), 40).tolist())
    # s1 from s2[3:]: 6 equal, 2 inserted, 5 equal, 1 changed, 4 equal, 3 of s2 skipped, 7 equal; s1 has 2 bytes before and 3 behind
    mid = s2[3:9] + b"GA" + s2[9:14] + bytes([cref.complement(s2[14])]) + s2[15:19] + s2[22:29]
    s1 = b"TT" + mid + b"CCC"
    runs = [6 << 4 | 7, 2 << 4 | 1, 5 << 4 | 7, 1 << 4 | 8, 4 << 4 | 7, 3 << 4 | 2, 7 << 4 | 7]
    fwd = cref.Consensus([s1, s2], [1, 2])
    rev = cref.Consensus([s1, rc_bytes(s2)], [1, 2])
    for _ in range(4):
        fwd.add(_record(1, 2, len(s1), len(s2), 0, 2, 3, runs), [0, len(runs)], runs)
        rev.add(_record(1, 2, len(s1), len(s2), 1, 2, 3, runs), [0, len(runs)], runs)
    assert fwd.votes[0].tolist() == rev.votes[0].tolist()          # view A does not see the difference
    vf, vr = fwd.votes[1], rev.votes[1]
    L = len(s2)
    assert vf[:, :6].sum() > 0
    for t in range(L):
        assert vr[L - 1 - t, :4].tolist() == vf[t, :4][::-1].tolist(), t          # A C G T -> T G C A
        assert vr[L - 1 - t, cref.DEL] == vf[t, cref.DEL]
        assert vr[L - 1 - t, cref.SPAN] == (vf[t - 1, cref.SPAN] if t > 0 else 0), t
    # the insertion group GA after s2[8]: in the reversed view it is TC after position L - 1 - 9
    assert vf[8, cref.INS0 + 2] == 4 and vf[8, cref.INS0 + 4 + 0] == 4
    assert vr[L - 1 - 9, cref.INS0 + 3] == 4 and vr[L - 1 - 9, cref.INS0 + 4 + 1] == 4
    assert vf[:, cref.INS0:].sum() == 8 == vr[:, cref.INS0:].sum()
    # four views and own against nothing else: no tie anywhere, so the corrected read is the reverse complement too
    (a_f, b_f), _ = fwd.call()
    (a_r, b_r), st = rev.call()
    assert a_f == a_r and b_r == rc_bytes(b_f) and b_f != s2
    assert b_f == s2[:9] + b"GA" + s2[9:14] + bytes([cref.complement(s2[14])]) + s2[15:19] + s2[22:]
    assert st[1].tolist() == [40, 39, 1, 3, 2, 14]


def test_cap_skips_whole_views_and_counts_them():
    c = cref.Consensus([b"ACGT"], [1])
    v = _m(b"ACGT")
    inc = np.array(cref.tally(v), np.int64)
    for _ in range(cref.CAP + 2):
        c._apply(0, inc)
    assert c.skipped_views == 2 and c.votes[0].max() == cref.CAP and c.views[0] == cref.CAP


def test_records_that_vote_nothing():
    c = cref.Consensus([b"ACGTACGT", b"ACGTACGT"], [1, 2])
    runs = [8 << 4 | 7]
    same = _record(1, 1, 8, 8, 0, 0, 0, runs)
    c.add(same, [0, 1], runs)                                       # both ids equal
    c.add(_record(1, 2, 8, 8, 0, 0, 0, runs), [0, 0], [])           # no runs: no alignment
    assert c.votes[0].sum() == 0 and c.votes[1].sum() == 0 and c.views == [0, 0]
    seqs, stats = c.call()
    assert seqs == [b"ACGTACGT"] * 2 and stats.tolist() == [[8, 8, 0, 0, 0, 8]] * 2      # unchanged, every position low
    c.add(_record(1, 2, 8, 8, 0, 0, 0, runs), [0, 1], runs)
    c.add(_record(1, 2, 8, 8, 0, 0, 0, runs), [0, 1], runs)         # nothing is de-duplicated
    assert c.votes[0][:, :4].sum() == 16 and c.views == [2, 2]


# ---- hand-made paths (tests/handmade_paths.py, what tests/test_correct_paths_gpu.py is built from) ----------------------------------

def _handmade_paths():
    """(runs, flank_a, flank_b) of every shape the helper is used for: runs_with at both parities of every kind, the parity shift
    included, gap runs next to each other, long runs, a path of one run."""
    out = []
    for kind in "IDX=":
        for at, total in ((62, 129), (63, 129), (64, 129), (65, 129), (127, 131), (128, 131), (1, 3), (2, 5), (4, 9), (5, 11)):
            if kind == ("=" if at % 2 else "X") and not 2 <= at <= total - 3:
                continue                                            # no room for the shift
            out.append((hp.runs_with(kind, 1 + (at + total) % 6, at, total), (at % 4, at % 3), (at % 2, at % 5)))
    for text in ("5=", "3= 2I 3D 1=", "1= 6D 1I 4D 2=", "2= 200I 1= 65D 1X 64= 1X 63=", "1= 1X 1="):
        out.append((hp.cigar(text), (2, 1), (0, 3)))
    return out


@pytest.mark.parametrize("to_rc", [0, 1])
def test_handmade_paths_obey_the_headers_identities(to_rc):
    """Every path tests/handmade_paths.py makes is one mhap_correct_add accepts: '=' at both ends, no two adjacent runs of one code,
    the rows and columns of the runs between the record's aligned ends, equal bytes on '=' and different bytes on 'X' columns; the two
    views of consensus_ref.views_of cover exactly the record's two intervals, one target position after the other; and the votes of
    consensus_ref.tally obey the coverage identity that the GPU tests assert on the session's counters."""
    rng = np.random.default_rng(21)
    for runs, flank_a, flank_b in _handmade_paths():
        assert hp.check_canonical(runs) == [int(r) for r in runs]
        s1, s2 = hp.pair_from_runs(rng, runs, flank_a, flank_b)
        rec = hp.record_for(1, 2, s1, s2, flank_a[0], flank_b[0], runs, to_rc)[0]
        rows, cols = hp.rows_cols(runs)
        assert len(s1) == sum(flank_a) + rows and len(s2) == sum(flank_b) + cols
        assert rec["a1"] == flank_a[0] and rec["a2"] - rec["a1"] + 1 == rows and rec["b2"] - rec["b1"] + 1 == cols
        assert (rec["alen"], rec["blen"], rec["to_rc"]) == (len(s1), len(s2), to_rc)
        j0 = rec["blen"] - rec["b2"] - 1 if to_rc else rec["b1"]
        assert j0 == flank_b[0]
        i, j = flank_a[0], flank_b[0]
        for r in runs:
            for _ in range(r >> 4):
                if r & 15 in (cref.OP_EQ, cref.OP_X):
                    assert (s1[i] == s2[j]) == (r & 15 == cref.OP_EQ), (hp.as_text(runs), i, j)
                i, j = i + (r & 15 != cref.OP_D), j + (r & 15 != cref.OP_I)
        assert (i, j) == (len(s1) - flank_a[1], len(s2) - flank_b[1])
        va, vb = cref.views_of(s1, s2, flank_a[0], flank_b[0], runs, bool(to_rc), len(s2))
        ia, ib = hp.target_intervals([rec])
        assert [c[1] for c in va if c[0] != "Ins"] == list(range(ia[0], ia[1] + 1)) and ia == (flank_a[0], flank_a[0] + rows - 1)
        assert [c[1] for c in vb if c[0] != "Ins"] == list(range(ib[0], ib[1] + 1))
        assert ib == ((flank_b[1], flank_b[1] + cols - 1) if to_rc else (flank_b[0], flank_b[0] + cols - 1))
        assert va[0][0] == va[-1][0] == vb[0][0] == vb[-1][0] == "M"
        for view, interval, length in ((va, ia, len(s1)), (vb, ib, len(s2))):
            votes = np.zeros((length, cref.NCOUNT), np.int64)
            for t, c in cref.tally(view):
                votes[t, c] += 1
            assert hp.coverage_identity(votes, [interval]) == []
            assert hp.coverage_identity(votes, [interval, interval]) != [] and hp.coverage_identity(votes, []) != []      # (it can fail)


def test_runs_with_puts_the_run_where_it_is_asked_for():
    for kind in "IDX":
        for at, total in ((62, 129), (63, 129), (64, 129), (65, 129), (127, 131), (128, 131)):
            for length in (1, 4, 6):
                runs = hp.runs_with(kind, length, at, total)
                assert len(runs) == total and runs[at] == hp.run(kind, length)
                assert all(r >> 4 <= 3 and r & 15 in (cref.OP_EQ, cref.OP_X, cref.OP_I, cref.OP_D) for u, r in enumerate(runs) if u != at)
                assert sum(r & 15 in (cref.OP_I, cref.OP_D) for u, r in enumerate(runs) if u != at) == (2 if kind == "X" and at % 2 == 0 else 0)
    with pytest.raises(ValueError):
        hp.runs_with("I", 1, 0, 5)
    with pytest.raises(ValueError):
        hp.runs_with("=", 1, 1, 5)
    for bad in ("2X 1=", "1= 2I", "1= 2I 3I 1=", "1= 0X 1=", ""):
        with pytest.raises(ValueError):
            hp.check_canonical(hp.cigar(bad) if bad != "1= 0X 1=" else [1 << 4 | 7, 0 << 4 | 8, 1 << 4 | 7])
    assert hp.as_text(hp.cigar("3= 2I1D 10=")) == "3=2I1D10="


def test_a_read_made_to_fit_a_given_s2():
    rng = np.random.default_rng(22)
    runs = hp.cigar("2= 1X 3D 2= 4I 1=")
    _, s2 = hp.pair_from_runs(rng, runs, (1, 1), (2, 3))
    s1, same = hp.pair_from_runs(rng, runs, (1, 1), (2, 3), s2=s2)
    assert same == s2 and len(s1) == 2 + 10
    assert s1[1:3] == s2[2:4] and s1[3] != s2[4] and s1[4:6] == s2[8:10] and s1[10] == s2[10]


@pytest.mark.parametrize("bad,merged", [("3= 2D 3D 3=", "3= 5D 3="), ("3= 2I 3I 3=", "3= 5I 3="), ("2= 1X 1X 2=", "2= 2X 2="), ("2= 3= 1X 1=", "5= 1X 1=")])
@pytest.mark.parametrize("to_rc", [0, 1])
def test_adjacent_runs_of_one_code_are_refused(bad, merged, to_rc):
    """The paths' rule, now a condition of add: two adjacent runs of one code are refused, by the record's index and before any vote,
    unless the earlier one is 2^28 - 1 columns long (a split run); the same columns as one run are accepted."""
    rng = np.random.default_rng(23)
    good = hp.cigar(merged)
    s1, s2 = hp.pair_from_runs(rng, good, (1, 2), (2, 1))
    reads = [s1, rc_bytes(s2) if to_rc else s2]
    rec = hp.record_for(1, 2, s1, s2, 1, 2, good, to_rc)
    c = cref.Consensus(reads, [1, 2])
    runs = good + hp.cigar(bad)
    with pytest.raises(ValueError, match="record 1 has runs"):
        c.add(np.concatenate([rec, rec]), [0, len(good), len(runs)], runs)
    assert c.votes[0].sum() == 0 and c.votes[1].sum() == 0 and c.views == [0, 0] and c.skipped_views == 0
    same = rec.copy()
    same["to_id"] = same["from_id"]
    c.add(same, [0, len(runs) - len(good)], hp.cigar(bad))          # a record of a read with itself votes nothing and is not looked at
    c.add(np.concatenate([rec, rec]), [0, len(good), 2 * len(good)], good + good)
    assert c.views == [2, 2]
    # the last run of one record and the first of the next are not adjacent, and a run of 2^28 - 1 columns may be followed by its code
    # (a path that long fits no read: add gets as far as looking for its columns)
    c.add(np.concatenate([rec, rec]), [0, len(good), 2 * len(good)], good + good)
    split = [cref.RUN_MAX << 4 | cref.OP_EQ, 1 << 4 | cref.OP_EQ]
    with pytest.raises(IndexError):
        c.add(rec, [0, 2], split)


# ---- the quality condition ----------------------------------------------------------------------------------------------------------

QUALITY_SEED = 7


@pytest.fixture(scope="module")
def quality():
    reads, truths, bases, pairs, meta = cref.quality_workload(QUALITY_SEED)
    results, offsets, ops = pref.align_pairs_banded_paths(bases, pairs)
    return reads, truths, pairs, meta, results, offsets, ops


def test_quality_condition_on_the_reference(quality):
    """A 2 500-base genome, 36 reads of 600 - 999 bases at 12 % error (79 / 12 / 9 % insertion / deletion / substitution), random
    strands, one record per pair of reads whose placements share at least 200 bases, band 150 around the true diagonal: the corrected
    reads are less than half as far from their true segments as the raw reads (summed Levenshtein distance).  Seed 7 gives 917 against 3 645 edits, a ratio of 0.252."""
    reads, truths, pairs, meta, results, offsets, ops = quality
    assert len(reads) == 36 and all(600 <= len(t) <= 999 for t in truths) and len(pairs) >= 100
    assert (results[:, 0] > 0).all() and {rc for _, _, rc in meta} == {0, 1}
    c = cref.Consensus(reads, range(1, len(reads) + 1))
    c.add(cref.quality_records(reads, meta, results), offsets, ops)
    seqs, stats = c.call(4)
    raw = sum(cref.levenshtein(r, t) for r, t in zip(reads, truths))
    cor = sum(cref.levenshtein(s, t) for s, t in zip(seqs, truths))
    total = sum(len(t) for t in truths)
    print(f"raw {raw} ({raw / total:.3%}), corrected {cor} ({cor / total:.3%}), ratio {cor / raw:.3f}")
    assert 0.08 * total < raw < 0.16 * total           # the workload is the one stated
    assert cor < 0.5 * raw, (cor, raw)
    assert stats[:, 0].tolist() == [len(r) for r in reads] and stats[:, 1].tolist() == [len(s) for s in seqs]


# ---- the writer of python -m mhap_amd.correct ------------------------------------------------------------------------------------

def test_fasta_writer_and_totals_line():
    from mhap_amd import correct as tool
    stats = np.array([[5, 6, 1, 0, 1, 0], [4, 3, 0, 1, 0, 2], [0, 0, 0, 0, 0, 0]], np.int32)
    text = tool.format_fasta([1, 2, 17], [b"ACTGTA", b"ACT", b""], stats)
    assert text == ">1 len=6 sub=1 del=0 ins=1 low=0\nACTGTA\n>2 len=3 sub=0 del=1 ins=0 low=2\nACT\n>17 len=0 sub=0 del=0 ins=0 low=0\n\n"
    assert tool.totals_line(stats, 4) == ("Corrected 3 reads: 9 bases in, 9 out; 1 substitutions, 1 deletions, 1 insertions, "
                                          "2 positions of low coverage; skipped_views = 4")
    assert tool.format_fasta(["read/7"], [b"A" * 200], [[200, 200, 0, 0, 0, 200]]).split("\n")[1] == "A" * 200     # lines are not wrapped
    off, ops = tool.select_paths(np.array([0, 2, 2, 5]), np.array([1, 2, 3, 4, 5], np.uint32), [2, 0])
    assert off.tolist() == [0, 3, 5] and ops.tolist() == [3, 4, 5, 1, 2]
    off, ops = tool.select_paths(np.array([0, 2]), np.array([1, 2], np.uint32), [])
    assert off.tolist() == [0] and len(ops) == 0


# ---- the driver's refusals: one line on stdout and status 1, before a handle exists (no GPU is touched) --------------------------

def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


@pytest.mark.parametrize("extra,word", [([], "--realign"), (["--realign", "-q", os.path.join(GOLD, "small_queries.fasta")], "-q"),
                                        (["--realign", "--gpus", "2"], "one GPU")])
def test_refusals(tmp_path, extra, word):
    p = _cli(["-s", os.path.join(GOLD, "small_reads.fasta"), "--correct", str(tmp_path / "x.fasta")] + extra, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--correct" in out and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "x.fasta").exists()


def test_refusal_of_dat_input(tmp_path):
    dat = tmp_path / "reads.dat"
    dat.write_bytes(b"")
    p = _cli(["-s", str(dat), "--realign", "--correct", str(tmp_path / "x.fasta")], timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--correct" in out and ".dat" in out, (out, p.stderr[-500:])
