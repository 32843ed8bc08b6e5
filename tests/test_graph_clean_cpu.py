"""The graph-cleaning contract on the CPU (tests/graph_clean_ref.py, written from the "graph cleaning" part of the string-graph
section of include/mhap_hip.h): the hand-made shapes with their expected answers written out, the twin symmetry of both verdicts,
invariance under permutation and splitting of the records, what a cleaned unitig is made of, the text helpers and the driver's
refusal.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graph_clean_ref as cr  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import unitig_ref as ur  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")


def _counts(rounds, tips=0, tip_reads=0, bubbles=0, bubble_reads=0, arcs=0):
    return dict(zip(cr.COUNT_NAMES, (rounds, tips, tip_reads, bubbles, bubble_reads, arcs)))


def _members(u):
    return [u.unitig_start[k + 1] - u.unitig_start[k] for k in range(len(u.unitig_len))]


def _dropped_ids(g, c, what):
    return [i for i, d in zip(g.ids, c.dropped) if d == what]


@pytest.mark.parametrize("mode", ["out", "in", "rc"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_tip_length_boundary(k, mode):
    """A side chain of k reads on read 6 of a backbone of 12: clipped for k <= tip_reads = 4 (an arc and its complement per read
    go with it), kept for k = 5."""
    g, c = cr.cleaned_of(*cr.tip_on_backbone(k, mode))
    assert ur.of_graph(g).counts["unitigs"] == 3
    if k <= 4:
        assert c.counts == _counts(2, 1, k, 0, 0, 2 * k)
        assert _dropped_ids(g, c, cr.TIP) == list(range(101, 101 + k)) and _members(c.unitigs) == [12] and not c.unitigs.links
    else:
        assert c.counts == _counts(1) and not any(c.dropped) and sorted(_members(c.unitigs)) == ([5, 5, 7] if mode == "in" else [5, 6, 6])
        assert c.gfa() == g.gfa()
    assert cr.cleaned_of(*cr.tip_on_backbone(k, mode), tip_reads=5)[1].counts["tip_reads"] == k


def test_terminal_fork_loses_only_its_lesser_arm():
    """Arms of 2 and 3 reads at the end of a chain of 8: the 2-read arm goes and the rest is one unitig of 11; the isolated chain of
    3, the lone reads and the cycle in the same table are untouched."""
    g, c = cr.cleaned_of(*cr.terminal_fork(extras=True))
    assert c.counts == _counts(2, 1, 2, 0, 0, 4) and _dropped_ids(g, c, cr.TIP) == [11, 12]
    assert sorted(_members(c.unitigs)) == [1, 1, 3, 5, 11] and c.unitigs.counts["circular"] == 1 and not c.unitigs.links
    before = ur.of_graph(g)
    assert sorted(_members(before)) == [1, 1, 2, 3, 3, 5, 8] and before.counts["circular"] == 1


def test_terminal_fork_of_equal_arms_is_decided_by_bases_then_by_number():
    for in_a, in_b, gone in ((2500, 2600, [11, 12]), (2700, 2500, [21, 22])):
        g, c = cr.cleaned_of(*cr.terminal_fork(2, 2, in_a, in_b))
        assert c.counts == _counts(2, 1, 2, 0, 0, 4) and _dropped_ids(g, c, cr.TIP) == gone and _members(c.unitigs) == [10]
    g, c = cr.cleaned_of(*cr.terminal_fork(2, 2, 2500, 2500))
    U, verdict = c.history[0]
    arms = [k for k, n in enumerate(_members(U)) if n == 2]
    assert len(arms) == 2 and U.unitig_len[arms[0]] == U.unitig_len[arms[1]] and arms[0] < arms[1]
    assert [verdict[k] for k in arms] == [0, cr.TIP]                                    # the higher number is the lesser rank
    assert c.counts == _counts(2, 1, 2, 0, 0, 4) and _members(c.unitigs) == [10]


def test_star_of_70_tips():
    """70 one-read tips entering one backbone read, more in-links than a wave has lanes.  At the backbone's first read the tips hold
    one another: the best-ranked (equal members and bases: the lowest number) has no holder and stays, 69 go, and the next round
    finds it joined to the backbone, a unitig of 13.  At read 6 the backbone's own first part (5 reads, no candidate) holds the
    junction and all 70 go."""
    g, c = cr.cleaned_of(*cr.star(70, 1))
    U, verdict = c.history[0]
    tips = [k for k, n in enumerate(_members(U)) if n == 1]
    assert len(tips) == 70 and [verdict[k] for k in tips] == [0] + [cr.TIP] * 69
    assert c.counts == _counts(2, 69, 69, 0, 0, 138) and _members(c.unitigs) == [13] and not c.unitigs.links
    g, c = cr.cleaned_of(*cr.star(70, 6))
    assert c.counts == _counts(2, 70, 70, 0, 0, 140) and _members(c.unitigs) == [12]


def test_simple_bubbles():
    g, c = cr.cleaned_of(*cr.bubble((2, 3)))
    assert c.counts == _counts(2, 0, 0, 1, 2, 6) and _dropped_ids(g, c, cr.BUBBLE) == [101, 102] and _members(c.unitigs) == [15]
    g, c = cr.cleaned_of(*cr.bubble((2, 3, 4)))
    assert c.counts == _counts(2, 0, 0, 2, 5, 14) and _dropped_ids(g, c, cr.BUBBLE) == [101, 102, 111, 112, 113] and _members(c.unitigs) == [16]
    # the lesser branch (2 reads) is the longer in bases, so that the limit meets it first: every branch must be within the limit
    long2 = cr.bubble((2, 3), inner=(9000, 2500))
    U = cr.cleaned_of(*long2)[1].history[0][0]
    lesser = U.unitig_len[_members(U).index(2)]
    assert lesser == 20000 + 9000 and U.unitig_len[_members(U).index(3)] == 20000 + 2500 + 2510   # the arcs inside a branch and its last read
    assert cr.cleaned_of(*long2, bubble_bases=lesser)[1].counts == _counts(2, 0, 0, 1, 2, 6)
    kept = cr.cleaned_of(*long2, bubble_bases=lesser - 1)[1]
    assert kept.counts == _counts(1) and sorted(_members(kept.unitigs)) == [2, 3, 6, 6]
    # a second in-link: the first branch is no branch, the other has no sibling (no tips here: the extra read would be one)
    g, c = cr.cleaned_of(*cr.bubble((2, 3), second_in=True), tip_reads=0)
    assert c.counts == _counts(1) and sorted(_members(c.unitigs)) == [1, 2, 3, 6, 6] and c.gfa() == g.gfa()


def test_cascade_of_a_tip_on_a_bubble_branch():
    g, c = cr.cleaned_of(*cr.bubble((2, 3), second_in=True))
    assert [sorted(set(v)) for _, v in c.history] == [[0, cr.TIP], [0, cr.BUBBLE], [0]]
    assert c.counts == _counts(3, 1, 1, 1, 2, 8) and _dropped_ids(g, c, cr.TIP) == [40] and _dropped_ids(g, c, cr.BUBBLE) == [101, 102]
    assert _members(c.unitigs) == [15]
    g, c = cr.cleaned_of(*cr.bubble((2, 3), second_in=True), max_rounds=1)
    assert c.counts == _counts(1, 1, 1, 0, 0, 2) and sorted(_members(c.unitigs)) == [2, 3, 6, 6]


def test_tiles_table():
    g, c = cr.cleaned_of(*cr.tiles())
    assert c.counts == _counts(2, 3, 6, 3, 6, 30) and ur.of_graph(g).counts["unitigs"] - c.unitigs.counts["unitigs"] == 15
    for lo in (5, 540, 1030):
        assert [c.dropped[i - 1] for i in (lo + 12, lo + 13, lo + 32, lo + 33)] == [cr.TIP, cr.TIP, cr.BUBBLE, cr.BUBBLE]


@pytest.fixture(scope="module")
def thinned():
    ids, lengths, _, recs = cr.thinned_layout(2, n_reads=150, genome=120000)
    return (ids, lengths, recs) + cr.cleaned_of(ids, lengths, recs)


def test_thinned_layout_gets_fewer_unitigs_and_both_verdicts_are_twin_symmetric(thinned):
    """Verdicts asserts the symmetry while it decides; here it is asked again, for every unitig of every round."""
    ids, lengths, recs, g, c = thinned
    assert c.counts["tip_unitigs"] > 5 and c.counts["bubble_unitigs"] > 0 and c.counts["rounds"] >= 2
    assert c.unitigs.counts["unitigs"] < ur.of_graph(g).counts["unitigs"]
    for U, verdict in c.history:
        V = cr.Verdicts(U, 4, 50000)
        assert V.verdict == verdict
        for X in range(len(verdict)):
            assert V.popped(X, 0) == V.popped(X, 1) and not (V.candidate(X, 0) and V.candidate(X, 1))
            for o in (0, 1):
                ends = V.branch(X, o)
                twin = V.branch(X, 1 - o)
                assert (ends is None) == (twin is None)
                if ends:
                    (S, s), (E, e) = ends
                    assert twin == ((E, 1 - e), (S, 1 - s))
    assert sum(c.removed) == c.counts["arcs_removed"] and all(g.rows[i][6] for i, x in enumerate(c.removed) if x)


def test_cleaning_depends_on_the_set_of_records_only(thinned):
    ids, lengths, recs, g, c = thinned
    perm = np.random.default_rng(4).permutation(len(recs))
    g2 = sg.Graph(ids, lengths)
    for part in (perm[:len(perm) // 3], perm[len(perm) // 3:len(perm) // 3 + 1], perm[len(perm) // 3 + 1:]):
        g2.add(recs[part])
    g2.finish()
    c2 = cr.Cleaned(g2)
    assert sg.strip_q(g2.rows) == sg.strip_q(g.rows)
    assert c2.dropped == c.dropped and c2.removed == c.removed and c2.counts == c.counts and c2.gfa() == c.gfa()
    a, b = c.unitigs.tables(), c2.unitigs.tables()
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "counts") and a["counts"] == b["counts"]


def _parses(seq, whole):
    """seq is a concatenation of sequences of `whole` (first vertex -> the vertices of an oriented unitig)."""
    at = 0
    while at < len(seq):
        piece = whole.get(seq[at])
        if piece is None or seq[at:at + len(piece)] != piece:
            return False
        at += len(piece)
    return True


@pytest.mark.parametrize("shape", ["thinned", "cascade", "star", "fork"])
def test_a_cleaned_unitig_is_a_concatenation_of_unitigs_that_were_there(thinned, shape):
    if shape == "thinned":
        g, c = thinned[3], thinned[4]
    else:
        g, c = cr.cleaned_of(*{"cascade": cr.bubble((2, 3), second_in=True), "star": cr.star(70, 1), "fork": cr.terminal_fork(extras=True)}[shape])
    before, after = ur.of_graph(g), c.unitigs
    whole = {}
    for k in range(len(before.unitig_len)):
        seq = before.vertex[before.unitig_start[k]:before.unitig_start[k + 1]]
        twin = [v ^ 1 for v in seq[::-1]]
        turns = range(len(seq)) if before.circular[k] else [0]
        for t in turns:
            whole[seq[t]] = seq[t:] + seq[:t]
            whole[twin[t]] = twin[t:] + twin[:t]
    for k in range(len(after.unitig_len)):
        seq = after.vertex[after.unitig_start[k]:after.unitig_start[k + 1]]
        assert not any(c.dropped[v >> 1] or g.contained[v >> 1] for v in seq)
        turns = range(len(seq)) if after.circular[k] else [0]
        assert any(_parses(seq[t:] + seq[:t], whole) for t in turns), k
    in_play = sorted(r for r in range(len(g.ids)) if not g.contained[r] and not c.dropped[r])
    assert sorted(v >> 1 for v in after.vertex) == in_play


def test_parameters_of_the_restatement():
    g = ur.graph_of(*cr.bubble((2, 3), second_in=True))
    assert cr.Cleaned(g, tip_reads=0, bubble_bases=0).counts == _counts(1)
    with pytest.raises(AssertionError):
        cr.Cleaned(g, max_rounds=0)
    empty = ur.graph_of([], [], np.zeros(0, sg.RECORD_DTYPE))
    assert cr.Cleaned(empty).counts == _counts(1) and cr.Cleaned(empty).gfa() == "H\tVN:Z:1.0\n"


def test_text_helpers_and_the_header():
    import mhap_amd
    mhap_amd.load_library()                                                             # every new entry point resolves
    assert tuple(mhap_amd.api.CLEAN_COUNTS) == cr.COUNT_NAMES
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = fh.read()
    assert f"#define MHAP_CLEAN_COUNTS {len(cr.COUNT_NAMES)}\n" in text and "tip_reads (4), bubble_bases (50 000), max_rounds (16)" in text
    assert mhap_amd.api.clean_counts_line(range(1, 7)) == "Cleaned in 1 rounds: 2 tips (3 reads), 4 bubbles (5 reads), 6 arcs removed"
    g, c = cr.cleaned_of(*cr.bubble((2, 3), second_in=True))
    rows = np.array(g.rows, np.int32)
    assert mhap_amd.format_gfa(g.ids, g.lengths, g.contained, rows) == g.gfa()
    assert mhap_amd.format_gfa(g.ids, g.lengths, g.contained, rows, np.array(c.dropped, np.uint8), np.array(c.removed, np.uint8)) == c.gfa()
    assert c.gfa() != g.gfa() and "S\t40\t" in g.gfa() and "S\t40\t" not in c.gfa()


@pytest.mark.parametrize("flag", [["--gfa-clean"], ["--gfa-tip-reads", "3"], ["--gfa-bubble-bases", "10"], ["--gfa-clean-rounds", "2"]])
def test_driver_refuses_cleaning_without_gfa(tmp_path, flag):
    p = subprocess.run([CLI, "-s", os.path.join(GOLD, "small_reads.fasta"), "--realign"] + flag, capture_output=True, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and flag[0] in out and "--gfa too" in out, (out, p.stderr[-500:])


def test_driver_refuses_negative_values_and_both_tools_list_the_flags(tmp_path):
    for flag in (["--gfa-tip-reads", "-1"], ["--gfa-bubble-bases", "-5"], ["--gfa-clean-rounds", "0"]):
        p = subprocess.run([CLI, "-s", os.path.join(GOLD, "small_reads.fasta"), "--realign", "--gfa", str(tmp_path / "g.gfa"), "--gfa-clean"] + flag,
                           capture_output=True, timeout=60)
        assert p.returncode == 1 and p.stdout.count(b"\n") == 1 and b"--gfa-clean-rounds" in p.stdout and not (tmp_path / "g.gfa").exists()
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and all(f"\t{n}," in h.stdout for n in ("--gfa-clean", "--gfa-tip-reads", "--gfa-bubble-bases", "--gfa-clean-rounds"))
    t = subprocess.run([sys.executable, "-m", "mhap_amd.graph", "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert t.returncode == 0 and all(n in t.stdout for n in ("--clean", "--tip-reads", "--bubble-bases", "--clean-rounds"))
    t = subprocess.run([sys.executable, "-m", "mhap_amd.graph", "x", "y", "--clean", "--clean-rounds", "0"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert t.returncode == 2 and "--clean-rounds >= 1" in t.stderr
