"""The string graph on the GPU (mhap_graph_*, graph_kernels.hip) against its CPU restatement (tests/string_graph_ref.py): the class of
every record, the contained flag of every read, the whole arc table except the q labels, the counts and the GFA text, exactly; then
`mhap-hip --realign --gfa` against `python -m mhap_amd.graph` end to end.  The records are fabricated from reads placed on a line:
no bases and no alignment are needed.  Two tests take one session through every call of the stage (the unitigs, their spelling and
the cleaning are unitig_kernels.hip's, over the session of graph_session.hpp): twice over with more records in between, and on
tables of no, one and two reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import graph_clean_ref as cr  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import unitig_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")


def _params(p):
    return sg.Params(**p)


def _compare(gs, ref, recs_in_order):
    """Everything the session gives against the restatement `ref` (both finished): returns (arcs, counts, contained, gfa)."""
    arcs, counts = gs.arcs, gs.counts
    assert arcs.dtype == np.int32 and arcs.shape == (len(ref.rows), 7), (arcs.shape, len(ref.rows))
    assert gs.classes().tolist() == ref.classes
    contained = gs.contained()
    assert contained.tolist() == ref.contained
    got, want = sg.strip_q(arcs), sg.strip_q(ref.rows)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])
    assert counts == ref.counts
    assert gs.info() == (len(ref.ids), len(ref.classes), len(ref.rows))
    for r in arcs.tolist():          # q names a record, by arrival, that gives the arc
        x = recs_in_order[r[4]]
        assert tuple(r[:3]) in sg.classify(x, ref.by_id[int(x["from_id"])], ref.by_id[int(x["to_id"])], ref.p)[1], r
    text = gs.gfa()
    assert text == ref.gfa()
    return arcs, counts, contained, text


def _check(ids, lengths, adds, **p):
    """One session and one restatement given the same adds, finished once and compared."""
    ref = sg.Graph(ids, lengths, _params(p))
    with mhap_amd.GraphSession(ids, lengths, **p) as gs:
        for recs in adds:
            gs.add(recs)
            ref.add(recs)
        gs.finish()
        ref.finish()
        allrecs = np.concatenate([np.asarray(a, sg.RECORD_DTYPE) for a in adds]) if adds else np.zeros(0, sg.RECORD_DTYPE)
        return _compare(gs, ref, allrecs)


def _hangs(k, qs, q3, tl5, tl3, span_q, span_t, rc, score=0.9):
    """The record of test_graph_cpu.hangs between reads 2 k + 1 and 2 k + 2, and the two lengths."""
    alen, blen = qs + span_q + q3, tl5 + span_t + tl3
    ts, te = tl5, tl5 + span_t
    b1, b2 = (ts, te - 1) if not rc else (blen - te, blen - ts - 1)
    return sg.record(2 * k + 1, 2 * k + 2, qs, qs + span_q - 1, alen, b1, b2, blen, rc, score), [alen, blen]


# (qs, q3, tl5, tl3, span_q, span_t): every class, then every boundary of tests/test_graph_cpu.py, each on two reads of its own
SHAPES = [(1500, 0, 1500, 0, 5000, 5000), (10, 20, 300, 400, 3000, 3000), (300, 400, 10, 20, 3000, 3000), (700, 0, 0, 700, 1500, 1500),
          (4000, 0, 0, 2500, 3000, 3000), (0, 1200, 3500, 0, 3000, 3000), (4100, 30, 100, 2500, 3000, 2990),
          (100, 50, 100, 60, 3000, 3000), (100, 60, 100, 60, 3000, 3000), (100, 61, 100, 60, 3000, 3000), (99, 60, 100, 60, 3000, 3000),
          (101, 60, 100, 60, 3000, 3000), (100, 3000, 3000, 100, 800, 800), (100, 3000, 3000, 100, 799, 799),
          (1000, 5000, 5000, 0, 5000, 5000), (1001, 5000, 5000, 0, 5000, 5000), (5000, 1000, 0, 5000, 5000, 5000),
          (5000, 1001, 0, 5000, 5000, 5000), (0, 500, 500, 0, 2000, 2000), (0, 500, 500, 0, 1999, 2000), (0, 500, 500, 0, 2000, 1999),
          (0, 500, 500, 0, 1999, 1999), (60, 500, 500, 40, 1900, 1900), (60, 500, 500, 39, 1900, 1900)]


@pytest.mark.parametrize("p", [{}, {"int_frac_permille": 799}, {"max_hang": 1001}, {"min_ovlp": 1999}, {"min_identity": 0.85}],
                         ids=["defaults", "int_frac_799", "max_hang_1001", "min_ovlp_1999", "min_identity_0.85"])
def test_hand_made_and_boundary_records(p):
    recs, lengths = [], []
    for rc in (0, 1):
        for shape in SHAPES:
            r, ln = _hangs(len(recs), *shape, rc, score=0.84 if len(recs) % 5 == 0 else 0.85)
            recs.append(r)
            lengths += ln
    k = len(recs)
    r, ln = _hangs(k, 4000, 0, 0, 2500, 3000, 3000, 0, score=0.0)             # no alignment
    same = sg.record(2 * k + 3, 2 * k + 3, 0, 2999, 3000, 0, 2999, 3000, 0)   # a read against itself
    recs += [r, same]
    lengths += ln + [3000]
    arcs, counts, contained, _ = _check(list(range(1, len(lengths) + 1)), lengths, [np.concatenate(recs)], **p)
    assert counts["none"] >= 2 and all(counts[c] > 0 for c in sg.CLASS_NAMES)


@pytest.mark.parametrize("degree", [0, 1, 63, 64, 65, 130])
def test_hub_vertex(degree):
    """Out-degrees around the wave's width and beyond two of them: the kernels rank, search and mark by counting and binary search
    over a vertex's own arcs, so they have no capacity that a degree could exceed."""
    ids, lengths, recs = sg.hub(degree)
    arcs, counts, _, _ = _check(ids, lengths, [recs])
    assert int((arcs[:, 0] == 0).sum()) == degree and counts["dovetail"] == len(recs) == degree * (degree + 1) // 2


def test_long_list_under_a_short_one():
    """v of out-degree 2 whose second target w has more than 64 arcs: the lanes go over w's arcs more than once."""
    ids, lengths, recs = sg.hub(2, w_degree=70, step=100)
    arcs, _, _, _ = _check(ids, lengths, [recs])
    assert int((arcs[:, 0] == 0).sum()) == 2 and int((arcs[:, 0] == 4).sum()) >= 65
    # and with the whole of w's list inside `longest` and inside fuzz
    arcs, _, _, _ = _check(ids, lengths, [recs], fuzz=5000)
    assert int((arcs[:, 0] == 4).sum()) >= 65


@pytest.mark.parametrize("len2,reduced", [(3000, 1), (3001, 0)])
def test_reduction_boundary_of_pass_1(len2, reduced):
    """v -> w 3 000, v -> x 5 000, so longest = 6 000; w -> y 2 000 comes first in w's list (y is no target of v) and w -> x has
    len2: 3 000 + 3 000 = longest eliminates x, 3 000 + 3 001 does not, and pass 2 stops at w's second arc (len2 >= fuzz)."""
    recs = np.concatenate([sg.dove(1, 2, 3000), sg.dove(1, 3, 5000), sg.dove(2, 4, 2000), sg.dove(2, 3, len2)])
    arcs, counts, _, _ = _check([1, 2, 3, 4], [20000] * 4, [recs])
    row = arcs[(arcs[:, 0] == 0) & (arcs[:, 1] == 4)][0].tolist()
    assert row[2] == 5000 and row[5] == reduced and row[6] == 0      # (never final: its complement 5 -> 1 is reduced through 5 -> 3 -> 1)


@pytest.mark.parametrize("len2,reduced", [(999, 1), (1000, 0)])
def test_boundary_of_pass_2(len2, reduced):
    """v -> z 1 000, v -> w 3 000, v -> x 3 500 and z -> w 100: pass 1 eliminates w through z and then skips it.  Pass 2 takes w's
    first arc (w -> y 500, y no target of v) and then w -> x only while its length is below fuzz."""
    recs = np.concatenate([sg.dove(1, 2, 1000), sg.dove(2, 3, 100), sg.dove(1, 3, 3000), sg.dove(1, 4, 3500), sg.dove(3, 5, 500), sg.dove(3, 4, len2)])
    arcs, _, _, _ = _check([1, 2, 3, 4, 5], [20000] * 5, [recs])
    assert arcs[(arcs[:, 0] == 0) & (arcs[:, 1] == 4)][0].tolist()[5] == 1          # w
    assert arcs[(arcs[:, 0] == 0) & (arcs[:, 1] == 6)][0].tolist()[5] == reduced    # x


def test_ties_duplicates_and_two_lengths_of_one_pair():
    recs = np.concatenate([sg.dove(1, 3, 3000), sg.dove(1, 2, 3000), sg.dove(1, 4, 3000, rc=1),       # equal len: ordered by v
                           sg.dove(1, 2, 3000), sg.dove(1, 2, 3000),                                   # the same record again, twice
                           sg.dove(1, 5, 4100), sg.dove(1, 5, 4000), sg.dove(1, 5, 4000), sg.dove(1, 5, 4200),   # one pair, three lengths
                           sg.dove(5, 1, 15000)])                                                      # and 5 before 1: other arcs
    arcs, counts, _, _ = _check([1, 2, 3, 4, 5], [20000] * 5, [recs])
    assert arcs[arcs[:, 0] == 0][:, 1:3].tolist() == [[2, 3000], [4, 3000], [7, 3000], [8, 4000]]
    assert counts["dovetail"] == 10 and counts["arcs"] == 10


def test_contained_and_dovetailed_read_and_a_containment_chain():
    a, b, c, d, e = (0, 10000, 0), (4000, 14000, 1), (7000, 17000, 0), (4500, 9500, 1), (5000, 8000, 0)      # e in d in a
    reads = [a, b, c, d, e]
    pairs = [(1, 2), (2, 3), (1, 3), (4, 3), (1, 4), (4, 5), (2, 5), (5, 3)]      # d dovetails c and lies in a; e lies in d, b and is short of c
    recs = np.concatenate([sg.placed(x, y, reads[x - 1], reads[y - 1]) for x, y in pairs])
    arcs, counts, contained, text = _check([1, 2, 3, 4, 5], [e1 - s for s, e1, _ in reads], [recs])
    assert contained.tolist() == [0, 0, 0, 1, 1] and counts["dovetail"] == 4 and counts["arcs"] == 6
    assert "S\t4\t" not in text and "S\t5\t" not in text and text.count("\nS\t") == 3


@pytest.fixture(scope="module", params=[2, 3, 5])
def layout(request):
    ids, lengths, reads, recs = sg.layout(request.param, jitter=300)
    ref = sg.Graph(ids, lengths)
    ref.add(recs)
    ref.finish()
    return ids, lengths, recs, ref


def test_random_layout_in_one_add_three_adds_and_shuffled(layout):
    ids, lengths, recs, ref = layout
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(recs)
        gs.finish()
        one = _compare(gs, ref, recs)
    ref3 = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths) as gs:
        for part in (recs[:100], recs[100:101], recs[101:]):
            gs.add(part)
            ref3.add(part)
        gs.finish()
        ref3.finish()
        three = _compare(gs, ref3, recs)
    perm = np.random.default_rng(11).permutation(len(recs))
    refs = sg.Graph(ids, lengths)
    refs.add(recs[perm])
    refs.finish()
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(recs[perm])
        gs.finish()
        shuffled = _compare(gs, refs, recs[perm])
        assert gs.classes()[np.argsort(perm)].tolist() == ref.classes      # the per-record output is permuted with the records
    for other in (three, shuffled):
        assert sg.strip_q(other[0]) == sg.strip_q(one[0]) and other[1] == one[1] and other[2].tolist() == one[2].tolist() and other[3] == one[3]
    assert one[1]["final"] > 100 and one[1]["reduced"] > 100 and one[1]["contained_reads"] > 50


def test_empty_adds_reads_without_records_finish_twice_and_add_after_finish(layout):
    ids, lengths, recs, _ = layout
    more_ids, more_lengths = ids + [1000, 1001], lengths + [5000, 0]           # two reads no record names, one of them empty
    ref = sg.Graph(more_ids, more_lengths)
    with mhap_amd.GraphSession(more_ids, more_lengths) as gs:
        assert gs.info() == (len(more_ids), 0, -1)
        gs.add(recs[:0])
        gs.finish()
        ref.finish()
        first = _compare(gs, ref, recs[:0])
        assert first[1]["arcs"] == 0 and first[3].count("\n") == 1 + len(more_ids)
        gs.add(recs[:300])
        gs.add(np.zeros(0, sg.RECORD_DTYPE))
        ref.add(recs[:300])
        gs.finish()
        ref.finish()
        a = _compare(gs, ref, recs)
        gs.finish()                                                             # again: the same table
        b = _compare(gs, ref, recs)
        assert a[0].tolist() == b[0].tolist() and a[1] == b[1]
        gs.add(recs[300:])                                                      # more records after a finish
        ref.add(recs[300:])
        gs.finish()
        ref.finish()
        _compare(gs, ref, recs)
    with mhap_amd.GraphSession([], []) as gs:                                   # no reads at all
        arcs, counts = gs.finish()
        assert len(arcs) == 0 and counts["records"] == 0 and gs.gfa() == "H\tVN:Z:1.0\n"
    arcs, counts, contained, text = mhap_amd.string_graph(recs, mhap_amd.FastaData(np.zeros(0, np.uint8), np.zeros(len(ids), np.int64), lengths, ids))
    assert sg.strip_q(arcs) == sg.strip_q(layout[3].rows) and text == layout[3].gfa()


def test_invalid_records_are_refused_with_their_index(layout):
    ids, lengths, recs, _ = layout
    ref = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(recs[:200])
        ref.add(recs[:200])
        gs.finish()
        ref.finish()
        before = _compare(gs, ref, recs)
        bad = recs[200:210].copy()
        bad[7]["to_id"] = 99999
        with pytest.raises(mhap_amd.MhapError, match="record 7 names read 99999"):
            gs.add(bad)
        bad = recs[200:210].copy()
        bad[3]["alen"] += 1
        with pytest.raises(mhap_amd.MhapError, match="record 3 gives read"):
            gs.add(bad)
        bad = recs[200:210].copy()
        bad[9]["blen"] -= 1
        with pytest.raises(mhap_amd.MhapError, match="record 9 gives read"):
            gs.add(bad)
        gs.finish()                                                             # a refused call has added nothing
        after = _compare(gs, ref, recs)
        assert after[0].tolist() == before[0].tolist() and after[1] == before[1] and gs.info()[1] == 200
        gs.add(recs[200:210])
        assert gs.info()[1] == 210
    with pytest.raises(mhap_amd.MhapError, match="int_frac_permille"):
        mhap_amd.GraphSession(ids, lengths, int_frac_permille=1001)


# ---- read tables past the scan's tile of 1 024 vertices --------------------------------------------------------------------------------

def _padded(pad, ids, lengths, recs):
    """`pad` reads that no record names (ids 1 .. pad, unequal lengths) in front of the given reads, whose ids move up by pad."""
    recs = recs.copy()
    recs["from_id"] += pad
    recs["to_id"] += pad
    return list(range(1, pad + 1)) + [i + pad for i in ids], [1000 + 7 * k for k in range(pad)] + list(lengths), recs


@pytest.mark.parametrize("pad,degree,edge", [(509, 3, 1024), (510, 3, 1024), (511, 3, 1024), (512, 3, 1024), (1023, 3, 2048), (1024, 3, 2048),
                                             (480, 65, 1024)])
def test_hub_across_the_edge_of_a_scan_tile(pad, degree, edge):
    """scan_kernel makes start and fstart 1 024 vertices at a time: `carry` takes the sum from tile to tile, a barrier keeps wave_sum
    of the tile before from being overwritten while it is read, and start[nv] = carry closes the last segment.  No other test has
    more than 410 vertices.  Here the vertices of a hub (read `pad` and the reads after it) lie on both sides of vertex 1 024 or
    2 048, or begin on it; with degree 65 segments of more than a wave's width lie on both sides.  scatter, dedup, place, reduce and
    find_arc all find a vertex's arcs through these sums."""
    ids, lengths, recs = _padded(pad, *sg.hub(degree))
    assert 2 * len(ids) > edge and 2 * pad <= edge < 2 * len(ids)                                      # the precondition
    arcs, counts, _, _ = _check(ids, lengths, [recs])
    assert int((arcs[:, 0] == 2 * pad).sum()) == degree and counts["dovetail"] == degree * (degree + 1) // 2
    assert (arcs[:, 0] >= edge).any() and (arcs[:, 0] < edge).any() == (2 * pad < edge)                # kept arcs at or above the edge
    assert counts["final"] > 0 and counts["reduced"] == (degree - 1) * degree


@pytest.fixture(scope="module", params=[2, 3])
def big_layout(request):
    ids, lengths, reads, recs = sg.layout(request.param, n_reads=1100, genome=880000, jitter=300)
    ref = sg.Graph(ids, lengths)
    ref.add(recs)
    ref.finish()
    return ids, lengths, recs, ref


def test_layout_of_1100_reads_in_one_add_and_shuffled_over_three(big_layout):
    """2 200 vertices: three tiles of the scan, the last one partial, with arcs in all of them, so that the carry into the second and
    into the third tile is not 0 and start[nv] is the sum of all three."""
    ids, lengths, recs, ref = big_layout
    rows = np.asarray(ref.rows, np.int64)
    assert 2 * len(ids) > 2048 and len(recs) > 5000
    for lo, hi in ((0, 1024), (1024, 2048), (2048, 2200)):                                             # the precondition
        tile = rows[(rows[:, 0] >= lo) & (rows[:, 0] < hi)]
        assert tile[:, 6].any() and tile[:, 5].any(), (lo, len(tile))
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(recs)
        gs.finish()
        one = _compare(gs, ref, recs)
    perm = np.random.default_rng(12).permutation(len(recs))
    parts = [perm[:len(perm) // 3], perm[len(perm) // 3:len(perm) // 3 + 1], perm[len(perm) // 3 + 1:]]
    refs = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths) as gs:
        for part in parts:
            gs.add(recs[part])
            refs.add(recs[part])
        gs.finish()
        refs.finish()
        shuffled = _compare(gs, refs, recs[perm])
    assert sg.strip_q(shuffled[0]) == sg.strip_q(one[0]) and shuffled[1] == one[1] and shuffled[2].tolist() == one[2].tolist() and shuffled[3] == one[3]
    high = one[0][one[0][:, 0] >= 2048]
    assert high[:, 6].any() and high[:, 5].any()


@pytest.mark.parametrize("n_reads", [511, 512, 513])
def test_read_counts_at_the_edge_of_a_scan_tile(n_reads):
    """nv = 1 022, 1 024 and 1 026: the last tile is almost full, full, and two vertices long, and start[nv] is written after one tile
    and after two.  The arcs are those of a hub of degree 2 on the last three reads; finished twice."""
    ids, lengths, recs = _padded(n_reads - 3, *sg.hub(2))
    assert len(ids) == n_reads
    ref = sg.Graph(ids, lengths)
    ref.add(recs)
    ref.finish()
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(recs)
        gs.finish()
        a = _compare(gs, ref, recs)
        gs.finish()
        b = _compare(gs, ref, recs)
    assert a[0].tolist() == b[0].tolist() and a[1] == b[1] and a[3] == b[3]
    assert a[1]["arcs"] == 6 and int(a[0][:, 0].max()) == 2 * n_reads - 1


# ---- the whole session: every group of buffers made, grown, reset and released ---------------------------------------------------------

UNITIG_TABLES = ("unitig_start", "unitig_len", "circular", "vertex", "offset", "span", "links")


def _same_unitigs(got, exp):
    for k in UNITIG_TABLES:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (k, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), k
    assert got["counts"] == exp["counts"]


def _spelled(gs, u, bases, offsets):
    out = np.full(u["counts"]["total_bases"], 1, np.uint8)      # (1: a byte no read holds)
    return gs.spell_into(bases, offsets, out).tobytes()


def _life(gs, ref, recs_in_order, bases, offsets):
    """finish, unitigs, spell, clean and spell on the session and on the restatement alike, every table and count vector compared
    (string_graph_ref, unitig_ref, graph_clean_ref); returns all of it as a list."""
    gs.finish()
    ref.finish()
    arcs, counts, contained, _ = _compare(gs, ref, recs_in_order)
    want_u = ur.of_graph(ref)
    u = gs.unitigs()
    _same_unitigs(u, want_u.tables())
    seq = _spelled(gs, u, bases, offsets)
    assert seq == b"".join(want_u.sequences(bases, offsets, ref.lengths))
    want = cr.Cleaned(ref)
    ccounts = gs.clean()
    assert ccounts == want.counts
    dropped, removed = gs.dropped(), gs.removed()
    assert dropped.tolist() == want.dropped and removed.tolist() == want.removed
    c = gs.cleaned_unitigs()
    _same_unitigs(c, want.unitigs.tables())
    assert gs.unitigs_info() == (len(c["unitig_len"]), len(c["vertex"]), len(c["links"]), c["counts"]["total_bases"])
    cseq = _spelled(gs, c, bases, offsets)
    assert cseq == b"".join(want.unitigs.sequences(bases, offsets, ref.lengths))
    return [arcs, counts, gs.classes(), contained, u, seq, ccounts, dropped, removed, c, cseq]


def _same_life(a, b):
    for x, y in zip(a, b):
        if isinstance(x, dict) and "vertex" in x:
            _same_unitigs(x, y)
        elif isinstance(x, np.ndarray):
            assert x.shape == y.shape and (sg.strip_q(x) == sg.strip_q(y) if x.ndim == 2 else np.array_equal(x, y))
        else:
            assert x == y


def _placed_anew(ids, lengths, seed, genome, share=2500):
    """The same reads placed on another line, and of that placement's records (sg.placed, at least `share` positions shared) the
    dovetails only: arcs that contradict the first layout, so forks, links and unitigs, and no new contained read."""
    rng = np.random.default_rng(seed)
    reads = []
    for ln in lengths:
        s = int(rng.integers(0, genome - ln + 1))
        reads.append((s, s + ln, int(rng.integers(0, 2))))
    recs = np.concatenate([sg.placed(ids[i], ids[j], reads[i], reads[j]) for i in range(len(ids)) for j in range(i + 1, len(ids))
                           if min(reads[i][1], reads[j][1]) - max(reads[i][0], reads[j][0]) >= share])
    g = sg.Graph(ids, lengths)
    g.add(recs)
    return recs[np.array(g.classes) == sg.DOVETAIL]


def test_one_session_two_lives():
    """finish -> unitigs -> clean -> spell, more records, the refusals that must hold until the next finish, and the sequence again:
    the second life's tables are those of a fresh session given both batches at once, and of the restatement.  40 reads; the first
    batch is their layout and a few contradicting dovetails (259 records: 122 arcs; served after the clean 10 unitigs, 17 members, 26
    links, six reads dropped), the second 86 more dovetails (198 arcs; 20 unitigs, 22 members, 72 links, one other read dropped), so
    the arc list, the link table, the removed bytes and the spelled bases outgrow the first life's buffers and the dropped bytes
    must start from zero again.  (The uncleaned member count cannot rise over one read table: every read that is not contained is
    a member of one unitig and an add only contains more reads.  It is the served, cleaned count that rises, 17 to 22.)"""
    ids, lengths, reads, recs = sg.layout(5, n_reads=40, genome=40000, jitter=300)
    _, bases, offsets = ur.plant(reads, 5, 40000)
    first = np.concatenate([recs, _placed_anew(ids, lengths, 202, 160000)])
    second = _placed_anew(ids, lengths, 300, 60000)
    both = np.concatenate([first, second])
    ref = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(first)
        ref.add(first)
        one = _life(gs, ref, first, bases, offsets)
        assert 200 < len(first) < 400 and one[7].any()
        gs.add(second)
        ref.add(second)
        for call in (gs.unitigs, gs.clean):
            with pytest.raises(mhap_amd.MhapError, match="records were added after the last mhap_graph_finish"):
                call()
        gs.finish()
        assert gs.unitigs_info()[0] == -1
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_unitigs: no mhap_graph_unitigs has completed since the last mhap_graph_finish"):
            gs._ms._chk(gs._lib.mhap_graph_copy_unitigs(gs._s, None, None, None))
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_layout: no mhap_graph_unitigs has completed"):
            gs._ms._chk(gs._lib.mhap_graph_copy_layout(gs._s, None, None, None))
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_links: no mhap_graph_unitigs has completed"):
            gs._ms._chk(gs._lib.mhap_graph_copy_links(gs._s, None))
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_spell: no mhap_graph_unitigs has completed"):
            gs.spell_into(bases, offsets, np.zeros(10, np.uint8))
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_dropped: no mhap_graph_clean has completed since the last mhap_graph_finish"):
            gs.dropped()
        gs.unitigs()
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_dropped: no mhap_graph_clean has completed"):
            gs.dropped()
        two = _life(gs, ref, both, bases, offsets)
    for k, name in ((0, None), (4, "unitig_len"), (4, "links"), (9, "unitig_len"), (9, "vertex"), (9, "links"), (8, None)):
        a, b = (one[k], two[k]) if name is None else (one[k][name], two[k][name])
        assert len(b) > len(a), (k, name, len(a), len(b))                           # every one of them had to grow
    assert len(two[10]) > len(one[10]) and two[7].tolist() != one[7].tolist()
    fresh_ref = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths) as gs:
        gs.add(both)
        fresh_ref.add(both)
        _same_life(two, _life(gs, fresh_ref, both, bases, offsets))


@pytest.mark.parametrize("n_reads", [0, 1, 2])
def test_empty_and_degenerate_sessions(n_reads):
    """No read; one read and no record; two reads whose only record is a containment: no arc, the contained read on no unitig, the
    other a unitig of one read without links.  Every call of the session, twice closed."""
    ids, lengths = list(range(1, n_reads + 1)), [10000, 4000][:n_reads]
    recs = sg.placed(1, 2, (0, 10000, 0), (3000, 7000, 1)) if n_reads == 2 else np.zeros(0, sg.RECORD_DTYPE)
    bases, offsets = ur.random_bases(lengths, 9)
    ref = sg.Graph(ids, lengths)
    gs = mhap_amd.GraphSession(ids, lengths)
    gs.add(recs)
    ref.add(recs)
    life = _life(gs, ref, recs, bases, offsets)
    arcs, counts, classes, contained, u, seq, ccounts, dropped, removed, c, cseq = life
    assert len(arcs) == 0 and counts["arcs"] == 0 and classes.tolist() == [sg.B_CONTAINED][:len(recs)] and contained.tolist() == [0, 1][:n_reads]
    assert gs.info() == (n_reads, len(recs), 0)
    assert u["unitig_start"].tolist() == [0, 1][:min(n_reads, 1) + 1] and u["unitig_len"].tolist() == [10000][:n_reads] and len(u["links"]) == 0
    assert u["vertex"].tolist() == [0][:n_reads] and seq == bytes(bases[:10000 * min(n_reads, 1)])
    _same_unitigs(c, u)
    assert cseq == seq and ccounts["rounds"] == 1 and not dropped.any() and len(removed) == 0
    assert gs.gfa() == ref.gfa() and gs.gfa(cleaned=True) == ref.gfa()
    gs._ms._chk(gs._lib.mhap_graph_copy_arcs(gs._s, None))                          # nothing to copy: no pointer is looked at
    gs._ms._chk(gs._lib.mhap_graph_copy_links(gs._s, None))
    gs._ms._chk(gs._lib.mhap_graph_copy_removed(gs._s, None))
    _same_life(life, _life(gs, ref, recs, bases, offsets))                          # and the whole sequence again
    gs.close()
    gs.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


def test_driver_and_tool_write_the_same_gfa(tmp_path):
    """40 synthetic reads of 3 000 bases at 8 x coverage and 10 % error, the graph's lengths scaled to them."""
    fa = mhap_amd.synth_reads(40, 3000, seed=77, coverage=8.0, error_rate=0.10)
    fasta = str(tmp_path / "reads.fasta")
    with open(fasta, "w") as fh:
        for i in range(len(fa)):
            fh.write(f">read{i}\n{fa.sequence(i)}\n")
    scaled = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]
    plain = _cli(["-s", fasta])
    base = _cli(["-s", fasta, "--realign"])
    out1, out2 = tmp_path / "one.gfa", tmp_path / "two.gfa"
    g1 = _cli(["-s", fasta, "--realign", "--gfa", str(out1)] + scaled)
    g2 = _cli(["-s", fasta, "--realign", "--gfa", str(out2), "--realign-paf"] + scaled)
    assert plain.returncode == 0 and base.returncode == 0 and g1.returncode == 0 and g2.returncode == 0, g1.stderr[-2000:]
    # stdout is what it is without --gfa (the driver's record order differs from run to run: compared sorted, as everywhere)
    assert sorted(g1.stdout.split(b"\n")) == sorted(base.stdout.split(b"\n")) and len(g1.stdout) == len(base.stdout) > 1000
    assert b"gfa" not in base.stderr and b"--gfa-fuzz = 300" in g1.stderr
    text = out1.read_text()
    assert out2.read_text() == text                                             # two runs, two record orders, one file
    lines = text.split("\n")
    n_s, n_l = sum(l.startswith("S\t") for l in lines), sum(l.startswith("L\t") for l in lines)
    print(f"{n_s} S lines, {n_l} L lines")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == "" and 0 < n_s <= 40 and n_l > 0 and n_l % 2 == 0
    totals = [l for l in g1.stderr.decode().split("\n") if l.startswith("String graph of ")]
    assert len(totals) == 1 and totals[0].endswith(f"{n_l} final")
    # the stand-alone tool on the driver's own plain output
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tool_out = tmp_path / "tool.gfa"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.graph", str(tmp_path / "ovl.txt"), fasta, "--max-hang", "300", "--min-overlap", "1000",
                        "--fuzz", "300", "-o", str(tool_out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tool_out.read_text() == text
    assert totals[0] in p.stderr
