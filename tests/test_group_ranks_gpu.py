"""The multi-rank driver (mhap_dist.hip: mhap_group_*, mhap_dist_*, the rendezvous protocol, the eager exchange) on ONE GPU: N ranks
share device 0 through the in-process peer transport.  What the other group tests leave out: the eager exchange together with the
streamed ingest (the `dist_ingest_scope` rendezvous, by which ranks whose ingest plans differ stay in step), the eager state against
the other calls, the edges of -q over ranks, and k-mer sizes off the (16, 12) fast path with ranks and with -q.  Every expectation is
the oracle's (group_rank_cases.py), compared as sorted record lines; every case asserts a witness of the branch it means to take
(`dist_eager_searches`, the intended ingest group counts, a record-count floor that the oracle alone satisfies).

The rendezvous each case makes, per rank and in order.  A rendezvous is a host barrier of all ranks without a time-out, and ranks that
meet in different kinds fail with "out of step", so every rank of a case must make the same sequence.  I = RV_INGEST (the ingest plan,
`dist_ingest_scope`), A = RV_ADD and AA = RV_ADD_ALLOC (`dist_eager_begin`; AA follows only when every rank said it can), S = RV_SEARCH and
SA = RV_SEARCH_ALLOC (`exchange_and_search`; SA and the four gathers follow only on the fall-back branch and when some rank has a row).

 1a  one ingest group on every rank        add_scan: I(1) A AA + 4 gathers | search: S | search: S                     (all ranks alike)
 1b  rank 0 two groups, rank 1 one         add_scan: I(2 | 1), then no add makes a rendezvous | search: S SA | clear, add_data: A AA |
                                           search: S
 1c  2 (1) records on 3 ranks              add_scan: I(1 | 1 | 0) (I(1 | 0 | 0)): the empty ranks announce 0 groups, nobody adds eagerly |
                                           search: S SA | clear, full add_scan: I(1) A AA | search: S
                                           (before the fix the empty ranks made A where the others made I: every rank left with MHAP_E_STATE)
 1d  a second add_scan                     add_scan 1: I(1) A AA | search: S | add_scan 2: I(1) A (every rank says "not the first add":
                                           no AA) | search: S SA
 1e  rank 1's share is unsketchable        add_scan: I(1) A AA + 4 gathers (its rows travel with status 2) | search: S
 1f  one RCCL rank                         add_scan: I(1) A AA | search: S | clear, add_scan in two groups: I(2) | search: S SA
 2a  -q between two self searches          add_data: A AA | search: S | -q: S SA | search: S SA
 2b  rank 1's shard replaced               add_data: A AA | search: S | (rank 1: export, clear, add_sketches: no rendezvous) | search: S SA
 3   -q edges                              add_data with the eager exchange off: none | every search: S, and SA unless no rank has a row
 4   other k-mer sizes                     as 3; the eager case: add_data: A AA | search: S
"""
import numpy as np
import pytest

import group_rank_cases as K
import mhap_amd
from mhap_amd import FastaScan, MinHashSearch, MinHashSearchGroup

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _plain_environment(monkeypatch):
    for name in ("MHAP_INGEST_GROUP_BASES", "MHAP_GROUP_FORCE_PEER", "MHAP_BATCH_BASES", "MHAP_GROUP_TRANSPORT"):
        monkeypatch.delenv(name, raising=False)


def _group(n, p=None, eager=False):
    g = MinHashSearchGroup(p or K.params(), n=n, devices=[0] * n)
    if eager:
        for r in range(n):
            g.rank(r).dist_set_eager(True)
    return g


def _eager_searches(g):
    return [g.rank(r).dist_eager_searches() for r in range(g.n)]


# ---- 1. eager exchange x streamed ingest ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_eager_add_scan_of_one_group_per_rank(tmp_path, n):
    """1a: every rank's share is one ingest group, so the ingest rendezvous keeps the eager exchange on: the add gathers, the search finds
    the rows in place (0 -> 1), and so does a second search (-> 2)."""
    index, _, want = K.main_set()
    assert len(want["lines"]) > 1000
    for r in range(n):
        assert len(K.ingest_groups(index.lengths[r::n])) == 1
    path = K.write_fasta(tmp_path / "reads.fasta", K.sequences(index), width=80)
    with FastaScan(path) as sc, _group(n, eager=True) as g:
        assert _eager_searches(g) == [0] * n
        g.add_scan(sc)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1] * n
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [2] * n


def test_eager_add_scan_with_different_group_counts(tmp_path, monkeypatch):
    """1b: rank 0's share (1.2 Mbase) splits into two ingest groups, rank 1's (0.3 Mbase) is one: the ranks learn it in the ingest
    rendezvous and suspend the eager exchange together, the search gathers by itself (eager_searches stays 0), and the flag is back
    afterwards: one add_data of one launch group into the cleared group gathers eagerly (-> 1)."""
    fa, seqs, want = K.long_short_set()
    assert len(want["lines"]) > 1000
    monkeypatch.setenv("MHAP_INGEST_GROUP_BASES", str(1 << 20))
    shares = [fa.lengths[0::2], fa.lengths[1::2]]
    assert int(shares[0].sum()) > K.FIRST_GROUP_FLOOR > int(shares[1].sum())
    assert [len(K.ingest_groups(s, 1 << 20)) for s in shares] == [2, 1]
    path = K.write_fasta(tmp_path / "long_short.fasta", seqs)
    with FastaScan(path) as sc, _group(2, eager=True) as g:
        assert sc.info()[1].tolist() == fa.lengths.tolist()
        g.add_scan(sc)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [0, 0]
        g.clear()
        g.add_data(fa)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1]


@pytest.mark.parametrize("records,force_peer", [(2, "0"), (2, "1"), (1, "0")])
def test_eager_add_scan_of_fewer_records_than_ranks(tmp_path, monkeypatch, records, force_peer):
    """1c: three ranks, two records or one: the ranks without a record take part in the ingest rendezvous their peers make (they used to
    make the add's, and every rank failed with "the ranks' collective calls are out of step").  The add succeeds and nobody gathers
    eagerly; the same group then takes the whole file after a clear, eagerly, and searches correctly."""
    monkeypatch.setenv("MHAP_GROUP_FORCE_PEER", force_peer)
    index, _, want = K.main_set()
    pair, want_pair = K.overlapping_pair()
    assert len(want_pair["lines"]) >= 1
    few = K.write_fasta(tmp_path / "few.fasta", K.sequences(pair)[:records])
    full = K.write_fasta(tmp_path / "full.fasta", K.sequences(index))
    with FastaScan(few) as sc_few, FastaScan(full) as sc_full, _group(3, eager=True) as g:
        assert len(sc_few) == records < g.n
        g.add_scan(sc_few)
        assert sum(g.rank(r).size() for r in range(3)) == 2 * records
        assert K.lines(g.find_matches()) == (want_pair["lines"] if records == 2 else [])
        assert _eager_searches(g) == [0, 0, 0]
        g.clear()
        g.add_scan(sc_full)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]


def test_second_add_scan_onto_a_group_that_holds_reads(tmp_path):
    """1d: two files, the second scanned with the first one's record count as id offset; 200 records are no multiple of three, so the deal of
    the second file starts at rank 2 (the phase `first` of mhap_group_add_scan).  The first add is eager, the second is not (only the
    add that fills an empty index can gather): the search after it gathers by itself and eager_searches stays where it was."""
    index, _, want = K.main_set()
    seqs, n1 = K.sequences(index), 200
    assert n1 % 3 != 0 and len(K.lines_among(want, n1)) > 200
    one = K.write_fasta(tmp_path / "one.fasta", seqs[:n1])
    two = K.write_fasta(tmp_path / "two.fasta", seqs[n1:], width=70)
    with FastaScan(one) as sc1, FastaScan(two, id_offset=n1) as sc2, _group(3, eager=True) as g:
        assert sc2.info()[0].tolist() == list(range(n1 + 1, len(index) + 1))
        g.add_scan(sc1)
        assert K.lines(g.find_matches()) == K.lines_among(want, n1)
        assert _eager_searches(g) == [1, 1, 1]
        g.add_scan(sc2)
        # the deal went on where the first file ended: rank r holds the reads whose ordinal in the data set is congruent to r
        for r in range(3):
            assert sorted(set(g.rank(r).export()["ids"].tolist())) == list(range(r + 1, len(index) + 1, 3))
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]


def test_eager_add_scan_with_a_rank_whose_share_is_unsketchable(tmp_path):
    """1e: every record of rank 1 is below --min-olap-length or shorter than k.  Its add is still one ingest group and one launch group, so
    the add is eager on both ranks and its rows travel with their status; no record is made or lost."""
    fa, seqs, want = K.unsketchable_share_set()
    assert max(len(s) for s in seqs[1::2]) < K.MIN_OLAP and min(len(s) for s in seqs[1::2]) < 16
    assert want["sketchable"] == len(seqs) // 2 and len(want["lines"]) > 500
    path = K.write_fasta(tmp_path / "unsketchable.fasta", seqs)
    with FastaScan(path) as sc, _group(2, eager=True) as g:
        g.add_scan(sc)
        assert g.rank(1).size() == len(seqs) and g.rank(1).stats()["strands_indexed"] == 0
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1]
        assert g.stats()["queries_searched"] == want["sketchable"]


def test_one_rccl_rank_add_scan_eager_and_suspended(tmp_path, monkeypatch):
    """1f: the same rendezvous over RCCL with a world of one rank (all one GPU can form): a scan of one ingest group adds eagerly, the
    same scan in two groups suspends the exchange."""
    index, _, want = K.main_set()
    lengths = index.lengths.tolist()
    assert len(K.ingest_groups(lengths)) == 1 and len(K.ingest_groups(lengths, 1 << 20)) == 2
    path = K.write_fasta(tmp_path / "reads.fasta", K.sequences(index))
    with FastaScan(path) as sc, MinHashSearch(K.params()) as ms:
        ms.dist_init(0, 1, MinHashSearch.dist_unique_id())
        ms.dist_set_eager(True)
        ms.add_scan(sc)
        assert K.lines(ms.dist_find_matches()) == want["lines"] and ms.dist_eager_searches() == 1
        ms.clear()
        monkeypatch.setenv("MHAP_INGEST_GROUP_BASES", str(1 << 20))
        ms.add_scan(sc)
        assert ms.size() == 2 * len(index)
        assert K.lines(ms.dist_find_matches()) == want["lines"] and ms.dist_eager_searches() == 1


# ---- 2. eager state against the other calls ---------------------------------------------------------------------------------------------
def test_query_search_between_two_self_searches_drops_the_eager_rows():
    """2a: a -q search overwrites the gather buffers the eager add filled, so it must clear `eager_valid`: the self search after it gathers
    again (eager_searches stays 1) and still equals the oracle's records."""
    index, queries, want = K.main_set()
    want_q = K.main_query_lines()
    assert len(want_q) > 500
    with _group(3, eager=True) as g:
        g.add_data(index)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]
        assert K.lines(g.find_matches_stream(queries)) == want_q
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]


def test_replaced_shard_makes_every_rank_fall_back():
    """2b: rank 1's shard is exported, cleared and added again as sketches: the same content under another index generation.  Only rank 1
    knows; the search's rendezvous tells the others, and all of them gather again."""
    index, _, want = K.main_set()
    with _group(3, eager=True) as g:
        g.add_data(index)
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]
        r1 = g.rank(1)
        tables = r1.export()
        assert (tables["status"] == 0).all()
        r1.clear()
        r1.add_sketches({k: v for k, v in tables.items() if k != "status"})
        assert K.lines(g.find_matches()) == want["lines"]
        assert _eager_searches(g) == [1, 1, 1]


# ---- 3. -q edges of the group -----------------------------------------------------------------------------------------------------------
def _from_id(line):
    return int(line.split()[0])


@pytest.mark.parametrize("n", [3, 4])
def test_query_edges_over_ranks(n):
    """0 queries (`total == 0`), one query and N - 1 queries (ranks that sketch nothing send padding rows only), and a set with a query
    shorter than k, one below --min-olap-length and an IUPAC read, against the brute force over the oracle's primitives."""
    index, _, _ = K.main_set()
    q, want_q = K.edge_queries()
    short = [int(q.ids[i]) for i in range(len(q)) if q.lengths[i] < K.MIN_OLAP]
    iupac = int(q.ids[-1])
    assert len(short) == 2 and len(q) % n != 0 and b"N" in q.bases.tobytes()
    assert not any(_from_id(ln) in short for ln in want_q) and sum(_from_id(ln) == iupac for ln in want_q) >= 10 and len(want_q) > 300
    with _group(n) as g:
        g.add_data(index)
        assert len(g.find_matches_stream(K.empty_reads())) == 0
        for count in (1, n - 1):
            sub = q.subset(np.arange(1, 1 + count))
            want_sub = [ln for ln in want_q if _from_id(ln) in sub.ids.tolist()]
            assert len(want_sub) >= 10 * count
            assert K.lines(g.find_matches_stream(sub)) == want_sub, count
        assert K.lines(g.find_matches_stream(q)) == want_q
        assert g.stats()["queries_searched"] == n + len(q) - len(short)      # sketched queries only, each counted once


@pytest.mark.parametrize("n", [3, 4])
def test_single_stored_read_and_a_group_never_added_to(n):
    """An index of one read leaves N - 1 shards empty: -q with queries that overlap it finds the oracle's records.  A group that has
    never been added to answers a self search and a -q search with no record and no error."""
    index, queries, _ = K.main_set()
    to_id = int(K.main_query_lines()[0].split()[1])
    stored = K.with_ids(index.subset(np.array([to_id - 1])), to_id)
    want_one = K.query_oracle(stored, queries)
    assert len(want_one) >= 1
    with _group(n) as g:
        assert len(g.find_matches()) == 0
        assert len(g.find_matches_stream(queries)) == 0
        assert len(g.find_matches_stream(K.empty_reads())) == 0
        g.add_data(stored)
        assert [g.rank(r).size() for r in range(n)] == [2] + [0] * (n - 1)
        assert K.lines(g.find_matches_stream(queries)) == want_one
        assert len(g.find_matches()) == 0


@pytest.mark.parametrize("n", [3, 4])
def test_group_statistics_on_a_ragged_data_set(n):
    """mhap_group_get_stats after one self search of a data set whose read count is no multiple of N and that holds unsketchable reads:
    every rank probes every sketched query and no padding row, so the sum over the ranks divided by N is exactly the number of
    sketchable reads; the compared candidates and the index elements walked add up to the single index's, which are the oracle's."""
    fa, want = K.ragged_set()
    assert len(fa) % n != 0 and want["sketchable"] < len(fa) and len(want["lines"]) > 500
    with _group(n) as g:
        g.add_data(fa)
        assert K.lines(g.find_matches()) == want["lines"]
        st = g.stats()
        per_rank = [g.rank(r).stats()["queries_searched"] for r in range(n)]
    assert per_rank == [want["sketchable"]] * n
    assert st["queries_searched"] == want["sketchable"]
    assert st["strands_indexed"] == want["strands"] and st["matches_found"] == len(want["lines"])
    assert st["candidates_compared"] == want["compared"]
    assert st["table_elements"] == want["elements"]


# ---- 4. other k-mer sizes with ranks and with -q ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,k2", [(15, 12), (16, 13), (33, 20)])
def test_other_kmer_sizes_with_ranks_and_queries(k, k2):
    """(15, 12), (16, 13) and (33, 20) each miss a condition of the (16, 12) fast path: reads are hashed into materialised rows.  Self
    search on 2 and 3 ranks, -q on one handle and on 3 ranks, and (16, 13) once more with the eager add."""
    index, queries = K.kmer_set()
    want, want_q = K.kmer_oracles(k, k2)
    assert len(want["lines"]) >= 30 and len(want_q) >= 30
    p = K.params(k, k2)
    with MinHashSearch(p) as ms:
        ms.add_data(index)
        assert K.lines(ms.find_matches_stream(queries)) == want_q
    for n in (2, 3):
        with _group(n, p) as g:
            g.add_data(index)
            assert K.lines(g.find_matches()) == want["lines"], n
            if n == 3:
                assert K.lines(g.find_matches_stream(queries)) == want_q
    if (k, k2) == (16, 13):
        with _group(3, p, eager=True) as g:
            g.add_data(index)
            assert K.lines(g.find_matches()) == want["lines"]
            assert _eager_searches(g) == [1, 1, 1]
