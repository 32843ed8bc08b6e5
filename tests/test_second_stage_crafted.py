"""The second stage (join_kernels.hip: overlap_join_kernel, its two wider instantiations, the per-lane kernel) pair by pair on crafted sketches: every pair is
built to sit on one branch — a cap of the join, a sketch size, a hash value, a launch shape — and its record is compared with the
oracle's literal getOverlapInfo (tests/sketch_search_ref.py, pinned to orc_run_self by tests/test_sketch_search_ref.py).

Launch shapes by sketch size (overlap_join_lds_bytes at the defaults, 64 KB of LDS per workgroup; MHAP_OJ_FILTER_BPE changes the
shared shapes' filter): alone fits up to S = 7 456, pair up to 6 624, team up to 5 692; the 512-wide pass up to 6 304, the 1 536-wide
one up to 3 232.  So a pinned `team` falls back to `alone` at S = 6 144 and 7 168, a pinned `pair` at 7 168; at S = 4 096 and 6 144 the
pairs above 512 joined k-mers skip the 1 536-wide pass; at S = 8 192 no shape fits and every pair takes the per-lane kernel.  A larger
sketch (S > OJ_MAX_S) is refused when the handle is made.
"""
import numpy as np
import pytest

import mhap_amd
from mhap_amd import MhapParams, MinHashSearch
import oracle_lib as O
import sketch_search_ref as R

pytestmark = pytest.mark.gpu

K2 = 12
SWITCHES = ("MHAP_JOIN_MODE", "MHAP_OVERLAP", "MHAP_OVERLAP_PRUNE", "MHAP_OJ_FILTER_BPE", "MHAP_OVERLAP_BLOCKS", "MHAP_QUERY_CHUNK",
            "MHAP_JOIN_WIDE")
SETTINGS = [{}, {"MHAP_JOIN_MODE": "alone"}, {"MHAP_JOIN_MODE": "pair"}, {"MHAP_JOIN_MODE": "team"}, {"MHAP_OVERLAP": "lane"},
            {"MHAP_OVERLAP_PRUNE": "0"}, {"MHAP_OVERLAP_PRUNE": "1"}, {"MHAP_OJ_FILTER_BPE": "1"}, {"MHAP_OJ_FILTER_BPE": "64"},
            {"MHAP_OVERLAP_BLOCKS": "1"}, {"MHAP_QUERY_CHUNK": "128"}]
EXTREMES = (R.INT32_MIN, R.INT32_MAX, -1, 0)


def _params(S, H=16, threshold=0.0, num_min_matches=3):
    return dict(H=H, k2=K2, num_min_matches=num_min_matches, min_store_length=0, threshold=threshold, max_shift=0.2)


def _search(monkeypatch, env, S, kw, entries, queries=None):
    """One search with a fresh handle under `env` (some switches are read once per handle): records and stats."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = MhapParams(num_hashes=kw["H"], ordered_kmer_size=K2, ordered_sketch_size=S, num_min_matches=kw["num_min_matches"],
                   min_store_length=kw["min_store_length"], threshold=kw["threshold"], max_shift=kw["max_shift"], device=0)
    with MinHashSearch(p) as ms:
        ms.add_sketches(entries)
        recs = ms.find_matches() if queries is None else ms.find_matches_sketches(queries)
        st = ms.stats()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return sorted(mhap_amd.records_to_lines(recs)), st


def _diff(got, want):
    g, w = set(got), set(want)
    return f"{len(got)} records, {len(want)} expected; missing {sorted(w - g)[:4]}, extra {sorted(g - w)[:4]}"


def _check_all_settings(monkeypatch, c, S, kw, settings=SETTINGS):
    ent, qry = c.tables()
    for mode, q in (("self", None), ("-q", qry)):
        want, compared = R.expected_records(ent, q, return_compared=True, **kw)
        assert compared > 0
        for env in settings:
            got, st = _search(monkeypatch, env, S, kw, ent, q)
            assert st["candidates_compared"] == compared, (S, mode, env, st, compared)
            assert got == want, (S, mode, env, _diff(got, want))


# ---- the caps ---------------------------------------------------------------------------------------------------------------
def _caps_corpus(S=2048):
    c = R.Corpus(S, seed=2048)
    for cap in (128, 512, 1536):
        for nj in (cap - 1, cap, cap + 1):
            c.pair(f"joined {nj}", joined=nj, seqlen_a=3 * S, seqlen_b=3 * S + 7, spread=2 * S)
    for ng in (16, 17):                                           # OJ_GCAP: duplicated-hash groups per pair
        c.pair(f"{ng} groups", joined=20, groups=[(2, 1)] * ng, seqlen_a=4 * S, seqlen_b=4 * S)
    for g in ((8, 1), (1, 8), (8, 8), (9, 1), (1, 9), (9, 9)):    # OJ_GLEN: entries of one sketch in a group
        c.pair(f"group {g}", joined=30, groups=[g, (2, 2)], seqlen_a=4 * S, seqlen_b=4 * S)
    c.pair("ties", joined=40, ties=3, seqlen_a=4 * S, seqlen_b=4 * S)       # optimizeShifts' strict > (the first record stays)
    c.pair("ties + groups", joined=60, ties=2, groups=[(1, 2), (3, 2)], seqlen_a=4 * S, seqlen_b=4 * S, rev_b=True)
    for _ in range(4):
        c.loner(S, 2 * S)
    return c


@pytest.mark.timeout(300)
@pytest.mark.parametrize("wide", ["0", "1", "2"])
def test_join_caps_on_both_sides(monkeypatch, wide):
    """cap - 1 / cap / cap + 1 joined k-mers for the three passes (128, 512, 1 536), 16 / 17 groups, groups of 8 / 9 entries in the
    query, the other sketch and both, and tied records — records equal to the oracle's, and exactly the pairs above the last enabled
    pass's cap (or over a group cap) go to the per-lane kernel."""
    S = 2048
    c = _caps_corpus(S)
    kw = _params(S)
    ent, qry = c.tables()
    want, compared = R.expected_records(ent, return_compared=True, **kw)
    assert compared == len(c.pair_joined)
    got, st = _search(monkeypatch, {"MHAP_JOIN_WIDE": wide}, S, kw, ent)
    assert st["candidates_compared"] == compared
    assert got == want, _diff(got, want)
    assert st["slow_pairs"] == R.slow_pairs_model(c.pair_joined, int(wide), S), (wide, st)
    assert st["slow_pairs"] == {"0": 11, "1": 8, "2": 5}[wide]
    want_q, compared_q = R.expected_records(ent, qry, return_compared=True, **kw)
    got_q, st_q = _search(monkeypatch, {"MHAP_JOIN_WIDE": wide}, S, kw, ent, qry)
    assert st_q["candidates_compared"] == compared_q and got_q == want_q, _diff(got_q, want_q)


@pytest.mark.timeout(300)
def test_join_caps_under_every_switch(monkeypatch):
    S = 2048
    _check_all_settings(monkeypatch, _caps_corpus(S), S, _params(S))


# ---- sketch sizes and hash values ---------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 63, 64, 65, 1535, 1536, 1537, 2048, 4096, 6144, 7168, 8192]


def _partial(n):
    """A size below n that is no multiple of 64 (the last block of the row is partial)."""
    for d in (5, 6, 7, 9):
        if n - d >= 1 and (n - d) % 64:
            return n - d
    return max(1, n - 1)


def _sizes_corpus(S):
    c = R.Corpus(S, seed=S, reserved=EXTREMES)
    long_ = 3 * S + 101
    if S <= 3:
        c.pair("full rows", joined=S, seqlen_a=long_, seqlen_b=long_ + 1)
        c.pair("short reads", joined=S, seqlen_a=S, seqlen_b=S)
        c.pair("size 1 / full", joined=1, size_a=1, seqlen_a=1, seqlen_b=long_)
        if S >= 2:
            c.pair("size 2 / 2, extremes", joined=0, fixed=(R.INT32_MIN, R.INT32_MAX), size_a=2, size_b=2, seqlen_a=2, seqlen_b=2)
        if S == 3:
            c.pair("three extremes", joined=0, fixed=(R.INT32_MIN, -1, R.INT32_MAX), seqlen_a=long_, seqlen_b=long_, rev_b=True)
    else:
        j = max(3, S // 4)
        c.pair("full rows", joined=j, seqlen_a=long_, seqlen_b=long_ + 33, spread=2 * S)
        c.pair("full rows, three quarters joined", joined=(3 * S) // 4 - 2, seqlen_a=long_, seqlen_b=long_, spread=3 * S, shift=S // 8)
        pa, pb = _partial(S), _partial(_partial(S) - 3)
        c.pair("partial rows of other sizes", joined=max(3, min(pa, pb) // 2), size_a=pa, size_b=pb, shift=-(pb // 16))
        c.pair("partial / full", joined=max(3, pa // 3), size_a=pa, seqlen_b=long_, rev_b=True)
        c.pair("size 1 / full", joined=1, size_a=1, seqlen_a=1, seqlen_b=long_)
        c.pair("size 2 / size 2", joined=2, size_a=2, size_b=2, seqlen_a=2, seqlen_b=2)
        c.pair("extremes", joined=max(0, S // 8 - 4), fixed=EXTREMES, seqlen_a=long_, seqlen_b=long_)
        lo = int(c.rng.integers(-(1 << 30), 1 << 30))
        c.pair("narrow hash range", joined=max(1, S // 3), hash_range=(lo, lo + 3 * S + 64), seqlen_a=long_, seqlen_b=long_)
        c.pair("filter-saturating rows", joined=max(3, S // 16), filter_noise=S // 2, seqlen_a=long_, seqlen_b=long_)
        if S >= 63:
            c.pair("groups and ties", joined=S // 5, groups=[(2, 1), (1, 3), (2, 2)], ties=2, seqlen_a=long_, seqlen_b=long_ + 5,
                   rev_b=True)
        if S >= 1024:
            c.pair("computeEdges wraps", joined=1000, seqlen_a=3_000_000, seqlen_b=5_000_000, start_a=2_100_000, spread=900_000)
        c.loner(S, long_)
        c.loner(_partial(S), fwd=False)
    return c


@pytest.mark.timeout(420)
@pytest.mark.parametrize("S", SIZES)
def test_sketch_sizes_under_every_switch(monkeypatch, S):
    """Full and partial rows (size % 64 != 0), query and entry of different sizes, rows of 1 and 2 entries (EMPTY), INT32_MIN /
    INT32_MAX / -1 / 0, a hash range narrower than the bucket table, rows that saturate the query's filter, and (S >= 1 536) a
    pair of megabase reads whose edges wrap — under every switch, in self and in -q mode, at threshold 0 (EMPTY is a record)."""
    _check_all_settings(monkeypatch, _sizes_corpus(S), S, _params(S))


@pytest.mark.timeout(60)
def test_sketch_size_above_the_join_limit_is_refused():
    with pytest.raises(mhap_amd.MhapError, match="ordered-sketch-size"):
        MinHashSearch(MhapParams(num_hashes=16, ordered_sketch_size=8193, device=0))


@pytest.mark.timeout(300)
def test_compute_edges_wraps_like_java(monkeypatch):
    """Reads of 3 / 5 Mb and 64 / 40 Mb: valid records x window start >= 2^31, so Java's int products in computeEdges wrap.  The
    test computes the wrapped and the exact start and end itself, checks they differ, and that the records carry the wrapped ones."""
    S = 1536
    c = R.Corpus(S, seed=31)
    geo = [(3_000_000, 5_000_000, 2_100_000, 900_000, 1200), (64_000_000, 40_000_000, 30_000_000, 2_000_000, 1400),
           (1_500_000, 1_600_000, 1_400_000, 90_000, 1100)]
    for la, lb, start, spread, nj in geo:
        c.pair(f"wrap {la}", joined=nj, seqlen_a=la, seqlen_b=lb, start_a=start, spread=spread)
    ent, qry = c.tables()
    kw = _params(S)
    wrapped_any = 0
    for i in range(len(geo)):
        a, b = 2 * i, 2 * i + 1
        ha, pa = ent["ordered"][a, :, 0], ent["ordered"][a, :, 1]
        hb = set(ent["ordered"][b, :, 0].tolist())
        joined = np.array([p for h, p in zip(ha.tolist(), pa.tolist()) if h in hb])
        n, le, re = len(joined), int(joined.min()), int(joined.max())
        assert n == geo[i][4]
        (w1, w2), (e1, e2) = R.wrap_edges(n, le, re)
        r = O.overlap(ent["ordered"][a], int(ent["ordered_seqlen"][a]), ent["ordered"][b], int(ent["ordered_seqlen"][b]), K2, 0.2)
        assert (r["a1"], r["a2"]) == (max(w1, 0), min(w2, int(ent["ordered_seqlen"][a])))
        assert (r["b1"], r["b2"]) == (max(w1, 0), min(w2, int(ent["ordered_seqlen"][b])))   # (B positions = A positions)
        if (w1, w2) != (e1, e2):
            wrapped_any += 1
    assert wrapped_any >= 2
    want = R.expected_records(ent, **kw)
    for env in ({}, {"MHAP_JOIN_WIDE": "0"}, {"MHAP_OVERLAP": "lane"}, {"MHAP_OVERLAP_PRUNE": "1"}):
        got, st = _search(monkeypatch, env, S, kw, ent)
        assert st["candidates_compared"] == len(geo) and got == want, (env, _diff(got, want))
        got_q, _ = _search(monkeypatch, env, S, kw, ent, qry)
        assert got_q == R.expected_records(ent, qry, **kw), env


# ---- volume and the automatic shape choice --------------------------------------------------------------------------------------
@pytest.mark.timeout(420)
@pytest.mark.parametrize("per_query", ["one", "two-three", "many"])
def test_candidates_per_query_pick_each_shape(monkeypatch, per_query):
    """S = 1 536.  Self mode: pairs (0.5 candidates per query: alone), groups of six (2.5: pair), one group of 300 entries (149.5:
    team, 44 850 pairs — at least eight per pull of every resident wave).  -q mode: 1, 3 and 300 per query (every query meets
    itself)."""
    S = 1536
    c = R.Corpus(S, H=16, seed={"one": 1, "two-three": 2, "many": 3}[per_query])
    if per_query == "one":
        for i in range(120):
            c.pair(f"p{i}", joined=int(c.rng.integers(3, 400)), seqlen_a=2 * S, seqlen_b=2 * S + 3, shift=int(c.rng.integers(-50, 50)),
                   rev_b=bool(i % 3 == 0))
    elif per_query == "two-three":
        for i in range(40):
            c.group(f"g{i}", 6, S, seqlen=2 * S + 17)
    else:
        c.group("big", 300, S, seqlen=4 * S, shared=0.3)
    kw = _params(S, threshold=0.0 if per_query != "many" else 0.02)
    ent, qry = c.tables()
    for mode, q in (("self", None), ("-q", qry)):
        want, compared = R.expected_records(ent, q, return_compared=True, **kw)
        for env in ({}, {"MHAP_OVERLAP_PRUNE": "1"}, {"MHAP_OVERLAP": "lane"}):
            got, st = _search(monkeypatch, env, S, kw, ent, q)
            assert st["candidates_compared"] == compared, (mode, env, st, compared)
            assert got == want, (mode, env, _diff(got, want))
    if per_query == "many":
        assert compared == 300 * 300 and len(want) > 1000
