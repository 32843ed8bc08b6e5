"""The entry points a multi-GPU host or the JNI shim calls (include/mhap_hip.h, INTEGRATION.md §6 "callers that own the device tables"):
the sharded and ranged self search, sketching into caller buffers, adopted device tables, the second-stage gate and a caller's stream.
Every expectation is the oracle's — O.run_self, or sketch_search_ref.expected_records over tables made from O.minhash / O.ordered /
O.overlap — never another GPU path's.  Device buffers are torch tensors; the library's kernels run on the handle's stream, torch's on
its own, so the tests synchronise wherever one side reads what the other wrote.

Corpora (section 1 of the shards / ranges):
  A  reads of one genome (true overlaps; some with N, some with IUPAC letters, one of 30 000 bases) with runs of placeholders between
     them: reads shorter than --min-olap-length (status 2) and reads of at least k2 but fewer than k bases (status 1).  Ids rise.
  B  the same reads under shuffled ids and --min-store-length 1500: no tile skipping, both id rules of MinHashSearch.java:211-225 live.
  C  the forward rows of A's sketched reads given to add_sketches: a read's ordinal is its entry index.
By the oracle alone every shard of every corpus at nshards <= 8 has records, and so has the range that starts and ends inside runs
of placeholders (asserted below, before any handle is made)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import mhap_amd
import oracle_lib as O
import sketch_search_ref as R
from mhap_amd import FastaData, MhapError, MhapParams, MinHashSearch, api

pytestmark = pytest.mark.gpu

H, S, MIN_OLAP, MIN_STORE_B = 128, 600, 14, 1500
SEARCH = dict(H=H, k2=12, num_min_matches=3, threshold=0.78, max_shift=0.2)
E_INVALID, E_STATE = -1, -4
SENTINEL = 0x5A5A5A5A
GUARD = 3
NSHARDS = (1, 2, 3, 7, 8)
PLACEHOLDER_RUNS = ((13,), (15, 9), (14, 13, 15), (9, 14, 15, 13))   # 9, 13: status 2 (< --min-olap-length 14); 14, 15: status 1 (< k)


def _params(**kw):
    return MhapParams(num_hashes=kw.pop("H", H), ordered_sketch_size=kw.pop("S", S), min_olap_length=MIN_OLAP, device=0, **kw)


def _lines(recs):
    return sorted(mhap_amd.records_to_lines(recs))


def _from_id(line):
    return int(line.split(" ", 1)[0])


def _rand_seq(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def _sprinkle(rnd, s, letters, every):
    s = list(s)
    for j in range(rnd.randrange(every), len(s), every):
        s[j] = rnd.choice(letters)
    return "".join(s)


# ---- corpora and their expectations (no GPU) ------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _genome():
    return np.random.default_rng(31).integers(0, 4, 36000, dtype=np.uint8)


@functools.lru_cache(None)
def _reads():
    """Corpus A as (FastaData, placeholder runs as (first read index, reads))."""
    rnd = random.Random(20261)
    lengths = np.random.default_rng(2).integers(700, 3600, 230)
    base = mhap_amd.synth_reads_from_genome(_genome(), lengths, seed=611, error_rate=0.06)
    long_read = mhap_amd.synth_reads_from_genome(_genome(), [30000], seed=5, error_rate=0.06).sequence(0)
    seqs, runs = [], []
    for i in range(len(base)):
        if i % 8 == 3:
            run = PLACEHOLDER_RUNS[(i // 8) % len(PLACEHOLDER_RUNS)]
            runs.append((len(seqs), len(run)))
            seqs += [_rand_seq(rnd, n) for n in run]
        s = base.sequence(i)
        if i % 37 == 5:
            s = _sprinkle(rnd, s, "N", 211)
        elif i % 37 == 20:
            s = _sprinkle(rnd, s, "RYKMSWBDHVN", 173)
        seqs.append(s)
        if i == 100:
            seqs.append(long_read)
    return FastaData.from_strings(seqs), tuple(runs)


@functools.lru_cache(None)
def _tables(Hh=H, Ss=S):
    return R.oracle_tables(_reads()[0], H=Hh, S=Ss, min_olap_length=MIN_OLAP)


class Case:
    """A corpus as the index holds it: how to load it, the oracle's records of its self search, and for every read id the index of
    its forward entry and its ordinal (its position among the forward entries, placeholders included)."""

    def __init__(self, name, params, load, want, entry_of, ordinal_of, size, queries):
        self.name, self.params, self.load, self.want = name, params, load, want
        self.entry_of, self.ordinal_of, self.size, self.queries = entry_of, ordinal_of, size, queries
        self.reads = len(ordinal_of)

    def shard(self, s, nshards):
        return [x for x in self.want if self.ordinal_of[_from_id(x)] % nshards == s]

    def range(self, q_first, q_count):
        q_end = self.size if q_count < 0 else min(self.size, q_first + q_count)
        return [x for x in self.want if q_first <= self.entry_of[_from_id(x)] < q_end]


@functools.lru_cache(None)
def _case(name):
    fa, _ = _reads()
    n = len(fa)
    if name in ("A", "B"):
        msl = MIN_STORE_B if name == "B" else 0
        if name == "B":
            fa = FastaData(fa.bases, fa.offsets, fa.lengths, np.random.default_rng(5).permutation(fa.ids))
        run = O.run_self(fa, H=H, S=S, min_olap_length=MIN_OLAP, min_store_length=msl, nthreads=16)
        ids = [int(x) for x in fa.ids]
        return Case(name, _params(min_store_length=msl), lambda ms: ms.add_data(fa), O.record_lines(run["records"]),
                    {rid: 2 * i for i, rid in enumerate(ids)}, {rid: i for i, rid in enumerate(ids)}, 2 * n,
                    int((run["status"][0::2] == 0).sum()))
    rows = R.stored_rows(_tables(), forward_only=True)
    want = R.expected_records(rows, min_store_length=0, **SEARCH)
    ids = [int(x) for x in rows["ids"]]
    return Case("C", _params(), lambda ms: ms.add_sketches(rows), want, {rid: i for i, rid in enumerate(ids)},
                {rid: i for i, rid in enumerate(ids)}, len(ids), len(ids))


def _ranges(case):
    """(q_first, q_count, least number of records the oracle must have in it) of the range cases."""
    size = case.size
    if case.name == "C":
        return [(0, -1, 1), (5, 33, 1), (7, 0, 0), (size, 3, 0), (size, -1, 0), (size - 9, 100, 0), (0, 1, 0)]
    runs = [r for r in _reads()[1] if r[1] >= 3]
    (a, _), (b, _) = runs[1], runs[4]
    inside = (2 * (a + 1), 2 * (b + 1) + 1 - 2 * (a + 1))        # from the second placeholder of one run into the second of a later one
    return [(0, -1, 1), (41, 61, 1), inside + (1,), (2 * a, 4, 0), (30, 0, 0), (size, 5, 0), (size, -1, 0), (size - 41, 1000, 0), (0, 1, 0)]


def _check_corpus(case):
    """Section 1's condition, from the oracle alone: no shard at nshards <= 8 and no range that claims records is empty."""
    assert len(case.want) > 300, (case.name, len(case.want))
    for nshards in NSHARDS:
        counts = [len(case.shard(s, nshards)) for s in range(nshards)]
        assert min(counts) >= 1 and sum(counts) == len(case.want), (case.name, nshards, counts)
    for q_first, q_count, least in _ranges(case):
        assert len(case.range(q_first, q_count)) >= least, (case.name, q_first, q_count)
    if case.name != "C":
        st = _tables()["status"]
        assert int((st[0::2] == 1).sum()) >= 10 and int((st[0::2] == 2).sum()) >= 10      # both kinds of placeholder, interleaved
        q_first, q_count, _ = _ranges(case)[2]
        assert st[q_first] != 0 and st[q_first + q_count - 1] != 0 and q_first % 2 == 0 and (q_first + q_count) % 2 == 1
        assert st[41] == 0 and _tables()["is_fwd"][41] == 0                                # a range that starts on a reverse entry


@functools.lru_cache(None)
def _queries():
    """-q reads for an index of corpus A: reads of the same genome under ids INSIDE the index's id range, copies of indexed reads under
    their own ids (toSelf = false keeps `from == to` and `to > from`; the toSelf rules would drop them) and reads too short to sketch."""
    fa, _ = _reads()
    rnd = random.Random(99)
    new = mhap_amd.synth_reads_from_genome(_genome(), np.random.default_rng(8).integers(900, 3000, 30), seed=77, error_rate=0.06)
    st = _tables()["status"]
    copies = [i for i in range(120, len(fa)) if st[2 * i] == 0][:10]
    seqs = [_rand_seq(rnd, 9)] + [new.sequence(i) for i in range(15)] + [_rand_seq(rnd, 14), _rand_seq(rnd, 15)]
    ids = [9001] + [3 * i + 2 for i in range(15)] + [9002, 9003]
    seqs += [fa.sequence(i) for i in copies] + [new.sequence(i) for i in range(15, 30)] + [_rand_seq(rnd, 13)]
    ids += [int(fa.ids[i]) for i in copies] + [3 * i + 2 for i in range(15, 30)] + [9004]
    fq = FastaData.from_strings(seqs)
    fq.ids[:] = ids
    tq = R.oracle_tables(fq, H=H, S=S, min_olap_length=MIN_OLAP, both_strands=False)
    want = R.expected_records(R.stored_rows(_tables()), R.stored_rows(tq), min_store_length=0, **SEARCH)
    froms_tos = [tuple(int(v) for v in x.split(" ")[:2]) for x in want]
    assert len(want) > 100 and sum(a == b for a, b in froms_tos) >= 10 and sum(a < b for a, b in froms_tos) >= 10
    assert int((tq["status"] != 0).sum()) == 4
    return fq, want


# ---- device tables ------------------------------------------------------------------------------------------------------------
def _sync():
    import torch
    torch.cuda.synchronize()


class DevTables:
    """MinHash, ordered and meta tensors of `rows` rows with GUARD rows of a sentinel in front of and behind each."""

    def __init__(self, rows, Hh=H, Ss=S):
        import torch
        self.rows = rows
        self.full = [torch.full((rows + 2 * GUARD,) + shape, SENTINEL, dtype=torch.int32, device=torch.device("cuda", 0))
                     for shape in ((max(1, Hh),), (Ss, 2), (4,))]
        self.mh, self.od, self.mt = (t[GUARD:GUARD + rows] for t in self.full)
        _sync()

    def ptrs(self):
        return self.mh.data_ptr(), self.od.data_ptr(), self.mt.data_ptr()

    def host(self):
        _sync()
        return tuple(t.cpu().numpy() for t in (self.mh, self.od, self.mt))

    def assert_guards(self, what):
        _sync()
        for t, name in zip(self.full, ("minhash", "ordered", "meta")):
            assert bool((t[:GUARD] == SENTINEL).all()) and bool((t[GUARD + self.rows:] == SENTINEL).all()), (what, name, "guard rows written")


def _sketched(ms, fa, Hh=H, Ss=S):
    dt = DevTables(2 * len(fa), Hh, Ss)
    ms.sketch_reads_device(fa, *dt.ptrs())
    return dt


def _entry_ids(fa):
    return np.repeat(fa.ids, 2), np.tile(np.array([1, 0], np.uint8), len(fa))


def _forward_rows(dt):
    q = tuple(t[0::2].contiguous() for t in (dt.mh, dt.od, dt.mt))
    _sync()
    return q


def _assert_rows(what, mh, od, meta, T, Ss):
    """Device rows against the oracle's: status and seq_length of every row; MinHash row, ordered_size, ordered_seqlen and the
    ordered row up to its size of every sketched one."""
    ok = T["status"] == 0
    assert np.array_equal(meta[:, 3], T["status"]), (what, "status", np.nonzero(meta[:, 3] != T["status"])[0][:8])
    assert np.array_equal(meta[:, 2], T["seq_length"]), (what, "seq_length")
    assert np.array_equal(meta[ok, 0], T["ordered_size"][ok]), (what, "ordered_size")
    assert np.array_equal(meta[ok, 1], T["ordered_seqlen"][ok]), (what, "ordered_seqlen")
    bad = np.nonzero(ok & (mh != T["minhash"]).any(axis=1))[0]
    assert len(bad) == 0, (what, "minhash", bad[:8])
    upto = (np.arange(Ss)[None, :] < T["ordered_size"][:, None]) & ok[:, None]
    bad = np.nonzero((od != T["ordered"]).any(axis=2) & upto)[0]
    assert len(bad) == 0, (what, "ordered", np.unique(bad)[:8])


# ---- 1. sharded and ranged self search ----------------------------------------------------------------------------------------------
def _assert_shards(ms, case, nshards_list, what):
    st0 = ms.stats()["queries_searched"]
    whole = _lines(ms.find_matches())
    whole_q = ms.stats()["queries_searched"] - st0
    assert whole == case.want and whole_q == case.queries, (what, len(whole), len(case.want), whole_q, case.queries)
    for nshards in nshards_list:
        parts, searched = [], 0
        for s in range(nshards):
            before = ms.stats()["queries_searched"]
            got = _lines(ms.find_matches_shard(s, nshards))
            searched += ms.stats()["queries_searched"] - before
            want = case.shard(s, nshards)
            if nshards <= 8:
                assert len(want) >= 1
            assert got == want, (what, nshards, s, len(got), len(want))
            parts.append(got)
        seen = set()
        for s, got in enumerate(parts):
            assert len(set(got)) == len(got) and not (seen & set(got)), (what, nshards, s, "shards overlap")
            seen |= set(got)
        assert seen == set(case.want) and sum(len(x) for x in parts) == len(case.want), (what, nshards, "union")
        assert searched == whole_q, (what, nshards, searched, whole_q)


@pytest.mark.parametrize("corpus", ["A", "B", "C"])
def test_shards_of_a_self_search_partition_the_oracles_records(corpus, monkeypatch):
    """mhap_find_matches_self_shard: shard s of n is exactly the oracle's records whose query read has ordinal % n == s — the ordinal counts
    forward entries, placeholders included — for n = 1, 2, 3, 7, 8 and one n above the number of reads; the shards are pairwise
    disjoint, their union is the whole search and so is the sum of their queries_searched.  With the inverted index and with the
    brute-force candidate tiles (the only path that skips tiles by id order), each with and without MHAP_NO_TRIANGULAR."""
    case = _case(corpus)
    _check_corpus(case)
    for cand in (None, "bruteforce"):
        for no_tri in (False, True):
            monkeypatch.delenv("MHAP_CANDIDATES", raising=False)
            monkeypatch.delenv("MHAP_NO_TRIANGULAR", raising=False)
            if cand:
                monkeypatch.setenv("MHAP_CANDIDATES", cand)
            if no_tri:
                monkeypatch.setenv("MHAP_NO_TRIANGULAR", "1")
            with MinHashSearch(case.params) as ms:
                case.load(ms)
                assert ms.size() == case.size
                _assert_shards(ms, case, NSHARDS + (() if no_tri else (case.reads + 5,)), (corpus, cand, no_tri))


def test_shards_on_two_compute_units(monkeypatch):
    """The shards of corpus A with every persistent grid sized for two compute units (MHAP_NUM_CUS=2)."""
    case = _case("A")
    _check_corpus(case)
    monkeypatch.setenv("MHAP_NUM_CUS", "2")
    with MinHashSearch(case.params) as ms:
        case.load(ms)
        _assert_shards(ms, case, NSHARDS, "two compute units")


@pytest.mark.parametrize("corpus", ["A", "B", "C"])
def test_ranged_self_search_against_the_oracle(corpus):
    """mhap_find_matches_self(q_first, q_count): the oracle's records whose query entry lies in the range — a range that starts on a reverse
    entry, one that starts and ends inside runs of placeholders, one that covers placeholders only, q_count = 0, q_first = size()
    (empty, MHAP_OK), q_count past the end, and a cover of the index by ranges with odd borders."""
    case = _case(corpus)
    _check_corpus(case)
    with MinHashSearch(case.params) as ms:
        case.load(ms)
        size = ms.size()
        assert size == case.size
        for q_first, q_count, least in _ranges(case):
            want = case.range(q_first, q_count)
            assert len(want) >= least
            assert _lines(ms.find_matches(q_first, q_count)) == want, (corpus, q_first, q_count, len(want))
        cuts = [0, 37, 38, 211, 212, size]
        parts = [_lines(ms.find_matches(a, b - a)) for a, b in zip(cuts, cuts[1:])]
        for (a, b), got in zip(zip(cuts, cuts[1:]), parts):
            assert got == case.range(a, b - a), (corpus, a, b)
        assert sorted(x for p in parts for x in p) == case.want


def test_bad_shard_and_range_arguments_are_refused_and_the_handle_survives():
    """shard < 0, shard >= nshards, nshards < 1, q_first < 0 and q_first > size(): MHAP_E_INVALID with the message of self_search, before any
    launch; the same handle then gives the oracle's records."""
    case = _case("A")
    want = case.shard(1, 3)
    assert len(want) >= 1
    with MinHashSearch(case.params) as ms:
        case.load(ms)
        size = ms.size()
        bad = [(lambda: ms.find_matches_shard(-1, 4), "bad shard"), (lambda: ms.find_matches_shard(4, 4), "bad shard"),
               (lambda: ms.find_matches_shard(0, 0), "bad shard"), (lambda: ms.find_matches_shard(0, -2), "bad shard"),
               (lambda: ms.find_matches(-1, 5), "query range outside the index"),
               (lambda: ms.find_matches(size + 1, 1), "query range outside the index")]
        for call, message in bad:
            before = ms.stats()
            with pytest.raises(MhapError, match=rf"^{message} \(code {E_INVALID}\)$"):
                call()
            assert ms.stats() == before
            assert _lines(ms.find_matches_shard(1, 3)) == want
        assert _lines(ms.find_matches(size, -1)) == [] and _lines(ms.find_matches()) == case.want


# ---- 2. sketching into caller buffers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hh,Ss", [(1, 256), (96, 512), (64, 100)])
def test_sketches_in_caller_buffers_match_the_oracle(Hh, Ss):
    """mhap_sketch_reads_device, mhap_stage_reads + mhap_sketch_staged_device and mhap_sketch_batch on corpus A (reads with N, with IUPAC
    letters, shorter than k, shorter than --min-olap-length, one of 30 000 bases): the oracle's MinHash rows, its ordered rows up to
    ordered_size, and the meta words {ordered_size, ordered_seqlen, seq_length, status}; at --num-hashes 1 (a MinHash row is
    max(1, H) words), at 96, and at an --ordered-sketch-size that is no multiple of 64.  Guard rows around every tensor stay untouched."""
    fa, _ = _reads()
    T = R.oracle_tables(fa, H=Hh, S=Ss, min_olap_length=MIN_OLAP)
    assert sorted(int(x) for x in np.unique(T["status"])) == [0, 1, 2] and int(fa.lengths.max()) == 30000
    p = _params(H=Hh, S=Ss)
    with MinHashSearch(p) as ms:
        direct = _sketched(ms, fa, Hh, Ss)
        _assert_rows("sketch_reads_device", *direct.host(), T, Ss)
        direct.assert_guards("sketch_reads_device")
        staged = DevTables(2 * len(fa), Hh, Ss)
        ms.stage(fa)
        ms.sketch_staged_device(*staged.ptrs())
        ms.synchronize()
        _assert_rows("sketch_staged_device", *staged.host(), T, Ss)
        staged.assert_guards("sketch_staged_device")
        sk = ms.sketch(fa)
    meta = np.stack([sk["ordered_size"], T["ordered_seqlen"], T["seq_length"], sk["status"].astype(np.int32)], axis=1)   # (sketch() returns no lengths)
    _assert_rows("sketch", sk["minhash"], sk["ordered"], meta, T, Ss)
    assert not sk["ordered_size"][T["status"] != 0].any()


# ---- 3. adopted device tables -------------------------------------------------------------------------------------------------------------
def test_adopted_tables_of_one_rank_search_like_the_librarys_own():
    """mhap_index_set_device over the tables mhap_sketch_reads_device made: size, strands_indexed, export() = the tensors, the self search =
    the oracle's, -q reads (mhap_find_matches_reads) and -q rows in device memory (mhap_find_matches_device, to_self = 0, rows that were
    not sketched among them) = the oracle's toSelf = false records."""
    fa, _ = _reads()
    T, case = _tables(), _case("A")
    fq, want_q = _queries()
    with MinHashSearch(case.params) as ms:
        dt = _sketched(ms, fa)
        ids, is_fwd = _entry_ids(fa)
        ms.set_device_index(ids, is_fwd, *dt.ptrs())
        assert ms.size() == 2 * len(fa)
        assert ms.stats()["strands_indexed"] == int((T["status"] == 0).sum())
        mh, od, mt = dt.host()
        ex = ms.export()
        assert np.array_equal(ex["ids"], ids) and np.array_equal(ex["is_fwd"], is_fwd)
        assert np.array_equal(ex["minhash"], mh) and np.array_equal(ex["ordered"], od)
        for word, key in enumerate(("ordered_size", "ordered_seqlen", "seq_length", "status")):
            assert np.array_equal(ex[key], mt[:, word]), key
        _assert_rows("export", ex["minhash"], ex["ordered"], mt, T, S)
        assert _lines(ms.find_matches()) == case.want
        assert _lines(ms.find_matches_stream(fq)) == want_q
        qt = _sketched(ms, fq)                                     # (sketching next to an adopted index leaves it alone)
        q = _forward_rows(qt)
        assert int((q[2][:, 3] != 0).sum().item()) == 4
        got = _lines(ms.find_matches_device(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), fq.ids, to_self=False))
        assert got == want_q, (len(got), len(want_q))
        assert _lines(ms.find_matches()) == case.want
        dt.assert_guards("adopted tables")
        qt.assert_guards("query rows")


def test_adopted_tables_gathered_from_two_ranks():
    """Two handles sketch their round-robin halves into their own tensors; the parts concatenated in rank-major order, with the matching
    ids, are a third handle's index: its self search is the oracle's on the whole data set (the ids no longer rise with the entries)."""
    import torch
    fa, _ = _reads()
    case = _case("A")
    parts = [fa.subset(np.arange(r, len(fa), 2)) for r in (0, 1)]
    with MinHashSearch(case.params) as r0, MinHashSearch(case.params) as r1, MinHashSearch(case.params) as ms:
        tabs = [_sketched(h, part) for h, part in zip((r0, r1), parts)]
        mh, od, mt = (torch.cat([getattr(t, name) for t in tabs]) for name in ("mh", "od", "mt"))
        _sync()
        ids = np.concatenate([_entry_ids(part)[0] for part in parts])
        is_fwd = np.concatenate([_entry_ids(part)[1] for part in parts])
        ms.set_device_index(ids, is_fwd, mh.data_ptr(), od.data_ptr(), mt.data_ptr())
        assert ms.size() == 2 * len(fa)
        assert _lines(ms.find_matches()) == case.want
        for nshards in (2, 3):
            got = sorted(x for s in range(nshards) for x in _lines(ms.find_matches_shard(s, nshards)))
            assert got == case.want, nshards


def test_index_prepare_reads_no_ordered_row():
    """mhap_index_prepare's contract: the tables are adopted with the ordered tensor full of garbage, the index is prepared, the real rows
    are copied in afterwards — the search is the oracle's and builds no index of its own."""
    import torch
    fa, _ = _reads()
    case = _case("A")
    with MinHashSearch(case.params) as ms:
        dt = _sketched(ms, fa)
        garbage = torch.randint(-(1 << 31), (1 << 31) - 1, tuple(dt.od.shape), dtype=torch.int64, device=dt.od.device).to(torch.int32)
        _sync()
        ids, is_fwd = _entry_ids(fa)
        ms.set_device_index(ids, is_fwd, dt.mh.data_ptr(), garbage.data_ptr(), dt.mt.data_ptr())
        ms.reset_kernel_times()
        ms.prepare_index()
        assert ms.kernel_times()["index_build"]["launches"] == 1
        garbage.copy_(dt.od)
        _sync()
        assert _lines(ms.find_matches()) == case.want
        kt = ms.kernel_times()
        assert kt["index_build"]["launches"] == 1 and kt["index_query"]["launches"] >= 1, kt


def test_adopted_index_refuses_adds_until_cleared_and_can_be_replaced():
    """An adopted index takes no reads (MHAP_E_STATE); mhap_index_clear gives the handle its own tables back; m = 0 is an index that finds
    nothing; a second set of tables adopted over a first one is the one searched."""
    import torch
    fa, _ = _reads()
    case = _case("A")
    half = fa.subset(np.arange(0, len(fa) // 2))
    want_half = O.record_lines(O.run_self(half, H=H, S=S, min_olap_length=MIN_OLAP, nthreads=16)["records"])
    assert 50 < len(want_half) < len(case.want)
    with MinHashSearch(case.params) as ms:
        whole, part = _sketched(ms, fa), _sketched(ms, half)
        ms.set_device_index(*_entry_ids(fa), *whole.ptrs())
        for add in (lambda: ms.add_data(half), lambda: ms.add_sketches(R.stored_rows(_tables()))):
            with pytest.raises(MhapError, match=rf"externally owned \(mhap_index_set_device\); clear the index first \(code {E_STATE}\)$"):
                add()
            assert ms.size() == 2 * len(fa)
        assert _lines(ms.find_matches()) == case.want
        # a second set over the first, of the same size: the reads in reverse order (an inverted index kept from the first set
        # would send every query to the wrong entries)
        back = np.arange(len(fa))[::-1].copy()
        order = torch.as_tensor(np.stack([2 * back, 2 * back + 1], axis=1).reshape(-1), device=whole.mh.device)
        turned = [t.index_select(0, order) for t in (whole.mh, whole.od, whole.mt)]
        _sync()
        ms.set_device_index(*_entry_ids(fa.subset(back)), *(t.data_ptr() for t in turned))
        assert ms.size() == 2 * len(fa) and _lines(ms.find_matches()) == case.want
        ms.set_device_index(*_entry_ids(half), *part.ptrs())          # and a smaller one over that
        assert ms.size() == 2 * len(half) and _lines(ms.find_matches()) == want_half
        ms.set_device_index(np.zeros(0, np.int64), np.zeros(0, np.uint8), 0, 0, 0)
        assert ms.size() == 0 and ms.stats()["strands_indexed"] == 0 and len(ms.find_matches()) == 0
        assert len(ms.find_matches_stream(_queries()[0])) == 0
        ms.set_device_index(*_entry_ids(fa), *whole.ptrs())
        assert _lines(ms.find_matches()) == case.want
        ms.clear()
        assert ms.size() == 0
        ms.add_data(half)
        assert _lines(ms.find_matches()) == want_half
        ms.add_data(fa.subset(np.arange(len(fa) // 2, len(fa))))
        assert _lines(ms.find_matches()) == case.want
        whole.assert_guards("whole")
        part.assert_guards("half")


# ---- 4. the second-stage gate ---------------------------------------------------------------------------------------------------------------
def _garbage_like(t):
    import torch
    g = torch.randint(-(1 << 31), (1 << 31) - 1, tuple(t.shape), dtype=torch.int64, device=t.device).to(torch.int32)
    _sync()
    return g


def _device_search(ms, q, ids, to_self, sink=None):
    """mhap_find_matches_device called directly: (return code, records or None with a sink of the caller's)."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)

    def call(cb):
        return ms._lib.mhap_find_matches_device(ms._h, C.c_void_p(q[0].data_ptr()), C.c_void_p(q[1].data_ptr()), C.c_void_p(q[2].data_ptr()),
                                                api._ptr(ids), C.c_int64(len(ids)), C.c_int(1 if to_self else 0), cb, None)
    if sink is not None:
        return call(sink), None
    rc = [0]
    recs = api._collect_records(call, lambda r: rc.__setitem__(0, r))
    return rc[0], recs


@pytest.mark.parametrize("prune", [None, "1"])
def test_no_ordered_query_row_is_read_before_the_gate(prune, monkeypatch):
    """The gate's contract (include/mhap_hip.h): the query rows' ordered tensor holds random int32 values — positions far outside any
    read among them — until the gate copies the real rows in; the records are the oracle's.  With the position-histogram pass of the
    second stage off (the default at these candidate counts) and on (MHAP_OVERLAP_PRUNE=1: it reads every query row, behind the gate)."""
    fa, _ = _reads()
    case = _case("A")
    if prune:
        monkeypatch.setenv("MHAP_OVERLAP_PRUNE", prune)
    with MinHashSearch(case.params) as ms:
        q_mh, q_real, q_mt = _forward_rows(_sketched(ms, fa))
        ms.add_data(fa)
        q_od = _garbage_like(q_real)
        calls = []

        def fill():
            calls.append(1)
            q_od.copy_(q_real)
            _sync()
        got = _lines(ms.find_matches_device(q_mh.data_ptr(), q_od.data_ptr(), q_mt.data_ptr(), fa.ids, to_self=True, before_second_stage=fill))
        assert calls == [1] and got == case.want, (prune, len(got), len(case.want))


def test_gate_is_called_once_per_chunk_with_candidates(monkeypatch):
    """With MHAP_QUERY_CHUNK=128 the C gate runs once for every chunk of queries that has candidates (at least two calls here, at most
    one per chunk), not at all for a search without candidates, and never again once it is removed."""
    fa, _ = _reads()
    case = _case("A")
    rnd = random.Random(3)
    strangers = FastaData.from_strings([_rand_seq(rnd, 1500) for _ in range(40)])
    ts = R.oracle_tables(strangers, H=H, S=S, min_olap_length=MIN_OLAP)
    assert R.expected_pairs(R.stored_rows(ts), R.stored_rows(_tables(), forward_only=True), num_min_matches=3, min_store_length=0) == []
    monkeypatch.setenv("MHAP_QUERY_CHUNK", "128")
    chunks = (len(fa) + 127) // 128
    assert chunks >= 3
    calls = []
    gate = api._GATE(lambda user: calls.append(1) or 0)
    with MinHashSearch(case.params) as ms, MinHashSearch(case.params) as other:
        q = _forward_rows(_sketched(ms, fa))
        ms.add_data(fa)
        other.add_data(strangers)
        for h in (ms, other):
            assert h._lib.mhap_set_second_stage_gate(h._h, gate, None) == 0
        rc, recs = _device_search(other, q, fa.ids, False)
        assert rc == 0 and len(recs) == 0 and calls == []
        rc, recs = _device_search(ms, q, fa.ids, True)
        assert rc == 0 and _lines(recs) == case.want
        assert 2 <= len(calls) <= chunks, (len(calls), chunks)
        seen = len(calls)
        assert ms._lib.mhap_set_second_stage_gate(ms._h, api._GATE(0), None) == 0
        rc, recs = _device_search(ms, q, fa.ids, True)
        assert rc == 0 and _lines(recs) == case.want and len(calls) == seen


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_gate_can_abort_a_search_and_the_handle_survives(pipeline, monkeypatch):
    """A gate that returns non-zero ends the search with MHAP_E_STATE "second-stage gate aborted the search", at its first call (no record
    was made yet) and at its second (the first chunk's records may be on their way to the sink: every record delivered is one of the
    oracle's, and none arrives once the call has returned); with the gate removed the same handle gives the oracle's records.  With the
    chunks' tails on the library's worker thread and inline (MHAP_SEARCH_PIPELINE=0)."""
    fa, _ = _reads()
    case = _case("A")
    monkeypatch.setenv("MHAP_QUERY_CHUNK", "128")
    monkeypatch.setenv("MHAP_SEARCH_PIPELINE", pipeline)
    with MinHashSearch(case.params) as ms:
        q = _forward_rows(_sketched(ms, fa))
        ms.add_data(fa)
        for stop_at in (1, 2):
            state = {"gate": 0, "returned": False, "late": 0}
            got = []

            def gate_fn(user):
                state["gate"] += 1
                return 7 if state["gate"] == stop_at else 0

            def sink_fn(recs, n, user):
                if state["returned"]:
                    state["late"] += 1
                got.append(np.frombuffer(C.string_at(recs, n * api.RECORD_DTYPE.itemsize), dtype=api.RECORD_DTYPE))
                return 0
            gate, sink = api._GATE(gate_fn), api._SINK(sink_fn)
            assert ms._lib.mhap_set_second_stage_gate(ms._h, gate, None) == 0
            rc, _ = _device_search(ms, q, fa.ids, True, sink=sink)
            state["returned"] = True
            assert rc == E_STATE and ms._lib.mhap_last_error(ms._h) == b"second-stage gate aborted the search", (pipeline, stop_at, rc)
            assert state["gate"] == stop_at
            delivered = _lines(np.concatenate(got)) if got else []
            assert len(delivered) < len(case.want) and set(delivered) <= set(case.want) and len(set(delivered)) == len(delivered)
            if stop_at == 1:
                assert delivered == []
            assert ms._lib.mhap_set_second_stage_gate(ms._h, api._GATE(0), None) == 0
            rc, recs = _device_search(ms, q, fa.ids, True)
            assert rc == 0 and _lines(recs) == case.want and state["late"] == 0 and state["gate"] == stop_at


# ---- 5. a caller's stream -------------------------------------------------------------------------------------------------------------------
def test_searches_on_a_callers_stream():
    """mhap_set_stream: the library's work goes to the caller's stream — an add and a search there, an adopted-table search there, the
    stream switched between the add and the search and between two searches, and back to the library's own (0): the oracle's records every
    time.  The tensors the library reads are complete before it is called (the tests synchronise; the header promises no more)."""
    import torch
    fa, _ = _reads()
    case = _case("A")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with MinHashSearch(case.params) as ms, MinHashSearch(case.params) as adopted:
        ms.set_stream(s1.cuda_stream)
        ms.add_data(fa)
        assert _lines(ms.find_matches()) == case.want
        ms.set_stream(s2.cuda_stream)                        # between an add and a search
        assert _lines(ms.find_matches_shard(1, 3)) == case.shard(1, 3)
        ms.set_stream(s1.cuda_stream)                        # between two searches
        assert _lines(ms.find_matches()) == case.want
        ms.set_stream(0)
        assert _lines(ms.find_matches()) == case.want
        ms.clear()
        ms.set_stream(s2.cuda_stream)
        ms.add_data(fa)
        ms.set_stream(0)
        assert _lines(ms.find_matches()) == case.want

        adopted.set_stream(s1.cuda_stream)
        dt = _sketched(adopted, fa)
        _assert_rows("sketch_reads_device on a caller's stream", *dt.host(), _tables(), S)
        adopted.set_device_index(*_entry_ids(fa), *dt.ptrs())
        assert _lines(adopted.find_matches()) == case.want
        adopted.set_stream(s2.cuda_stream)
        q = _forward_rows(dt)
        assert _lines(adopted.find_matches_device(q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr(), fa.ids, to_self=True)) == case.want
        adopted.set_stream(0)
        assert _lines(adopted.find_matches()) == case.want
        dt.assert_guards("caller's stream")
