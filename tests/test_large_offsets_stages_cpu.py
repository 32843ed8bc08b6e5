"""What tests/test_large_offsets_stages_gpu.py stands on, without a GPU: the layouts put every mark where the GPU cases say, with the
same constants (tests/large_offsets_stages.py); a filler's written-out expectations are what the restatements give a read that
takes no record; the composition rule of the read of 2^31 - 9 bases holds against hpc_ref.compress_read on whole reads; and the
restatement on the five places laid back to back is, read by read, the restatement on one place plus each cross-place record's own
views.  The paths come from the restated aligner (tests/align_paths_ref.py), whose paths are the GPU aligner's."""
import numpy as np
import pytest

import align_paths_ref as pref
import consensus_ref as cref
import hpc_ref
import large_offsets as lo
import large_offsets_stages as los
import quality_ref as qref
import variant_ref as vr
import weighted_vote_ref as wref
from mhap_amd import api

M30, M31, M32 = lo.MARKS


@pytest.fixture(scope="module")
def realigned():
    """The part A workload with the restated aligner's records and paths."""
    reads, bases, pairs, meta = los.workload()
    results, op_offsets, ops = pref.align_pairs_banded_paths(bases, pairs)
    return reads, cref.quality_records(reads, meta, results), op_offsets, ops


# ---- the layouts ------------------------------------------------------------------------------------------------------------------------------

def _naive_starts(lengths, per_base):
    starts, at = [], 0
    for n in lengths:
        starts.append(at)
        at += per_base * n
    return starts, at


def test_the_marks_of_the_device_tables_lie_inside_their_straddlers(realigned):
    reads = realigned[0]
    tlen = [len(r) for r in reads]
    for make, per_base, straddlers, marks, planes in ((los.correction_layout, 12, los.VOTE_STRADDLERS, lo.MARKS, (2, 6, 10)),
                                                      (los.variant_layout, 3, los.VARIANT_STRADDLERS, lo.MARKS, (0, 1, 2)),
                                                      (los.site_layout, 1, los.SITE_STRADDLERS, los.SITE_MARKS, (0, 0))):
        lay, at = make(tlen)
        starts, total = _naive_starts(lay.lengths, per_base)
        assert starts == lay.starts and total == lay.total and total > M32 and all(isinstance(s, int) for s in starts)
        assert [lay.lengths[i] for i in lay.test] == tlen and all(1 <= lay.lengths[i] <= los.FILLER_BASES for i in lay.fillers)
        for mark, plane in zip(marks, planes):
            k, t = at[mark]
            i = lay.test[k]
            assert k == straddlers[mark] and starts[i] + plane * tlen[k] + t == mark and los.MARGIN <= t < tlen[k] - los.MARGIN
    lay, _ = los.site_layout(tlen)
    assert 12 * lay.total + lay.total >= los.SITE_TABLE_BYTES and 3 * lay.total > 3 * M32


def test_the_variant_workload_has_sites_round_every_mark_and_both_keeps(realigned):
    """What the GPU cases assert from the restatement before they run, here on the restated aligner's paths."""
    reads, recs, op_offsets, ops = realigned
    tlen = [len(r) for r in reads]
    v = vr.Variants(reads, range(1, len(reads) + 1), **los.VARIANT_PARAMS)
    v.add(recs, op_offsets, ops)
    counts = v.finish()
    assert counts[2] > 0
    los.sites_round(v, los.variant_layout(tlen)[1])
    lay, at = los.site_layout(tlen)
    los.sites_round(v, at)
    keep, _ = v.apply(recs, op_offsets, ops)
    assert set(keep.tolist()) == {0, 1}
    for mark in los.SITE_MARKS:
        assert los.records_across(lay, recs, mark) == {(True, 0), (True, 1), (False, 0), (False, 1)}, mark


def test_the_five_places_and_the_homopolymer_table():
    reads, _, _, _ = los.b_workload()
    P = los.Places(reads)
    assert P.size < M32 + (1 << 20) and len(P.ids) == len(set(P.ids.tolist())) == 5 * len(reads)
    for p, f in enumerate(los.PLACE_FIRSTS):
        assert P.at[p][0] == f and P.offsets[p * P.k] == f
    crossing = [r for r in range(len(P.ids)) for m in (M31, M32) if P.offsets[r] < m < P.offsets[r] + P.lengths[r]]
    assert crossing == [P.k, 3 * P.k]
    T = api.HPC_TILE
    H = los.HpcTable(T)                                                       # (its check runs in the constructor)
    assert los.HPC_SIZE < M32 + (1 << 20) and H.lengths[H.long] == lo.LONGEST and H.kinds.count(("zero",)) == los.HPC_ZERO_READS
    groups = los.plan_groups(H.lengths, los.HPC_GROUP_DEFAULT)
    assert len(groups) > 16 and sum(g[2] for g in groups) == int(H.lengths.astype(np.int64).sum()) and (H.long, H.long + 1, lo.LONGEST) in groups
    assert all(b <= los.HPC_GROUP_DEFAULT or e - s == 1 for s, e, b in groups)
    # the block: a read begins on the mark's offset and on the next, each behind a byte equal to its first; the mark lies inside a run
    c = H.content
    assert c[los.HPC_MARK_AT - 1] == c[los.HPC_MARK_AT] == c[los.HPC_MARK_AT + 1] and H.c not in (c[0], c[-1])
    for o, n in H.rows:
        assert n == 0 or o == 0 or c[o - 1] == c[o]


# ---- a filler's expected result --------------------------------------------------------------------------------------------------------------

def test_the_quality_lookup_is_what_the_restatements_give_voteless_reads():
    """Reads of 1 to 5 equal or mixed bytes that nobody voted on, every byte (N, lower case, 0 and 255 among them) and every class."""
    rng = np.random.default_rng(3)
    for min_cov, per_vote, cap in ((4, 15, 60), (1, 30, 93)):
        w_lut = los.filler_quality_lookup(True, min_cov, per_vote, cap)
        u_lut = los.filler_quality_lookup(False, min_cov, per_vote, cap)
        assert w_lut.shape == (256, 3, 2) and u_lut.shape == (256, 1, 2)
        for b, q_ends in ((b, q) for b in range(256) for q in (6, 7, 19, 20)):     # every byte in every class, first and last
            L = 1 + (b + q_ends) % 5
            own = bytes([b] * L) if b % 2 else bytes([b] + rng.integers(0, 256, max(L - 2, 0)).tolist() + [b])[:L]
            q = rng.choice(los.PHRED, L).astype(np.uint8)
            q[0] = q[-1] = q_ends
            votes = np.zeros((L, cref.NCOUNT), np.int64)
            seq, quals, counts = wref.call(own, q, votes, min_cov, per_vote, cap)
            arr, cls = np.frombuffer(own, np.uint8), los.weight_class(q)
            want = w_lut[arr, cls, 0]
            want[-1] = w_lut[arr[-1], cls[-1], 1]
            assert seq == own and quals.tolist() == want.tolist() and counts == (0, 0, 0, L)
            assert cls.tolist() == [wref.weight(int(x), wref.DEFAULT_Q_LO, wref.DEFAULT_Q_HI) - 1 for x in q]
            seq, quals = qref.call(own, votes, min_cov, per_vote, cap)
            want = u_lut[arr, 0, 0]
            want[-1] = u_lut[arr[-1], 0, 1]
            assert seq == own and quals.tolist() == want.tolist()
            fq = los.FillerQualities(u_lut, arr)
            assert fq.equals(quals, L) and fq.hist(L).tolist() == qref.histogram([quals]).tolist()
    lut = los.filler_quality_lookup(True)
    assert len({int(lut[ord("A"), c, 1]) for c in range(3)}) == 3 and lut[ord("N")].max() == 0    # the classes differ; an N has the fixed 0
    assert (lut[ord("A"), :, 0] <= lut[ord("A"), :, 1]).all() and lut[ord("A"), 2, 0] < lut[ord("A"), 2, 1]   # the last position has no stop margin


def test_a_filler_of_the_corrections_and_of_the_variant_table():
    """A table in which one read takes no record: the weighted correction, the unweighted one and the variant stage."""
    rng = np.random.default_rng(4)
    reads = [b"ACGTACGTAC", b"GATTACANNACGT", b"ACGTACGTAC"]
    quals = [rng.choice(los.PHRED, len(r)).astype(np.uint8) for r in reads]
    rec = cref.records_from_results([1], [3], [10], [10], [0], [[20, 0, 9, 0, 9, 10, 0]])
    off, ops = [0, 1], np.array([10 << 4 | 7], np.uint32)
    w = wref.WeightedConsensus(reads, quals, [1, 2, 3])
    w.add(rec, off, ops)
    assert not w.votes[1].any() and w.votes[0].any()
    seq, stats, q = w.call_read(1)
    assert (seq, list(stats)) == lo.correct_filler(reads[1])
    arr = np.frombuffer(reads[1], np.uint8)
    assert los.FillerQualities(los.filler_quality_lookup(True), arr, los.weight_class(quals[1])).equals(q, len(arr))
    lay = lo.Layout([10, 13, 10], [False, True, False], los.variant_words)
    for params in (los.VARIANT_PARAMS, dict(los.VARIANT_PARAMS, min_depth=2, min_minor=1, min_pct=0)):
        whole = vr.Variants(reads, [1, 2, 3], **params)
        small = vr.Variants([reads[0], reads[2]], [1, 3], **params)
        for v in (whole, small):
            v.add(np.concatenate([rec] * 3), [0, 1, 2, 3], np.concatenate([ops] * 3))
        want, counts = whole.finish(), small.finish()
        c, rows, offsets, sites = los.variant_with_fillers(lay, small, counts, params)
        assert c == want and rows.tolist() == whole.rows.tolist() and offsets.tolist() == whole.offsets.tolist() and sites.tolist() == whole.sites.tolist()
        assert whole.rows[1].tolist() == [0, 0] and whole.votes(1).sum() == 0 and want[3] == 20


# ---- the composition rule of the long read ---------------------------------------------------------------------------------------------------

def test_two_windows_and_a_filling_compose_to_the_whole_read():
    rng = np.random.default_rng(6)
    alphabet = np.array(list(b"ACGTNacgt") + [0, 255], np.uint8)
    seen = dict(a_ends_in_run=0, b_begins_in_run=0, fill_one=0, odd_filling=0)
    for draw in range(240):
        def window(n):
            k = n // 2 + 2
            return np.repeat(alphabet[rng.integers(0, len(alphabet), k)], rng.integers(1, 5, k))[:n]
        A, B = window(int(rng.integers(1, 3000))), window(int(rng.integers(1, 3000)))
        fill = 1 if draw % 4 == 0 else int(rng.integers(1, 4000))
        c = int(rng.choice([x for x in alphabet.tolist() if x != A[-1] and x != B[0]]))
        whole = np.concatenate([A, np.full(fill, c, np.uint8), B])
        heads, start = hpc_ref.compress_read(whole)
        got_heads, got_start = los.hpc_compose(A, c, fill, B)
        assert got_heads.tolist() == heads.tolist() and got_start.tolist() == start.tolist() and got_start.dtype == np.int32
        if fill > 1:
            assert int(np.diff(start).max()) >= fill
        seen["a_ends_in_run"] += len(A) > 1 and A[-1] == A[-2]
        seen["b_begins_in_run"] += len(B) > 1 and B[0] == B[1]
        seen["fill_one"] += fill == 1
        seen["odd_filling"] += c in (0, 255, ord("N"), ord("a"), ord("c"), ord("g"), ord("t"))
    assert min(seen.values()) >= 20, seen
    for bad in ((b"AC", ord("C"), 3, b"GT"), (b"AC", ord("G"), 3, b"GT"), (b"AC", ord("T"), 0, b"GT")):     # a filling that would join a run is refused
        with pytest.raises(AssertionError):
            los.hpc_compose(np.frombuffer(bad[0], np.uint8), bad[1], bad[2], np.frombuffer(bad[3], np.uint8))
    # the assembly of a table is hpc_ref.compress's
    seqs = [np.frombuffer(b"AACCCGT", np.uint8), np.zeros(0, np.uint8), np.zeros(9, np.uint8), np.frombuffer(b"TTTTA", np.uint8)]
    import hpc_cases as hc
    fa = hc.table(seqs)
    want = hpc_ref.compress(fa)
    got = los.hpc_assemble([hpc_ref.compress_read(s) for s in seqs], fa.lengths, fa.ids)
    assert got["counts"] == want["counts"] and all(got[k].tolist() == want[k].tolist() for k in ("cbases", "coff", "clen", "starts"))


# ---- the replication argument of the five places ---------------------------------------------------------------------------------------------

def test_five_places_back_to_back_are_one_place_and_each_cross_records_own_views():
    reads, bases, pairs, meta = los.b_workload()
    results, op_offsets, ops = pref.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    assert len(recs) >= 8 and {int(x) for x in recs["to_rc"]} == {0, 1}
    rng = np.random.default_rng(7)
    quals = [rng.choice(los.PHRED, len(r)).astype(np.uint8) for r in reads]
    P = los.Places(reads)
    big, boff, bops, where = P.records(recs, op_offsets, ops)
    assert len(big) == 12 * len(recs) and where.count((4, 1)) == len(recs)
    P.records_across(big, where)
    K, ids1 = P.k, list(range(1, P.k + 1))
    for weighted in (False, True):
        make = (lambda r, i: wref.WeightedConsensus(r, quals * (len(r) // K), i)) if weighted else (lambda r, i: cref.Consensus(r, i))
        one = make(reads, ids1)
        one.add(recs, op_offsets, ops)
        want = [one.votes[k].copy() for _ in range(5) for k in range(K)]
        # the per-place records alone: every place is the one place
        per_place = np.array([pa == pb for pa, pb in where])
        rows = np.flatnonzero(per_place)
        sel_off = np.concatenate([[0], np.cumsum(np.diff(boff)[rows])])
        sel_ops = np.concatenate([bops[boff[q]:boff[q + 1]] for q in rows])
        alone = make(P.small_reads, P.ids)
        alone.add(big[rows], sel_off, sel_ops)
        assert all(np.array_equal(alone.votes[r], want[r]) for r in range(5 * K))
        # every cross-place record adds its own two views, one to each of its reads
        for q in np.flatnonzero(~per_place):
            rec = big[q:q + 1].copy()
            pa, pb = where[q]
            x, y = int(rec["from_id"][0]) % los.ID_STEP - 1, int(rec["to_id"][0]) % los.ID_STEP - 1
            rec["from_id"], rec["to_id"] = x + 1, y + 1
            single = make(reads, ids1)
            single.add(rec, [0, boff[q + 1] - boff[q]], bops[boff[q]:boff[q + 1]])
            want[pa * K + x] = want[pa * K + x] + single.votes[x]
            want[pb * K + y] = want[pb * K + y] + single.votes[y]
            assert not any(single.votes[k].any() for k in range(K) if k not in (x, y))
        full = make(P.small_reads, P.ids)
        full.add(big, boff, bops)
        assert all(np.array_equal(full.votes[r], want[r]) for r in range(5 * K))
        assert full.skipped_views == 0 and max(full.views) < 1000
