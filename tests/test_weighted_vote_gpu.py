"""The quality-weighted votes on the GPU (mhap_correct_begin_weighted, mhap_consensus_begin_weighted; weighted_vote.hpp) against their
restatement (tests/weighted_vote_ref.py), counter for counter and byte for byte: the correction over the crafted piles of the base-quality
tests with qualities of every class, paths round the walk's chunk of 64 runs, own weights that decide a tie, the cap of 21 845 views,
the middle-class identity next to an unweighted session, the unitig consensus round its tile of 4 096, and the weighted workload."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import consensus_ref as cref  # noqa: E402
import handmade_paths as hp  # noqa: E402
import quality_ref as qref  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import test_quality_gpu as tq  # noqa: E402
import test_unitig_consensus_gpu as tuc  # noqa: E402
import test_weighted_vote_cpu as twc  # noqa: E402
import weighted_vote_ref as wref  # noqa: E402
from align_ref import rc_bytes  # noqa: E402
from mhap_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = tuc.TILE
CLASSES = (0, 5, 6, 7, 14, 19, 20, 30, 93)     # Phred values on both sides of the thresholds of every parameter set below
PARAMS = [(7, 20), (6, 15), (0, 93)]           # (7, 20): the defaults; (0, 93): nothing weighs 1, only Q93 weighs 3


def _quals(rng, reads, values=CLASSES):
    return [rng.choice(values, len(r)).astype(np.uint8) for r in reads]


def _fasta(reads, quals):
    f = tq._fasta(reads)
    f.qualities = np.concatenate(quals).astype(np.uint8) if len(reads) else np.zeros(0, np.uint8)
    return f


def _session(reads, quals, q_lo, q_hi, **kw):
    f = _fasta(reads, quals)
    return mhap_amd.CorrectSession(f, qualities=api.all_qualities(f), weights=api.WeightParams(q_lo, q_hi), **kw)


def _compare(cs, ref, reads, min_cov=4, per_vote=15, cap=60):
    """Counters, bytes, the six counts, the output qualities and their histogram of every read."""
    for r in range(len(reads)):
        v = cs.votes(r).astype(np.int64)
        rows = np.flatnonzero((v != ref.votes[r]).any(axis=1))
        assert len(rows) == 0, (r, rows[:5], v[rows[:3]], ref.votes[r][rows[:3]])
    seqs, stats, skipped = cs.finish(min_cov)
    quals, hist = cs.quality(per_vote, cap)
    want = [ref.call_read(r, min_cov, per_vote, cap) for r in range(len(reads))]
    assert [bytes(s) for s in seqs] == [w[0] for w in want]
    assert stats.tolist() == [list(w[1]) for w in want]
    for r, (g, w) in enumerate(zip(quals, want)):
        assert g.tolist() == w[2].tolist(), r
    assert hist.tolist() == qref.histogram([w[2] for w in want]).tolist()
    assert skipped == ref.skipped_views
    return seqs, stats, quals


@pytest.fixture(scope="module")
def pile():
    """The pile of tests/test_quality_gpu.py (reads of 1, 2, 255, 256, 257 and 513 bases; substitutions, deletions and insertions of 1, 4
    and 5 bytes at 255, 256 and the read's end, every other evidence read stored reverse-complemented; Ns) with a quality drawn per base."""
    reads, recs, off, ops, untouched = tq._pile()
    return reads, _quals(np.random.default_rng(8), reads), recs, off, ops


@pytest.mark.parametrize("q_lo,q_hi", PARAMS)
def test_correction_equals_the_restatement(pile, q_lo, q_hi):
    """Each parameter set a session of its own: every weight class lands on M columns, on Ins slots 0 .. 3 and on a fifth inserted
    byte, in view A, in view B and in view B of a to_rc record, on Ns and next to Del columns; own bytes of every class."""
    reads, quals, recs, off, ops = pile
    ref = wref.WeightedConsensus(reads, quals, range(1, len(reads) + 1), q_lo, q_hi)
    ref.add(recs, off, ops)
    with _session(reads, quals, q_lo, q_hi) as cs:
        half = len(recs) // 2                                            # split over two calls: the same sums
        cs.add(recs[:half], off[:half + 1], ops[:off[half]])
        cs.add(recs[half:], off[half:] - off[half], ops[off[half]:])
        _compare(cs, ref, reads)
        _compare(cs, ref, reads, min_cov=1, per_vote=1000, cap=93)
    weights = {wref.weight(int(q), q_lo, q_hi) for q in np.concatenate(quals)}
    assert weights == ({2, 3} if q_lo == 0 else {1, 2, 3})


@pytest.mark.parametrize("total_runs", [63, 65, 129])
@pytest.mark.parametrize("to_rc", [0, 1])
def test_paths_round_the_chunk_of_64_runs(total_runs, to_rc):
    """Paths of 63, 65 and 129 runs and, through a D run turned into D I, of 64: a gap of 5 columns on the last run of a chunk and on
    the first of the next, both kinds, so that both views see a fifth inserted byte there."""
    rng = np.random.default_rng(100 * total_runs + to_rc)
    reads, recs, ops, off = [], [], [], [0]
    paths = [hp.runs_with(kind, 5, at, total_runs) for kind in "DI" for at in {min(63, total_runs - 2), min(64, total_runs - 2), 1}]
    if total_runs == 63:                                                 # 64 runs: an I run behind the D run of a 63-run path
        p = hp.runs_with("D", 5, 31, 63)
        paths.append(hp.check_canonical(p[:32] + [hp.run("I", 2)] + p[32:]))
        assert len(paths[-1]) == 64
    for runs in paths:
        A, s2 = hp.pair_from_runs(rng, runs, (3, 2), (1, 4))
        reads += [A, rc_bytes(s2) if to_rc else s2]
        recs.append(hp.record_for(len(reads) - 1, len(reads), A, s2, 3, 1, runs, to_rc))
        ops.extend(runs)
        off.append(len(ops))
    quals = _quals(rng, reads, (5, 14, 30))
    ref = wref.WeightedConsensus(reads, quals, range(1, len(reads) + 1), 7, 20)
    recs, off, ops = np.concatenate(recs), np.array(off, np.int64), np.array(ops, np.uint32)
    ref.add(recs, off, ops)
    with _session(reads, quals, 7, 20) as cs:
        cs.add(recs, off, ops)
        _compare(cs, ref, reads, min_cov=1)


@pytest.mark.parametrize("to_rc", [0, 1])
def test_own_weight_decides_a_tie(to_rc):
    """Targets CTC under one view that says G in the middle, min_cov 1 (d = 2 = 2 min_cov): an evidence byte of weight 3 against an own
    byte of weight 1, 2, 3, and one of weight 2 against the same.  The own byte stays exactly when its weight reaches the evidence's."""
    reads, quals, recs, ops, off = [], [], [], [], [0]
    runs = hp.cigar("1= 1X 1=")
    for q_e in (30, 14):
        for q_own in (5, 14, 30):
            e = b"CGC"
            reads += [b"CTC", rc_bytes(e) if to_rc else e]
            quals += [np.array([14, q_own, 14], np.uint8), np.array([14, q_e, 14], np.uint8)]
            recs.append(hp.record_for(len(reads) - 1, len(reads), b"CTC", e, 0, 0, runs, to_rc))
            ops.extend(runs)
            off.append(len(ops))
    recs, off, ops = np.concatenate(recs), np.array(off, np.int64), np.array(ops, np.uint32)
    ref = wref.WeightedConsensus(reads, quals, range(1, len(reads) + 1), 7, 20)
    ref.add(recs, off, ops, views=[1] * len(recs))
    with _session(reads, quals, 7, 20) as cs:
        cs.add(recs, off, ops, views=np.full(len(recs), 1, np.uint8))    # view A only: the targets are the CTC reads
        seqs, _, _ = _compare(cs, ref, reads, min_cov=1)
    assert [bytes(s) for s in seqs[0::2]] == [b"CGC", b"CGC", b"CTC", b"CGC", b"CTC", b"CTC"]


def test_the_cap_of_21845_views():
    """21 846 views on a read of 2 bases, every evidence byte of weight 3: exactly one is skipped and the counters stand at 65 535."""
    n = wref.CAP + 1
    reads, quals = [b"GA", b"GA"], [np.array([30, 30], np.uint8)] * 2
    rec = hp.record_for(1, 2, b"GA", b"GA", 0, 0, [2 << 4 | cref.OP_EQ], 0)
    recs = np.concatenate([rec] * n)
    off, ops = np.arange(n + 1, dtype=np.int64), np.full(n, 2 << 4 | cref.OP_EQ, np.uint32)
    with _session(reads, quals, 7, 20) as cs:
        cs.add(recs[:1000], off[:1001], ops[:1000], views=np.full(1000, 1, np.uint8))
        cs.add(recs[1000:], off[1000:] - 1000, ops[1000:], views=np.full(n - 1000, 1, np.uint8))
        v = cs.votes(0).astype(np.int64)
        seqs, stats, skipped = cs.finish(4)
        assert skipped == 1 and api.WEIGHTED_VIEW_CAP == wref.CAP == 21845
        assert v[0].tolist() == [0, 0, 65535, 0, 0, 2 * wref.CAP] + [0] * 18 and v[1].tolist() == [65535] + [0] * 23
        assert cs.votes(1).any() == False and [bytes(s) for s in seqs] == reads    # noqa: E712


def test_middle_class_identity_on_the_device(pile):
    """Every quality in [q_lo, q_hi): next to an unweighted session on the same records the counters are exactly double, and the bytes,
    the six counts, the qualities and their histogram are identical."""
    reads, _, recs, off, ops = pile
    quals = _quals(np.random.default_rng(9), reads, (7, 10, 14, 19))
    with _session(reads, quals, 7, 20) as ws, mhap_amd.CorrectSession(tq._fasta(reads)) as us:
        ws.add(recs, off, ops)
        us.add(recs, off, ops)
        for r in range(len(reads)):
            assert np.array_equal(ws.votes(r).astype(np.int64), 2 * us.votes(r).astype(np.int64)), r
        for min_cov in (4, 1):
            (wseq, wst, wsk), (useq, ust, usk) = ws.finish(min_cov), us.finish(min_cov)
            assert wseq == useq and wst.tolist() == ust.tolist() and wsk == usk == 0
            for per_vote, cap in ((15, 60), (7, 93)):
                (wq, wh), (uq, uh) = ws.quality(per_vote, cap), us.quality(per_vote, cap)
                assert all(a.tolist() == b.tolist() for a, b in zip(wq, uq)) and wh.tolist() == uh.tolist()


def test_begin_refusals_and_the_unweighted_sibling(pile):
    reads, quals, recs, off, ops = pile
    for q_lo, q_hi in ((-1, 5), (6, 5), (0, 94)):
        with pytest.raises(mhap_amd.MhapError, match="0 <= q_lo <= q_hi <= 93"):
            _session(reads, quals, q_lo, q_hi)
    d = api.WeightParams()
    assert (d.q_lo, d.q_hi) == (wref.DEFAULT_Q_LO, wref.DEFAULT_Q_HI)
    with pytest.raises(mhap_amd.MhapError, match="quality bytes"):
        mhap_amd.CorrectSession(tq._fasta(reads), qualities=np.zeros(3, np.uint8))
    # NULL qualities make the call its sibling; NULL weights are the defaults
    f = _fasta(reads[:4], quals[:4])
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        s = api.C.c_void_p()
        args = (api._ptr(f.bases), len(f.bases), api._ptr(f.ids), api._ptr(f.offsets), api._ptr(f.lengths), len(f.ids))
        ms._chk(ms._lib.mhap_correct_begin_weighted(ms._h, args[0], None, *args[1:], None, api.C.byref(s)))
        ms._lib.mhap_correct_free(s)
        ms._chk(ms._lib.mhap_correct_begin_weighted(ms._h, args[0], api._ptr(f.qualities), *args[1:], None, api.C.byref(s)))
        ms._lib.mhap_correct_free(s)


# ---- the unitig consensus ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _consensus(ms, case, seed, q_lo=7, q_hi=20, min_cov=4, values=CLASSES):
    """The weighted consensus of a case against the restatement: counters, bytes, counts and qualities of every unitig."""
    fasta, recs = case.fasta(), case.records()
    quals = _quals(np.random.default_rng(seed), case.reads, values)
    fasta.qualities = np.concatenate(quals)
    with api.GraphSession(case.ids, case.lengths, handle=ms, **tuc.PARAMS) as gs:
        gs.add(recs)
        gs.finish()
        gs.unitigs()
        tables, drafts = gs.unitigs_table, gs.unitig_sequences(fasta)
        with api.ConsensusSession(gs, fasta, band=tuc.BAND, min_cov=min_cov, qualities=fasta.qualities, weights=api.WeightParams(q_lo, q_hi)) as cs:
            cs.add(recs)
            cs.run()
            seqs, stats = cs.sequences(), cs.stats.copy()
            votes = [cs.votes(k).astype(np.int64) for k in range(len(drafts))]
            got_q, hist = cs.quality()
        plain = None
        if q_lo <= min(values) and max(values) < q_hi:                    # the middle class: an unweighted session next to it
            with api.ConsensusSession(gs, fasta, band=tuc.BAND, min_cov=min_cov) as us:
                us.add(recs)
                us.run()
                plain = (us.sequences(), us.stats.copy(), [us.votes(k).astype(np.int64) for k in range(len(drafts))], us.quality())
    want_votes = wref.unitig_votes(case.ids, case.lengths, case.reads, quals, recs, tables, drafts, sg.Params(**tuc.PARAMS), band=tuc.BAND,
                                   q_lo=q_lo, q_hi=q_hi)
    want_q = []
    for k, d in enumerate(drafts):
        rows = np.flatnonzero((votes[k] != want_votes[k]).any(axis=1))
        assert len(rows) == 0, (k, rows[:5], votes[k][rows[:3]], want_votes[k][rows[:3]])
        seq, q, counts = wref.call(d, None, want_votes[k], min_cov, 15, 60, q_lo, q_hi)
        assert seqs[k] == seq and stats[k].tolist() == [len(d), len(seq)] + list(counts) and got_q[k].tolist() == q.tolist(), k
        want_q.append(q)
    assert hist.tolist() == qref.histogram(want_q).tolist()
    if plain is not None:
        assert plain[0] == seqs and plain[1].tolist() == stats.tolist() and all(np.array_equal(2 * u, w) for u, w in zip(plain[2], votes))
        assert all(a.tolist() == b.tolist() for a, b in zip(plain[3][0], got_q)) and plain[3][1].tolist() == hist.tolist()
    return tables, seqs, stats


@pytest.mark.parametrize("L,kind,seed", [(TILE - 1, "sub", 51), (TILE, "del", 52), (TILE + 1, ("ins", 4), 53)], ids=["4095", "4096", "4097"])
def test_consensus_lengths_round_the_tile(ms, L, kind, seed):
    """Drafts of 4 095, 4 096 and 4 097 bases, each next to a unitig of one base."""
    c = tuc.Case(first_id=7)
    c.read(b"A")
    tuc.tile_unitig(c, L, kind, [0, L // 2, TILE - 1, L - 1] if L > TILE else [0, L // 2, L - 1], seed)
    tables, seqs, _ = _consensus(ms, c, seed)
    assert sorted(tables["unitig_len"].tolist()) == [1, L]


@pytest.mark.parametrize("values", [CLASSES, (7, 14, 19)], ids=["every_class", "middle_class"])
def test_consensus_two_tiles_and_a_position(ms, values):
    """A draft of 8 193 bases with insertions of 5 bytes at 0, 4 095, 4 096 and L - 1; with the middle class alone, next to an
    unweighted session."""
    L = 2 * TILE + 1
    c = tuc.Case()
    tuc.tile_unitig(c, L, ("ins", 5), [0, TILE - 1, TILE, L - 1], seed=45)
    tables, _, stats = _consensus(ms, c, 60, values=values)
    assert tables["unitig_len"].tolist() == [L]


def test_consensus_guard_still_reads_the_lowered_cap(ms, monkeypatch):
    """The guard of a weighted run refuses a tile met by more reads than min(MHAP_CONSENSUS_TILE_CAP, 21 845), before any vote."""
    c = tuc.Case()
    tuc.tile_unitig(c, 1500, "sub", [700], seed=46)
    monkeypatch.setenv("MHAP_CONSENSUS_TILE_CAP", "3")
    with pytest.raises(api.MhapError, match="more than 3"):
        _consensus(ms, c, 61)


# ---- the weighted workload on the GPU's own paths ---------------------------------------------------------------------------------------

_counts = {}


def _workload(seed, compare):
    """(wrong bytes of the unweighted session, of the weighted one) on weighted_workload(seed), realigned on the GPU, min_cov 4, the
    default thresholds; compare: the weighted session is the restatement's on the same records."""
    reads, quals, truths, bases, pairs, meta = wref.weighted_workload(seed)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    f = _fasta(reads, quals)
    with mhap_amd.CorrectSession(f, qualities=f.qualities) as ws, mhap_amd.CorrectSession(f) as us:
        ws.add(recs, offsets, ops)
        us.add(recs, offsets, ops)
        wseqs, useqs = ws.finish(4)[0], us.finish(4)[0]
        if compare:
            ref = wref.WeightedConsensus(reads, quals, range(1, len(reads) + 1))
            ref.add(recs, offsets, ops)
            _compare(ws, ref, reads)
    return tuple(sum(int(qref.wrong_bytes(s, t).sum()) for s, t in zip(seqs, truths)) for seqs in (useqs, wseqs))


@pytest.mark.parametrize("seed", twc.SEEDS)
def test_weighted_workload_seed(seed):
    """One seed on the GPU's own paths: both counts are printed; weighting leaves no more wrong bytes on any seed."""
    _counts[seed] = _workload(seed, compare=seed == twc.SEEDS[0])
    print(f"seed {seed}: wrong bytes {_counts[seed][0]} unweighted, {_counts[seed][1]} weighted")
    assert _counts[seed][1] <= _counts[seed][0]


def test_weighted_workload_on_the_gpus_own_paths():
    """Summed over seeds 11 .. 15, the relative reduction of wrong bytes against the unweighted session is at least half of the g
    measured on the CPU restatement (tests/test_weighted_vote_cpu.py).  Measured on an MI355X: 4822 -> 3298, 0.316, the restatement's."""
    for seed in twc.SEEDS:
        if seed not in _counts:
            _counts[seed] = _workload(seed, compare=False)
    plain, weighted = (sum(_counts[s][k] for s in twc.SEEDS) for k in (0, 1))
    print(f"wrong bytes over seeds {twc.SEEDS}: {plain} unweighted, {weighted} weighted, reduction {(plain - weighted) / plain:.3f}")
    assert (plain - weighted) / plain >= twc.G_MEASURED / 2
