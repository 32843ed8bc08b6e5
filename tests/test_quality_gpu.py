"""Base qualities on the GPU (mhap_correct_quality, mhap_consensus_quality; vote_common.hpp's decide_quality) against their
restatement (tests/quality_ref.py), byte for byte, the histogram included: the correction over crafted piles planted at the edges of
the call kernel's 256 positions, the unitig consensus over drafts round its tile of 4 096, and the quality workload."""
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
import test_unitig_consensus_gpu as tuc  # noqa: E402
import unitig_ref as ur  # noqa: E402
from align_ref import rc_bytes  # noqa: E402
from mhap_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

OP_I, OP_D, OP_EQ, OP_X = cref.OP_I, cref.OP_D, cref.OP_EQ, cref.OP_X
TILE = tuc.TILE


def _fasta(reads):
    lengths = np.array([len(r) for r in reads], np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64)
    return mhap_amd.FastaData(np.frombuffer(b"".join(reads), np.uint8), offsets, lengths, np.arange(1, len(reads) + 1))


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).tolist())


def _other(c):
    return next(x for x in b"ACGT" if x != c)


def _edited(target, edits):
    """(evidence read, runs): the target with `edits` {position: ("X",) | ("D",) | ("I", bytes after it)} and the path that says so,
    the target as read A.  A substitution on the first or the last position is spelled '=' (a path begins and ends with '=', and the
    vote reads the bytes, not the code), so a plant can reach L - 1; nothing else can stand there."""
    L, e, cols = len(target), bytearray(), []
    for t, c in enumerate(target):
        kind = edits.get(t, (None,))
        if kind[0] == "D":
            cols.append(OP_I)                                           # consumes the target only
        elif kind[0] == "X":
            cols.append(OP_EQ if t in (0, L - 1) else OP_X)
            e.append(_other(c))
        else:
            cols.append(OP_EQ)
            e.append(c)
        if kind[0] == "I":
            cols += [OP_D] * len(kind[1])
            e += kind[1]
    runs, k = [], 0
    while k < len(cols):
        n = 1
        while k + n < len(cols) and cols[k + n] == cols[k]:
            n += 1
        runs.append(n << 4 | cols[k])
        k += n
    return bytes(e), hp.check_canonical(runs)


KINDS = [("X",), ("D",), ("I", b"T"), ("I", b"TACG"), ("I", b"TACGA")]     # a substitution, a deletion, insertions of 1, 4 and 5


def _pile():
    """Reads, records and runs: five targets of 513 bases, target k with KINDS[k], [k + 1], [k + 2] at 255, 256 and L - 2 (L - 1 for
    the substitution), each under five evidence reads with the plants and one without, every other one stored reverse-complemented
    (to_rc); a target of 257 bases with Ns; two reads of 2 bases under four views; and reads of 1, 2, 255, 256, 257 and 513 bases
    that no record touches."""
    rng = np.random.default_rng(21)
    reads, recs, ops, off = [], [], [], [0]

    def add(t_index, edits, to_rc):
        e, runs = _edited(reads[t_index], edits)
        reads.append(rc_bytes(e) if to_rc else e)
        recs.append(hp.record_for(t_index + 1, len(reads), reads[t_index], e, 0, 0, runs, to_rc))
        ops.extend(runs)
        off.append(len(ops))

    L = 513
    for k in range(5):
        t = len(reads)
        reads.append(_rand(rng, L))
        last = KINDS[(k + 2) % 5]
        edits = {255: KINDS[k], 256: KINDS[(k + 1) % 5], (L - 1 if last[0] == "X" else L - 2): last}
        for c in range(6):
            add(t, edits if c < 5 else {}, c % 2)
    t = len(reads)
    tn = bytearray(_rand(rng, 257))
    tn[10] = tn[20] = tn[256] = ord("N")
    reads.append(bytes(tn))
    for c in range(5):
        e = bytearray(tn)
        e[10] = ord("G")                                                # N outvoted; N under N; an N in the evidence; N kept at L - 1
        e[30] = ord("N")
        reads.append(rc_bytes(bytes(e)) if c % 2 else bytes(e))
        recs.append(hp.record_for(t + 1, len(reads), bytes(tn), bytes(e), 0, 0, [257 << 4 | OP_EQ], c % 2))
        ops.append(257 << 4 | OP_EQ)
        off.append(len(ops))
    t = len(reads)
    reads += [b"GA", b"GA"]
    for _ in range(4):
        recs.append(hp.record_for(t + 1, t + 2, b"GA", b"GA", 0, 0, [2 << 4 | OP_EQ], 0))
        ops.append(2 << 4 | OP_EQ)
        off.append(len(ops))
    # an insertion that only 2 of 6 views want (not called: the stop margin of the base byte is the smaller), and one that 3 of 3
    # want under min_cov 4 (not called for lack of span: quality 0), at 255 and at 256
    for n_with, n_all in ((2, 6), (3, 3)):
        t = len(reads)
        reads.append(_rand(rng, 300))
        for c in range(n_all):
            add(t, {255: ("I", b"G"), 256: ("I", b"CA")} if c < n_with else {}, c % 2)
    untouched = len(reads)
    reads += [_rand(rng, n) for n in (1, 2, 255, 256, 257, 513)]
    return reads, np.concatenate(recs), np.array(off, np.int64), np.array(ops, np.uint32), untouched


@pytest.fixture(scope="module")
def pile():
    reads, recs, off, ops, untouched = _pile()
    ref = cref.Consensus(reads, range(1, len(reads) + 1))
    ref.add(recs, off, ops)
    return reads, recs, off, ops, untouched, ref


def _expect(reads, ref, min_cov, per_vote, cap):
    out = [qref.call(reads[r], ref.votes[r], min_cov, per_vote, cap) for r in range(len(reads))]
    return [s for s, _ in out], [q for _, q in out]


def _same(got, hist, seqs, wseqs, wquals):
    assert [bytes(s) for s in seqs] == wseqs
    for r, (g, w) in enumerate(zip(got, wquals)):
        assert g.dtype == np.uint8 and g.tolist() == w.tolist(), (r, np.flatnonzero(np.asarray(g) != w)[:5] if len(g) == len(w) else (len(g), len(w)))
    assert hist.dtype == np.int64 and hist.tolist() == qref.histogram(wquals).tolist()


def test_correction_qualities_equal_the_restatement(pile):
    reads, recs, off, ops, untouched, ref = pile
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        cs.add(recs, off, ops)
        seqs, stats, _ = cs.finish(4)
        quals, hist = cs.quality()
        wseqs, wquals = _expect(reads, ref, 4, qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP)
        _same(quals, hist, seqs, wseqs, wquals)
        # the plants were called, 4 bytes of the 5-byte insertion: {n_sub, n_del, n_ins} of the five targets
        assert stats[0:35:7, 2:5].tolist() == [[1, 1, 1], [0, 1, 1 + 4], [0, 0, 1 + 4 + 4], [1, 0, 4 + 4], [1, 1, 4]]
        # a read no record touches: every position low, margin 1
        for r in range(untouched, len(reads)):
            assert quals[r].tolist() == [qref.q_of(1)] * len(reads[r])
        # the Ns: outvoted at 10, kept with the fixed 0 at 20 and at L - 1
        tn = 35
        assert seqs[tn][10:11] == b"G" and quals[tn][10] > 0 and seqs[tn][20:21] == b"N" and quals[tn][20] == 0 and quals[tn][256] == 0
        # an insertion minority lowers the base byte through the stop margin; a majority without span takes it to 0
        assert quals[43][254:258].tolist() == [qref.q_of(m) for m in (7, 3, 3, 7)] and quals[50][254:258].tolist() == [qref.q_of(m) for m in (4, -2, -2, 4)]
        # a second call with other parameters after the one finish: the cap binds, the slope of one tenth, the widest cap
        for per_vote, cap in ((1000, 60), (1, 60), (7, 93), (30, 1), (30, 60)):
            q2, h2 = cs.quality(per_vote, cap)
            _same(q2, h2, seqs, *_expect(reads, ref, 4, per_vote, cap))
        h = cs.quality(1000, 60)[1]
        assert h[60] > 1000 and h[1:60].sum() == 0 and h[61:].sum() == 0     # at 100 per vote every positive margin is at the cap
        # a finish with another min_cov, then quality: the session remembers it
        for min_cov in (1, 7):
            seqs, _, _ = cs.finish(min_cov)
            q3, h3 = cs.quality()
            _same(q3, h3, seqs, *_expect(reads, ref, min_cov, qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP))
        # the raw entry point: NULL parameters are the defaults, the histogram may be left out
        flat = np.zeros(int(cs.offsets[-1]), np.uint8)
        cs._ms._chk(cs._lib.mhap_correct_quality(cs._s, None, flat.ctypes.data, None))
        assert flat.tolist() == np.concatenate(q3).tolist()


def test_correction_quality_is_refused(pile):
    reads, recs, off, ops, _, _ = pile
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        cs.add(recs, off, ops)
        with pytest.raises(mhap_amd.MhapError, match="no mhap_correct_finish has completed"):
            cs.quality()
        cs.finish(4)
        for per_vote, cap in ((0, 60), (1001, 60), (30, 0), (30, 94), (-5, 60)):
            with pytest.raises(mhap_amd.MhapError, match="per_vote must be 1 .. 1000 and cap 1 .. 93"):
                cs.quality(per_vote, cap)
        cs.quality(1000, 93)
        cs.add(recs[:1], off[:2], ops[:off[1]])                         # the offsets of that finish are not this table's any more
        with pytest.raises(mhap_amd.MhapError, match="since the last mhap_correct_finish"):
            cs.quality()
        cs.finish(4)
        cs.quality()
    with mhap_amd.CorrectSession(_fasta([b"", b""])) as cs:          # nothing to write
        cs.finish(4)
        quals, hist = cs.quality()
        assert [len(q) for q in quals] == [0, 0] and hist.sum() == 0


def test_quality_workload_on_the_gpus_own_paths():
    """quality_workload(7) realigned on the GPU: the qualities are the restatement's on the same records, and the wrong-byte share
    at or above the median quality is below one quarter of the share below it."""
    reads, truths, bases, pairs, meta = cref.quality_workload(7)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    ref = cref.Consensus(reads, range(1, len(reads) + 1))
    ref.add(recs, offsets, ops)
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        cs.add(recs, offsets, ops)
        seqs, _, _ = cs.finish(4)
        quals, hist = cs.quality()
    _same(quals, hist, seqs, *_expect(reads, ref, 4, qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP))
    med, (w_lo, n_lo), (w_hi, n_hi) = qref.ranking(quals, [qref.wrong_bytes(s, t) for s, t in zip(seqs, truths)])
    print(f"median {med}: below {w_lo} wrong of {n_lo}, at or above {w_hi} wrong of {n_hi}")
    assert n_lo > 0 and n_hi > 0 and w_hi / n_hi < 0.25 * (w_lo / n_lo)


# ---- the unitig consensus ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _consensus(ms, case, params=((qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP),), min_cov=4, clean=False):
    """Run the consensus of a case and compare the qualities of every (per_vote, cap) with the restatement on the session's own
    counters and drafts (tests/test_unitig_consensus_gpu.py pins those); returns (sequences, qualities of the first, stats, tables)."""
    fasta, recs = case.fasta(), case.records()
    with api.GraphSession(case.ids, case.lengths, handle=ms, **tuc.PARAMS) as gs:
        gs.add(recs)
        gs.finish()
        gs.clean() if clean else gs.unitigs()
        drafts = gs.unitig_sequences(fasta)
        with api.ConsensusSession(gs, fasta, band=tuc.BAND, min_cov=min_cov) as cs:
            cs.add(recs)
            cs.run()
            seqs, first = cs.sequences(), None
            votes = [cs.votes(k).astype(np.int64) for k in range(len(drafts))]
            for per_vote, cap in params:
                quals, hist = cs.quality(per_vote, cap)
                want = [qref.call(drafts[k], votes[k], min_cov, per_vote, cap) for k in range(len(drafts))]
                _same(quals, hist, seqs, [s for s, _ in want], [q for _, q in want])
                first = first or quals
            return seqs, first, cs.stats.copy(), gs.unitigs_table


@pytest.mark.parametrize("kind", ["sub", "del", ("ins", 1), ("ins", 4), ("ins", 5)], ids=lambda k: k if isinstance(k, str) else f"ins{k[1]}")
def test_consensus_two_tiles_and_a_position(ms, kind):
    """A draft of 8 193 bases with the plant at 0, 4 095, 4 096 and L - 1."""
    L = 2 * TILE + 1
    c = tuc.Case()
    tuc.tile_unitig(c, L, kind, [0, TILE - 1, TILE, L - 1], seed=40 + (kind[1] if isinstance(kind, tuple) else len(kind)))
    seqs, quals, stats, tables = _consensus(ms, c, params=((qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP), (1000, 93), (1, 60), (30, 60)))
    assert tables["unitig_len"].tolist() == [L] and stats[0, {"sub": 2, "del": 3}.get(kind, 4)] >= 2
    assert len(quals[0]) == len(seqs[0]) == stats[0, 1] and int(quals[0].min()) < int(quals[0].max())


@pytest.mark.parametrize("L,kind,seed", [(TILE - 1, "sub", 51), (TILE, "del", 52), (TILE + 1, ("ins", 4), 53)], ids=["4095", "4096", "4097"])
def test_consensus_lengths_round_the_tile(ms, L, kind, seed):
    """Drafts of 4 095, 4 096 and 4 097 bases, each next to a unitig of one base."""
    c = tuc.Case(first_id=7)
    c.read(b"A")
    tuc.tile_unitig(c, L, kind, [0, L // 2, TILE - 1, L - 1] if L > TILE else [0, L // 2, L - 1], seed)
    seqs, quals, stats, tables = _consensus(ms, c)
    assert sorted(tables["unitig_len"].tolist()) == [1, L]
    k1 = tables["unitig_len"].tolist().index(1)
    assert seqs[k1] == b"A" and quals[k1].tolist() == [qref.q_of(2)]                  # the member votes on its own draft: s = 2 of n = 2


def test_consensus_circular_unitig(ms):
    C, n, step, ln = 2400, 6, 400, 800
    g = ur.draw_bases(C, 71)
    gg = g + g
    c = tuc.Case()
    m = [c.read(gg[i * step:i * step + ln]) for i in range(n)]
    for i in range(n):
        c.rec(tuc.sg.dove(m[i], m[(i + 1) % n], step, read_len=ln))
    for s in (2200, 2250, 2290, 2330):
        x = c.read(gg[s:s + 450])
        c.rec(tuc.sg.record(x, m[5], 0, 449, 450, s - 2000, s - 2000 + 449, ln, 0))
    seqs, quals, _, tables = _consensus(ms, c, min_cov=2)
    assert tables["circular"].tolist() == [1] and seqs[0] == g and len(set(quals[0].tolist())) > 2


def test_consensus_three_unitigs(ms):
    """Three unitigs: the offsets of the quality bytes cross unitig boundaries."""
    c, _ = tuc.tip_case()
    seqs, quals, _, tables = _consensus(ms, c, params=((qref.DEFAULT_PER_VOTE, qref.DEFAULT_CAP), (7, 93)))
    assert len(tables["unitig_len"]) == 3 and [len(q) for q in quals] == [len(s) for s in seqs]
    _consensus(ms, c, clean=True)


def test_consensus_quality_is_refused(ms, monkeypatch):
    g = ur.draw_bases(700, 91)
    c = tuc.Case()
    m = c.cut(g, 0, 700, 0)
    for k in range(3):
        c.placed(c.cut(g, 50 + 10 * k, 500 + 10 * k, 0), m)
    fasta = c.fasta()
    with api.GraphSession(c.ids, c.lengths, handle=ms, **tuc.PARAMS) as gs:
        gs.add(c.records())
        gs.finish()
        gs.unitigs()
        with api.ConsensusSession(gs, fasta, band=tuc.BAND) as cs:
            cs.add(c.records())
            with pytest.raises(api.MhapError, match="no mhap_consensus_run has completed"):
                cs.quality()
            cs.run()
            assert cs.quality()[1].sum() == cs.info()[3]
            for per_vote, cap in ((0, 60), (1001, 60), (30, 0), (30, 94)):
                with pytest.raises(api.MhapError, match="per_vote must be 1 .. 1000 and cap 1 .. 93"):
                    cs.quality(per_vote, cap)
            monkeypatch.setenv("MHAP_CONSENSUS_TILE_CAP", "3")
            with pytest.raises(api.MhapError, match="more than 3"):
                cs.run()
            with pytest.raises(api.MhapError, match="no mhap_consensus_run has completed"):   # after a run the guard refused
                cs.quality()
            monkeypatch.delenv("MHAP_CONSENSUS_TILE_CAP")
            cs.run()
            cs.quality()
            gs.unitigs()                                                  # the graph session has moved on
            with pytest.raises(api.MhapError, match="since mhap_consensus_begin"):
                cs.quality()
