"""The per-base stages that came after tests/test_large_offsets_gpu.py past element 2^30 (byte 2^32 of a 4-byte element), 2^31 and 2^32
of their arrays, against the restatements, byte for byte: the base qualities and the quality-weighted votes of the read correction
(qcall_kernel and the QualityWeight instances of the three correction kernels), the variant stage's table of 3 words per position,
its site bytes and its judge, homopolymer compression, and the correction's and the variant stage's reads of the caller's bases.

Part A puts the marks into device tables: fillers that take no record alias one small host buffer and push the offsets, the test
reads carry every record, the restatements run on the test reads alone and a filler's result is written out from the contract
(tests/large_offsets_stages.py).  Part B puts the marks into the caller's bases: one buffer of a little over 2^32 bytes holds the
same small reads at five places (below byte 2^31, across it, between the marks, across 2^32, above it), every copy a read of its own,
and the restatements run on the same reads and ids laid back to back.  Every case first asserts from the layout alone that its
marks lie where it says, so a case that stopped crossing a mark fails, and prints its wall time (EXPERIMENTS.md, "Large offsets").
The cases of part A take about 17 GB of device memory; the one with positions past 2^32 takes 56 GB and is gated on the free device
memory on its own.

Not here: compressed output and maps past element 2^31 (HpcReads downloads both whole, and 2^32 map entries are a 17 GB download),
the correction table at positions past 2^32 (206 GB), the unitig consensus and its qualities (58 B per base of draft: a mark needs
real megabase reads), and FASTQ files of more than 4 GB."""
import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, hpc

import consensus_ref as cref
import hpc_ref
import large_offsets as lo
import large_offsets_stages as los
import quality_ref as qref
import variant_ref as vr
import weighted_vote_ref as wref
from test_large_offsets_gpu import _timed, ms   # noqa: F401  (the device-memory gate and the timer of the cases next door)

pytestmark = pytest.mark.gpu
M30, M31, M32 = lo.MARKS
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _realigned(ms, reads, bases, pairs, meta):
    results, op_offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs, handle=ms)
    recs = cref.quality_records(reads, meta, results)
    assert (recs["score"] > 0).all()
    return reads, recs, op_offsets, ops


@pytest.fixture(scope="module")
def realigned(ms):
    """The reads of part A with their records and paths, realigned on the GPU once."""
    return _realigned(ms, *los.workload())


@pytest.fixture(scope="module")
def b_realigned(ms):
    """The reads of part B, likewise."""
    return _realigned(ms, *los.b_workload())


# ---- A1: the vote table of 12 words per base, weighted, with qualities -----------------------------------------------------------------------

def test_weighted_correction_and_qualities_across_words_2_30_2_31_and_2_32(ms, realigned):
    """The layout of the unweighted case next door, begun weighted with Phred bytes of every weight class in the test reads and in
    the filler buffer: votes, bytes, stats and quality bytes of the test reads against the weighted restatement, the fillers' against
    the lookup, the 94 bins against their sum; then an unweighted session over the same table for its quality bytes."""
    reads, recs, op_offsets, ops = realigned
    n, tlen = len(reads), [len(r) for r in reads]
    lay, at = los.correction_layout(tlen)
    rng = np.random.default_rng(51)
    quals = [rng.choice(los.PHRED, L).astype(np.uint8) for L in tlen]
    filler = ACGT[rng.integers(0, 4, los.FILLER_BASES)]
    filler[rng.integers(0, los.FILLER_BASES, los.FILLER_BASES // 50)] = ord("N")
    filler_q = np.array(los.PHRED, np.uint8)[rng.integers(0, len(los.PHRED), los.FILLER_BASES)]
    assert set(los.weight_class(np.concatenate(quals)).tolist()) == set(los.weight_class(filler_q[:1000]).tolist()) == {0, 1, 2}
    host, ids, offsets, lengths = los.aliased_table(lay, reads, filler)
    host_q = np.concatenate(quals + [filler_q])
    fasta = mhap_amd.FastaData(host, offsets, lengths, ids)
    ref = wref.WeightedConsensus(reads, quals, range(1, n + 1))
    ref.add(recs, op_offsets, ops)
    want = [ref.call_read(k, 4) for k in range(n)]
    assert all(ref.votes[los.VOTE_STRADDLERS[m]].any() for m in lo.MARKS) and sum(w[0] != r for w, r in zip(want, reads)) > 12
    raw = filler.tobytes()
    with _timed("weighted correction and qualities, 2^32 words"):
        with mhap_amd.CorrectSession(fasta, handle=ms, qualities=host_q) as cs:
            assert cs.table_bytes() == 4 * lay.total and (cs.weights.q_lo, cs.weights.q_hi) == (wref.DEFAULT_Q_LO, wref.DEFAULT_Q_HI)
            cs.add(recs, op_offsets, ops)
            for k, i in enumerate(lay.test):
                bad = np.argwhere(cs.votes(i).astype(np.int64) != ref.votes[k])
                assert len(bad) == 0, (k, i, bad[:5].tolist())
            seqs, stats, skipped = cs.finish(4)
            got_q, hist = cs.quality()
    assert skipped == ref.skipped_views == 0
    for k, i in enumerate(lay.test):
        assert seqs[i] == want[k][0] and stats[i].tolist() == list(want[k][1]) and got_q[i].tolist() == want[k][2].tolist(), (k, i)
    fq = los.FillerQualities(los.filler_quality_lookup(True), filler, los.weight_class(filler_q))
    want_hist = qref.histogram([w[2] for w in want])
    for i in lay.fillers:
        L = lay.lengths[i]
        assert stats[i].tolist() == [L, L, 0, 0, 0, L] and seqs[i] == raw[:L] and fq.equals(got_q[i], L), i
        want_hist = want_hist + fq.hist(L)
    assert hist.dtype == np.int64 and hist.tolist() == want_hist.tolist() and int(hist.sum()) > 300_000_000
    del seqs, got_q, fq
    # qcall_kernel<UnitWeight> over the same table
    uref = cref.Consensus(reads, range(1, n + 1))
    uref.add(recs, op_offsets, ops)
    uwant = [qref.call(reads[k], uref.votes[k], 4) for k in range(n)]
    with _timed("unweighted qualities, 2^32 words"):
        with mhap_amd.CorrectSession(fasta, handle=ms) as us:
            us.add(recs, op_offsets, ops)
            seqs, stats, _ = us.finish(4)
            got_q, hist = us.quality()
    for k, i in enumerate(lay.test):
        assert seqs[i] == uwant[k][0] and got_q[i].tolist() == uwant[k][1].tolist(), (k, i)
    fq = los.FillerQualities(los.filler_quality_lookup(False), filler)
    want_hist = qref.histogram([w[1] for w in uwant])
    for i in lay.fillers:
        L = lay.lengths[i]
        assert seqs[i] == raw[:L] and fq.equals(got_q[i], L), i
        want_hist = want_hist + fq.hist(L)
    assert hist.tolist() == want_hist.tolist()


# ---- A2 and A3: the variant stage's table of 3 words per position and its site bytes -----------------------------------------------------------

def _variant_table(ms, realigned, lay, at, what):
    """One session over a layout with fillers against the restatement on the test reads: the counters of every test read, the
    counts, the rows, offsets and site list, and keep and tallies of every record."""
    reads, recs, op_offsets, ops = realigned
    n, P = len(reads), los.VARIANT_PARAMS
    v = vr.Variants(reads, range(1, n + 1), **P)
    v.add(recs, op_offsets, ops)
    counts = v.finish()
    los.sites_round(v, at)                                                  # sites on both sides of every mark's position
    assert counts[2] > 0
    want_keep, want_tallies = v.apply(recs, op_offsets, ops)
    assert set(want_keep.tolist()) == {0, 1} and (want_tallies.sum(axis=0) > 0).all()
    filler = ACGT[np.random.default_rng(52).integers(0, 4, los.FILLER_BASES)]
    host, ids, offsets, lengths = los.aliased_table(lay, reads, filler)
    ecounts, erows, eoffsets, esites = los.variant_with_fillers(lay, v, counts, P)
    with _timed(what):
        with api.VariantSession(mhap_amd.FastaData(host, offsets, lengths, ids), handle=ms, **P) as vs:
            for q0 in range(0, len(recs), 43):
                q1 = min(q0 + 43, len(recs))
                vs.add(recs[q0:q1], op_offsets[q0:q1 + 1] - op_offsets[q0], ops[op_offsets[q0]:op_offsets[q1]])
            for k, i in enumerate(lay.test):
                assert vs.votes(i).astype(np.int64).tolist() == v.votes(k).tolist(), (k, i)
            got = vs.finish()
            assert [got[k] for k in api.VARIANT_COUNTS] == ecounts
            rows, soff, sites = vs.table()
            assert rows.tobytes() == erows.tobytes() and soff.tobytes() == eoffsets.tobytes() and sites.tobytes() == esites.tobytes()
            keep, tallies = vs.apply(recs, op_offsets, ops)
            assert keep.tobytes() == want_keep.tobytes() and tallies.tobytes() == want_tallies.tobytes()


def test_variant_sites_across_table_words_2_30_2_31_and_2_32(ms, realigned):
    """The marks in planes 0, 1 and 2 of a straddler each; 17.2 GB of votes and 1.4 GB of site bytes."""
    lay, at = los.variant_layout([len(r) for r in realigned[0]])
    _variant_table(ms, realigned, lay, at, "variant sites, 2^32 table words")


def test_variant_sites_across_positions_2_31_and_2_32(ms, realigned):
    """A little over 2^32 positions: the site bytes and read_pos reach 2^31 and 2^32, the table's words 3 * 2^32.  Records pair reads on
    opposite sides of each mark in both orders and on both strands, so the judge reads site_a below and site_b above a mark, and
    the reverse."""
    import torch
    lay, at = los.site_layout([len(r) for r in realigned[0]])
    need = 13 * lay.total + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{free >> 30} GiB of device memory are free; this case needs {need / 1e9:.0f} GB (51.5 GB of votes, 4.3 GB of site bytes)")
    for mark in los.SITE_MARKS:
        assert los.records_across(lay, realigned[1], mark) == {(True, 0), (True, 1), (False, 0), (False, 1)}, mark
    _variant_table(ms, realigned, lay, at, "variant sites, 2^32 positions")


# ---- B: the caller's bases, a little over 2^32 bytes -------------------------------------------------------------------------------------------

@pytest.fixture
def big_buffer():     # (function scope: the host memory goes back before the next case takes its own)
    return np.zeros(los.BIG_SIZE, np.uint8)


def _places(b_realigned, big):
    """(places, the session's table over the big buffer, records, op_offsets, ops) with the leading assertions of the B cases."""
    reads, recs, op_offsets, ops = b_realigned
    P = los.Places(reads)
    assert len(big) >= P.size and {int(x) for x in recs["to_rc"]} == {0, 1}
    P.lay(big)
    big_recs, boff, bops, where = P.records(recs, op_offsets, ops)
    P.records_across(big_recs, where)
    crossing = {m for r in range(len(P.ids)) for m in (M31, M32) if P.offsets[r] < m < P.offsets[r] + P.lengths[r]}
    assert crossing == {M31, M32}
    return P, mhap_amd.FastaData(big, P.offsets, P.lengths, P.ids), big_recs, boff, bops


def test_weighted_correction_with_reads_across_bytes_2_31_and_2_32(ms, b_realigned, big_buffer):
    """bases[at], quals[at], own[t] and own_weight(first + t) above both marks in the three QualityWeight kernels: votes, bytes, stats
    and quality bytes of every placed read."""
    P, fasta, recs, op_offsets, ops = _places(b_realigned, big_buffer)
    rng = np.random.default_rng(53)
    quals = [rng.choice(los.PHRED, len(r)).astype(np.uint8) for r in P.reads]
    big_q = np.zeros(len(big_buffer), np.uint8)
    P.lay(big_q, np.concatenate(quals))
    ref = wref.WeightedConsensus(P.small_reads, quals * 5, P.ids)
    ref.add(recs, op_offsets, ops)
    want = [ref.call_read(r, 4) for r in range(len(P.ids))]
    assert sum(w[0] != r for w, r in zip(want, P.small_reads)) > len(P.ids) // 2
    with _timed(f"weighted correction, {len(P.ids)} reads in 2^32 bytes of bases"):
        with mhap_amd.CorrectSession(fasta, handle=ms, qualities=big_q) as cs:
            cs.add(recs, op_offsets, ops)
            for r in range(len(P.ids)):
                bad = np.argwhere(cs.votes(r).astype(np.int64) != ref.votes[r])
                assert len(bad) == 0, (r, bad[:5].tolist())
            seqs, stats, skipped = cs.finish(4)
            got_q, hist = cs.quality()
    assert skipped == ref.skipped_views == 0
    for r in range(len(P.ids)):
        assert seqs[r] == want[r][0] and stats[r].tolist() == list(want[r][1]) and got_q[r].tolist() == want[r][2].tolist(), r
    assert hist.tolist() == qref.histogram([w[2] for w in want]).tolist()


def test_variant_sites_with_reads_across_bytes_2_31_and_2_32(ms, b_realigned, big_buffer):
    """The walk's and the judge's bases[a_off + i] and bases[b_off + jb] on opposite sides of the marks: votes, counts, table, apply."""
    P, fasta, recs, op_offsets, ops = _places(b_realigned, big_buffer)
    v = vr.Variants(P.small_reads, P.ids, **los.VARIANT_PARAMS)
    v.add(recs, op_offsets, ops)
    counts = v.finish()
    want_keep, want_tallies = v.apply(recs, op_offsets, ops)
    assert counts[2] > 0 and (want_tallies[:, 0] > 0).any()
    with _timed(f"variant sites, {len(P.ids)} reads in 2^32 bytes of bases"):
        with api.VariantSession(fasta, handle=ms, **los.VARIANT_PARAMS) as vs:
            vs.add(recs, op_offsets, ops)
            for r in range(len(P.ids)):
                assert vs.votes(r).astype(np.int64).tolist() == v.votes(r).tolist(), r
            got = vs.finish()
            assert [got[k] for k in api.VARIANT_COUNTS] == counts
            rows, soff, sites = vs.table()
            assert rows.tobytes() == v.rows.tobytes() and soff.tobytes() == v.offsets.tobytes() and sites.tobytes() == v.sites.tobytes()
            keep, tallies = vs.apply(recs, op_offsets, ops)
            assert keep.tobytes() == want_keep.tobytes() and tallies.tobytes() == want_tallies.tobytes()


def _same_compression(hp, want):
    n = len(want["clen"])
    assert hp.counts == want["counts"]
    assert hp.fasta.lengths.tobytes() == want["clen"].tobytes() and hp.fasta.offsets.tobytes() == want["coff"][:n].tobytes()
    assert hp.fasta.bases.tobytes() == want["cbases"].tobytes() and hp.starts.dtype == np.int32 and hp.starts.tobytes() == want["starts"].tobytes()


def test_homopolymer_compression_with_reads_across_bytes_2_31_and_2_32(ms, big_buffer):
    """One table over the buffer: blocks of crafted reads at the five places, reads of zeros that share bytes, and a read of 2^31 - 9
    bases whose windows are two of the blocks; the default groups and groups of 2^30 give the same; records between reads on
    opposite sides of the marks expand as the restatement says; then the same table with a head on each mark instead of a run."""
    T = api.HPC_TILE
    H = los.HpcTable(T)                                                      # (the layout's assertions run in the constructor)
    big = big_buffer
    H.lay(big)
    for mark in (M31, M32):                                                  # the mark inside a run
        assert big[mark - 2] == big[mark - 1] == big[mark] == big[mark + 1] != 0
    fasta = mhap_amd.FastaData(big, H.offsets, H.lengths, H.ids)
    want = H.expected(big)
    fill = lo.LONGEST - 2 * los.HPC_W
    assert want["counts"]["longest_run"] == fill and want["counts"]["raw_bases"] > 16 * los.HPC_GROUP_DEFAULT
    assert int(want["starts"][want["coff"][H.long] + H.long + want["clen"][H.long]]) == lo.LONGEST and want["clen"][H.long] > 5000
    below, between, above = H.rows_of(0), H.rows_of(2), H.rows_of(4)
    pairs = [(a, b) for a, b in zip(below, above)] + [(b, a) for a, b in zip(between, above)] + [(H.long, above[0]), (above[1], H.long)]
    pairs += [(a, b) for a, b in zip(H.rows_of(1), H.rows_of(3))]
    recs = los.hpc_records(np.random.default_rng(54), want, pairs, 400)
    with _timed("homopolymer compression, 2^32 bytes of bases, three calls"):
        with hpc.compress(fasta, handle=ms) as hp:
            _same_compression(hp, want)
            assert hp.expand(recs).tobytes() == hpc_ref.expand(recs, want).tobytes()
        with hpc.compress(fasta, handle=ms, group_bases=1 << 30) as hp:
            _same_compression(hp, want)
        for mark in (M31, M32):                                              # the second copy: a head on the mark
            big[mark] = ord("G")
            assert big[mark - 1] != big[mark] != big[mark + 1]
        want2 = H.expected(big)
        assert want2["counts"]["compressed_bases"] > want["counts"]["compressed_bases"]
        with hpc.compress(fasta, handle=ms) as hp:
            _same_compression(hp, want2)
