"""The per-base stages behind --realign past element 2^30 (byte 2^32 of a 4-byte element), 2^31 and 2^32 of their device arrays,
against the restatements: the difference array of the trimming and the repeat marking, the vote table of the read correction, the
caller's bases under the three aligners, the pair k-mer statistics and the spelling, and the trace buffer of the path pass.

Fillers that take no record push the offsets (tests/large_offsets.py); small test reads carry every record and lie round the marks;
the restatements run on the test reads alone and a filler's result is written out from the contract.  Every case first asserts
that its marks fall inside a test read's own range (or, for the trace, that the documented lower bound of the words in front of
the last copy exceeds 2^32), so a case that stopped crossing a mark fails.  Each case needs about 20 GB of device memory and
prints its wall time (EXPERIMENTS.md, "Large offsets").

Not here: the unitig consensus's draft (58 B per base: a mark needs real megabase reads), the k-mer counter's and evaluator's stores
(ingest groups bound their offsets), spelled output past 2^32 bytes (a 4-GiB download), and `x * G` inside one pair's trace, which
passes 2^31 only for a pair of 8 GiB of trace that no restatement follows."""
import time

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api

import align_banded_ref as bref
import align_paths_ref as pref
import align_ref
import consensus_ref as cref
import ksim_ref
import large_offsets as lo
import repeat_ref
import string_graph_ref as sg
import trim_cases as tc
import trim_ref
import unitig_ref as ur

pytestmark = pytest.mark.gpu
M30, M31, M32 = lo.MARKS


@pytest.fixture(scope="module")
def ms():
    import torch
    total = torch.cuda.get_device_properties(0).total_memory
    if total < lo.MIN_DEVICE_BYTES:
        pytest.skip(f"the device has {total >> 30} GiB in total; these cases need about 20 GB each and run from 48 GiB")
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


class _timed:
    def __init__(self, what):
        self.what = what

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        print(f"large offsets: {self.what}: {time.perf_counter() - self.t0:.2f} s")


# ---- cases 1 and 2: the difference array, a little over 2^32 slots -------------------------------------------------------------------------
PILE_LENGTHS = [700, 4097, 6000, 3000, 20, 6001, 4096, 5999, 1500, 2500]
PILE_STRADDLERS = {M30: 2, M31: 5, M32: 7}
LONELY = 4            # no record names it
PARTNERS = (1, 6)     # the other read of the crafted records


def _pile_table():
    """(layout, {mark: (test read, slot)}, ids of every entry, ids and lengths of the test reads)."""
    lay = lo.place(PILE_LENGTHS, PILE_STRADDLERS, lo.pile_slots, 1 << 28)
    found = lay.marks_inside_test_reads(lo.MARKS, lo.pile_used, 2600)
    assert lay.total > M32 and not lay.filler[0] and not lay.filler[-1] and max(lay.lengths[i] for i in lay.fillers) <= 1 << 28
    assert [found[m][0] for m in lo.MARKS] == [PILE_STRADDLERS[m] for m in lo.MARKS]
    ids = np.arange(1000, 1000 + len(lay), dtype=np.int64)
    return lay, found, ids, ids[lay.test], np.array(PILE_LENGTHS, np.int32)


def _pile_records(rng, found, tids, shapes, noise):
    """Crafted records on every straddler — shapes = [(first, last + 1, depth)] relative to the mark's position in the read — with
    random intervals on a partner, and `noise` random records among the other test reads but LONELY."""
    out = []
    for mark in lo.MARKS:
        k, p = found[mark]
        for u, (a, b, depth) in enumerate(shapes):
            for d in range(depth):
                q = PARTNERS[(u + d) % 2]
                n = int(rng.integers(200, 1500))
                t = int(rng.integers(0, PILE_LENGTHS[q] - n))
                rc = int(rng.integers(0, 2))
                if (u + d) % 3:
                    out.append(tc.rec(int(tids[k]), int(tids[q]), p + a, p + b - 1, PILE_LENGTHS[k], t, t + n - 1, PILE_LENGTHS[q], rc))
                else:
                    out.append(tc.rec(int(tids[q]), int(tids[k]), t, t + n - 1, PILE_LENGTHS[q], p + a, p + b - 1, PILE_LENGTHS[k], rc))
    ok = [k for k in range(len(PILE_LENGTHS)) if k != LONELY and k not in PILE_STRADDLERS.values()]
    for _ in range(noise):
        x, y = rng.choice(ok, 2, replace=False).tolist()
        iv = []
        for L in (PILE_LENGTHS[x], PILE_LENGTHS[y]):
            n1 = int(rng.integers(1, min(L, 1200) + 1))
            s = int(rng.integers(0, L - n1 + 1))
            iv += [s, s + n1 - 1]
        out.append(tc.rec(int(tids[x]), int(tids[y]), iv[0], iv[1], PILE_LENGTHS[x], iv[2], iv[3], PILE_LENGTHS[y], int(rng.integers(0, 2)),
                          float(rng.choice([0.0, 0.4, 0.7, 0.9]))))
    recs = tc.recs(out)
    return recs[rng.permutation(len(recs))]


def test_trimming_across_slots_2_30_2_31_and_2_32(ms):
    """One session of a little over 2^32 slots (17.2 GB).  Every straddler has a run of coverage 2 on each side of its mark and one
    record across it; read LONELY is deleted; split adds."""
    lay, found, ids, tids, tlen = _pile_table()
    P = trim_ref.params(min_cov=2, end_clip=20, min_span=100, min_identity=0.5)
    records = _pile_records(np.random.default_rng(31), found, tids, [(-2400, -400, 2), (400, 2400, 2), (-150, 150, 1)], 60)
    rows_s, flags_s, counts_s, cov = trim_ref.trim(tids, tlen, records, P)
    for mark in lo.MARKS:     # what the case is for, from the restatement: runs end in front of the mark's slot and begin behind it
        k, p = found[mark]
        runs = trim_ref.runs_of(cov[k], P["min_cov"])
        assert any(e <= p for _, e in runs) and any(s > p for s, _ in runs) and cov[k][p] == 1 and flags_s[k] & trim_ref.GAPPED
    assert flags_s[LONELY] == trim_ref.DELETED
    erows, eflags, ecounts = lo.trim_with_fillers(lay, rows_s, flags_s, counts_s)
    with _timed("trimming, 2^32 slots"):
        with api.TrimSession(ids, np.array(lay.lengths, np.int32), handle=ms, **P) as ts:
            for q0 in range(0, len(records), 37):
                ts.add(records[q0:q0 + 37])
            counts = ts.finish()
            rows, flags = ts.table()
            assert counts == ecounts
            assert rows.tobytes() == erows.tobytes() and flags.tobytes() == eflags.tobytes()
            for k, i in enumerate(lay.test):
                assert ts.coverage(i).tobytes() == cov[k].astype(np.int32).tobytes(), (k, i)
            out, keep = ts.apply(records)
            eout, ekeep = trim_ref.apply(ids, erows, eflags, records, P)
            assert keep.tobytes() == ekeep.tobytes() and out.tobytes() == eout.tobytes() and 0 < int(keep.sum()) < len(records)


def test_repeat_marking_across_slots_2_30_2_31_and_2_32(ms):
    """The same table.  Every straddler has an interval of depth 3 that begins in front of its mark and ends behind it, and one on
    each side; max_cov 2."""
    lay, found, ids, tids, tlen = _pile_table()
    P = repeat_ref.params(max_cov=2, min_run=50, min_unique=100, min_identity=0.5)
    records = _pile_records(np.random.default_rng(32), found, tids, [(-700, 700, 3), (-2400, -1500, 3), (1500, 2400, 3)], 60)
    m = repeat_ref.mark(tids, tlen, records, P)
    for mark in lo.MARKS:
        k, p = found[mark]
        iv = m["intervals"][m["offsets"][k]:m["offsets"][k + 1]].tolist()
        assert any(a < p < b for a, b in iv) and any(b < p for _, b in iv) and any(a > p for a, _ in iv), (mark, p, iv)
    e = lo.repeat_with_fillers(lay, m)
    with _timed("repeat marking, 2^32 slots"):
        with api.RepeatSession(ids, np.array(lay.lengths, np.int32), handle=ms, **P) as rs:
            for q0 in range(0, len(records), 41):
                rs.add(records[q0:q0 + 41])
            counts = rs.finish()
            rows, flags, offsets, iv = rs.table()
            assert counts == e["counts"]
            assert offsets.tobytes() == e["offsets"].tobytes() and iv.tobytes() == e["intervals"].tobytes()
            assert rows.tobytes() == e["rows"].tobytes() and flags.tobytes() == e["flags"].tobytes()
            assert rs.histogram().tobytes() == e["hist"].tobytes()
            keep, unique = rs.apply(records)
            ekeep, eunique = repeat_ref.apply(ids, e["offsets"], e["intervals"], records, P)
            assert keep.tobytes() == ekeep.tobytes() and unique.tobytes() == eunique.tobytes() and 0 < int(keep.sum()) < len(records)


# ---- case 3: the longest read a table takes -----------------------------------------------------------------------------------------------
WINDOW, PARTNER_LEN = 20000, 3000


def _longest_records(seed):
    """Folded and real records of a read of 2^31 - 9 bases: runs in its first and its last 20 000 positions, among them the very
    first and the very last position and the windows' inner edges, stretches of depth 2 between some of them, and a partner behind it."""
    rng = np.random.default_rng(seed)
    W = WINDOW
    runs = [(lo.A_ID, 0, 900, 4), (lo.A_ID, 5000, 9000, 4), (lo.A_ID, W - 700, W, 4), (lo.B_ID, 0, 600, 4), (lo.B_ID, 7000, 11000, 4),
            (lo.B_ID, 12000, 15000, 6), (lo.B_ID, W - 1200, W, 4), (lo.A_ID, 800, 5200, 2), (lo.B_ID, 11000, 12000, 2), (lo.A_ID, 12000, 12040, 6)]
    folded = tc.recs(lo.window_records(rng, W, PARTNER_LEN, runs, tc.rec))
    folded["score"][::7] = 0.4     # below the min_identity of these cases: a run's depth above is one less here and there (its records follow each other)
    real = lo.unfold(folded, lo.LONGEST, W)
    assert int(real["a2"].max()) == lo.LONGEST - 1 or int(real["b2"].max()) == lo.LONGEST - 1
    return folded, real


def test_trimming_a_read_of_2_31_minus_9_bases(ms):
    folded, real = _longest_records(33)
    ids, lengths = np.array([lo.A_ID, lo.P_ID], np.int64), np.array([lo.LONGEST, PARTNER_LEN], np.int32)
    P = trim_ref.params(min_cov=3, end_clip=10, min_span=50, min_identity=0.5)
    erows, eflags, ecounts = lo.trim_unfolded(folded, lo.LONGEST, WINDOW, PARTNER_LEN, P)
    assert erows[0, 2] >= 6 and erows[0, 0] == 5000 and eflags[0] & trim_ref.GAPPED     # the two runs of 4 000: the first wins
    with _timed("trimming, one read of 2^31 - 9 bases"):
        with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
            ts.add(real)
            assert ts.finish() == ecounts
            rows, flags = ts.table()
            assert rows.tolist() == erows.tolist() and flags.tolist() == eflags.tolist()
            assert ts.coverage(1).tobytes() == trim_ref.trim([lo.A_ID, lo.B_ID, lo.P_ID], [WINDOW, WINDOW, PARTNER_LEN], folded, P)[3][2].astype(np.int32).tobytes()
            out, keep = ts.apply(real)
            eout, ekeep = trim_ref.apply(ids, erows, eflags, real, P)
            assert keep.tobytes() == ekeep.tobytes() and out.tobytes() == eout.tobytes() and keep.any()
    # a best run in the last window: its begin and end are past 2^31 - 20 009
    P2 = trim_ref.params(min_cov=5, end_clip=0, min_span=1, min_identity=0.5)
    erows, eflags, ecounts = lo.trim_unfolded(folded, lo.LONGEST, WINDOW, PARTNER_LEN, P2)
    assert erows[0, 0] > lo.LONGEST - WINDOW
    with api.TrimSession(ids, lengths, handle=ms, **P2) as ts:
        ts.add(real)
        assert ts.finish() == ecounts
        rows, flags = ts.table()
        assert rows.tolist() == erows.tolist() and flags.tolist() == eflags.tolist()


def test_repeat_marking_a_read_of_2_31_minus_9_bases(ms):
    folded, real = _longest_records(34)
    ids, lengths = np.array([lo.A_ID, lo.P_ID], np.int64), np.array([lo.LONGEST, PARTNER_LEN], np.int32)
    P = repeat_ref.params(max_cov=2, min_run=100, min_unique=200, min_identity=0.5)
    e = lo.repeat_unfolded(folded, lo.LONGEST, WINDOW, PARTNER_LEN, P)
    long_iv = e["intervals"][:e["offsets"][1]]
    assert len(long_iv) >= 6 and long_iv[0, 0] == 0 and long_iv[-1, 1] == lo.LONGEST and e["hist"][0] > (1 << 31) - 2 * WINDOW
    with _timed("repeat marking, one read of 2^31 - 9 bases"):
        with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:
            rs.add(real)
            assert rs.finish() == e["counts"]
            rows, flags, offsets, iv = rs.table()
            assert offsets.tolist() == e["offsets"].tolist() and iv.tolist() == e["intervals"].tolist()
            assert rows.tolist() == e["rows"].tolist() and flags.tolist() == e["flags"].tolist()
            assert rs.histogram().tolist() == e["hist"].tolist()
            keep, unique = rs.apply(real)
            ekeep, eunique = repeat_ref.apply(ids, e["offsets"], e["intervals"], real, P)
            assert keep.tobytes() == ekeep.tobytes() and unique.tobytes() == eunique.tobytes()


# ---- case 4: the vote table, a little over 2^32 words --------------------------------------------------------------------------------------
VOTE_STRADDLERS = {M30: 4, M31: 11, M32: 18}
VOTE_FRACTION = {M30: 2.5 / 12, M31: 6.5 / 12, M32: 10.5 / 12}     # the plane of the straddler the mark falls into: 2, 6, 10
FILLER_BASES = 1 << 26


def test_read_correction_across_words_2_30_2_31_and_2_32(ms):
    """24 reads of a 2 500-base genome at 10 % error with their realigned records and paths, between fillers that alias one buffer of
    2^26 random bases; the vote table is a little over 2^32 words (17.2 GB)."""
    reads, _, bases, pairs, meta = cref.quality_workload(9, n_reads=24, error=0.10)
    results, op_offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs, handle=ms)
    recs = cref.quality_records(reads, meta, results)
    tlen = [len(r) for r in reads]
    lay = lo.place(tlen, VOTE_STRADDLERS, lo.vote_words, FILLER_BASES, VOTE_FRACTION)
    found = lay.marks_inside_test_reads(lo.MARKS, lo.vote_words, 100)
    assert lay.total > M32 and max(lay.lengths[i] for i in lay.fillers) <= FILLER_BASES
    for mark in lo.MARKS:     # the plane the mark lies in, with planes of the same read on both sides of it
        k, o = found[mark]
        assert k == VOTE_STRADDLERS[mark] and 1 <= o // tlen[k] <= 10 and o // tlen[k] == int(12 * VOTE_FRACTION[mark])
    ref = cref.Consensus(reads, range(1, len(reads) + 1))
    ref.add(recs, op_offsets, ops)
    wseqs, wstats = ref.call(4)
    assert all(ref.votes[VOTE_STRADDLERS[m]].any() for m in lo.MARKS) and sum(s != r for s, r in zip(wseqs, reads)) > 12
    rng = np.random.default_rng(35)
    filler = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, FILLER_BASES)]
    small = np.frombuffer(b"".join(reads), np.uint8)
    host = np.concatenate([small, filler])
    n = len(lay)
    ids, offsets = np.zeros(n, np.int64), np.zeros(n, np.int64)
    starts = np.concatenate([[0], np.cumsum(tlen)])
    for k, i in enumerate(lay.test):
        ids[i], offsets[i] = k + 1, starts[k]
    for u, i in enumerate(lay.fillers):
        ids[i], offsets[i] = 1000 + u, len(small)
    fasta = mhap_amd.FastaData(host, offsets, np.array(lay.lengths, np.int32), ids)
    with _timed("read correction, 2^32 words"):
        with mhap_amd.CorrectSession(fasta, handle=ms) as cs:
            assert cs.table_bytes() == 4 * lay.total
            cs.add(recs, op_offsets, ops)
            for k, i in enumerate(lay.test):
                got = cs.votes(i).astype(np.int64)
                bad = np.argwhere(got != ref.votes[k])
                assert len(bad) == 0, (k, i, bad[:5].tolist())
            seqs, stats, skipped = cs.finish(4)
    assert skipped == ref.skipped_views == 0
    for k, i in enumerate(lay.test):
        assert seqs[i] == wseqs[k] and stats[i].tolist() == wstats[k].tolist(), (k, i)
    raw = filler.tobytes()
    for i in lay.fillers:
        L = lay.lengths[i]
        assert stats[i].tolist() == [L, L, 0, 0, 0, L] and seqs[i] == raw[:L], i


# ---- case 5: the caller's bases, a little over 2^32 bytes ----------------------------------------------------------------------------------

def _mutate(rng, s, div):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < div / 3:
            continue
        if u < 2 * div / 3:
            out.append(c)
            out.append(int(rng.choice(list(b"ACGT"))))
            continue
        out.append(int(rng.choice(list(b"ACGT"))) if u < div else c)
    return bytes(out)


class Bases:
    """Segments laid into one zeroed buffer of a little over 2^32 bytes at five places: below 2^31, across it (the mark lies 300
    bytes into the block's first segment), between the marks, across 2^32 and above it.  at[p][s]: segment s's offset at place p;
    small, small_at[s]: the same segments back to back for the restatements."""

    def __init__(self, segments):
        self.segments = [bytes(s) for s in segments]
        assert len(self.segments[0]) > 400
        self.small = np.frombuffer(b"".join(self.segments), np.uint8)
        self.small_at = np.concatenate([[0], np.cumsum([len(s) for s in self.segments])])[:-1].tolist()
        block = len(self.small)
        firsts = [1000, M31 - 300, M31 + (1 << 30), M32 - 300, M32 + 50000]
        self.big = np.zeros(M32 + 50000 + block + 1000, np.uint8)
        self.at = []
        for f in firsts:
            self.big[f:f + block] = self.small
            self.at.append([f + o for o in self.small_at])
        # the places are where they are said to be
        a = self.at
        assert a[0][-1] + len(self.segments[-1]) < M31 and a[1][0] < M31 < a[1][0] + len(self.segments[0]) and a[1][1] > M31
        assert M31 < a[2][0] and a[2][-1] + len(self.segments[-1]) < M32
        assert a[3][0] < M32 < a[3][0] + len(self.segments[0]) and a[3][1] > M32 and a[4][0] > M32 and len(self.big) > M32

    def rows(self, pairs):
        """pairs = [(segment a, segment b, ...)]: (big rows, small rows, the index of each big row's small row).  Every pair at all
        five places, and with its two segments at different places, on opposite sides of each mark."""
        big, small, which = [], [], []
        for q, (sa, sb, *rest) in enumerate(pairs):
            small.append((self.small_at[sa], len(self.segments[sa]), self.small_at[sb], len(self.segments[sb]), *rest))
            for pa, pb in [(p, p) for p in range(5)] + [(0, 2), (2, 0), (2, 4), (4, 2), (0, 4), (4, 1), (3, 0)]:
                big.append((self.at[pa][sa], len(self.segments[sa]), self.at[pb][sb], len(self.segments[sb]), *rest))
                which.append(q)
        return np.array(big, np.int64), np.array(small, np.int64), np.array(which)


@pytest.fixture
def big_bases():     # (function scope: the 4.3 GB of host memory go back before the next case takes its own)
    rng = np.random.default_rng(36)
    segs, pairs = [], []     # pairs: (segment a, segment b, b_rc, the diagonal the pair lies on)
    for n, rc in ((700, 0), (2300, 1), (450, 1), (1400, 0)):     # the one-wave and the four-wave forms of the aligners, both strands
        s = bytes(rng.choice(list(b"ACGT"), n).tolist())
        st = int(rng.integers(0, n // 5))
        t = _mutate(rng, s[st:], 0.12)
        segs += [s, align_ref.rc_bytes(t) if rc else t]
        pairs.append((len(segs) - 2, len(segs) - 1, rc, -st))
    return Bases(segs), pairs


def test_aligners_and_pair_statistics_with_segments_across_bytes_2_31_and_2_32(ms, big_bases):
    """One call each of align_pairs, align_pairs_banded, align_pairs_banded_paths and pair_kmer_stats over the big buffer; every row
    equals the restatement's row of the same two segments."""
    B, pairs = big_bases
    assert {rc for _, _, rc, _ in pairs} == {0, 1}
    big5, small5, which = B.rows([(a, b, rc) for a, b, rc, _ in pairs])
    assert (big5[:, 0] > M32).any() and (big5[:, 2] > M32).any() and ((big5[:, 0] < M31) & (big5[:, 2] > M32)).any()
    with _timed("align_pairs, 2^32 bytes of bases"):
        got = mhap_amd.align_pairs(B.big, big5, handle=ms)
    want = align_ref.align_pairs(B.small, small5)
    assert (want[:, 0] > 0).all() and got.tolist() == want[which].tolist()

    big7, small7, which = B.rows([(a, b, rc, d, 90) for a, b, rc, d in pairs])
    with _timed("align_pairs_banded, 2^32 bytes of bases"):
        got = mhap_amd.align_pairs_banded(B.big, big7, handle=ms)
    want = bref.align_pairs_banded(B.small, small7)
    assert (want[:, 0] > 0).all() and got.tolist() == want[which].tolist()

    with _timed("align_pairs_banded_paths, 2^32 bytes of bases"):
        got, offs, ops = mhap_amd.align_pairs_banded_paths(B.big, big7, handle=ms)
    want, woffs, wops = pref.align_pairs_banded_paths(B.small, small7)
    assert got.tolist() == want[which].tolist()
    for q, w in enumerate(which.tolist()):
        assert ops[offs[q]:offs[q + 1]].tolist() == wops[woffs[w]:woffs[w + 1]].tolist(), q
    assert len(ops) > 100 * len(which)

    big4, small4, which = B.rows([(a, b) for a, b, _, _ in pairs])
    with _timed("pair_kmer_stats, 2^32 bytes of bases"):
        got = mhap_amd.pair_kmer_stats(B.big, big4, 12, handle=ms)
    want = [ksim_ref.pair_stats(B.segments[a].decode(), B.segments[b].decode(), 12) for a, b, _, _ in pairs]
    assert sum(w[0] > 100 for w in want) == 2     # the forward pairs share k-mers; a stored reverse complement shares none
    assert got.tolist() == [list(want[w]) for w in which.tolist()]


def test_spelling_reads_that_lie_across_bytes_2_31_and_2_32(ms):
    """A chain of six reads and four lone ones whose bytes lie below 2^31, across it (one read; another ends where it begins), between
    the marks, across 2^32 (likewise) and above it."""
    ids, lengths, reads, recs = ur.chain(6, 41)
    lone = [3100, 2800, 5200, 999]
    ids, lengths = list(ids) + [101, 102, 103, 104], list(lengths) + lone
    _, chain_bases, chain_offsets = ur.plant(reads, 41)
    lone_bases, lone_offsets = ur.random_bases(lone, 42)
    small = np.concatenate([chain_bases, lone_bases])
    small_offsets = np.concatenate([chain_offsets, lone_offsets + len(chain_bases)]).astype(np.int64)
    places = [1000, M31 - 2000, M31 + (1 << 29), M32 - 2500, M32 + 70000, M31 - 40000, M31 - 2000 - lone[0], M32 - 9000, M32 - 2500 + lengths[3], M32 + 10000]
    spans = sorted((at, at + lengths[r]) for r, at in enumerate(places))
    assert all(e <= s for (_, e), (s, _) in zip(spans, spans[1:]))                     # no two reads share a byte
    big = np.zeros(M32 + 100000, np.uint8)
    big_offsets = np.array(places, np.int64)
    for r, at in enumerate(places):
        big[at:at + lengths[r]] = small[small_offsets[r]:small_offsets[r] + lengths[r]]
    crossing = [r for r, at in enumerate(places) for m in (M31, M32) if at < m < at + lengths[r]]
    assert crossing == [1, 3] and places[6] + lengths[6] == places[1] and min(places[4], places[8], places[9]) > M32
    ref = sg.Graph(ids, lengths, sg.Params())
    ref.add(recs)
    ref.finish()
    want = ur.of_graph(ref)
    assert len(want.unitig_len) == 5 and {v & 1 for v in want.vertex} == {0, 1}     # the chain and the lone reads; members on both strands
    want_seqs = want.sequences(small, small_offsets, lengths)
    with _timed("spelling, 2^32 bytes of bases"):
        with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
            gs.add(recs)
            gs.finish()
            got = gs.unitigs()
            assert got["vertex"].tolist() == list(want.vertex) and got["counts"] == want.tables()["counts"]
            out = np.full(sum(want.unitig_len), 1, np.uint8)
            gs.spell_into(big, big_offsets, out)
    assert out.tobytes() == b"".join(want_seqs)


# ---- case 6: the trace buffer, more than 2^32 words in one group ----------------------------------------------------------------------------
TRACE_PAIR, TRACE_BAND, TRACE_DISTINCT = 10000, 1100, 2


def test_paths_whose_trace_lies_past_word_2_32(ms, monkeypatch):
    """Two distinct pairs of 10 kb at 30 % divergence, a good 8 MB of trace each, repeated in one call under a trace budget that keeps
    all copies in one group: copy 0 equals the restatement, every other copy equals copy 0, and by the documented lower bound
    (I + D + 1) ceil(rows / 8) the last copy's words begin behind 2^32."""
    rng = np.random.default_rng(37)
    segs, rows = [], []
    for d in range(TRACE_DISTINCT):
        s = bytes(rng.choice(list(b"ACGT"), TRACE_PAIR).tolist())
        t = _mutate(rng, s, 0.3)
        at = sum(len(x) for x in segs)
        rows.append((at, len(s), at + len(s), len(t), d & 1, 0, TRACE_BAND))
        segs += [s, align_ref.rc_bytes(t) if d & 1 else t]
    bases = np.frombuffer(b"".join(segs), np.uint8)
    rows = np.array(rows, np.int64)
    want, woffs, wops = pref.align_pairs_banded_paths(bases, rows)
    # the bound of docs/DESIGN.limits.md, "Paths", holds while the band does not cut the I + D + 1 diagonals
    words = []
    for a in want.tolist():
        m, n = a[2] - a[1] + 1, a[4] - a[3] + 1
        ins, dele, d0 = a[5] - n, a[5] - m, a[3] - a[1]
        assert a[0] > 0 and ins + abs(d0) < TRACE_BAND and dele + abs(d0) < TRACE_BAND and m > 9000
        words.append((ins + dele + 1) * -(-m // 8))
    assert min(words) > 1 << 20
    copies = -(-(M32 + 1) // sum(words)) + 1
    pairs = np.tile(rows, (copies, 1))
    monkeypatch.setenv("MHAP_REALIGN_TRACE_BYTES", str(40 << 30))
    with _timed(f"paths, {len(pairs)} pairs, trace past word 2^32"):
        got, offs, ops = mhap_amd.align_pairs_banded_paths(bases, pairs, handle=ms)
    # from the returned results: the words in front of the last copy
    in_front = 0
    for a in got[:-TRACE_DISTINCT].tolist():
        in_front += (2 * a[5] - (a[4] - a[3] + 1) - (a[2] - a[1] + 1) + 1) * -(-(a[2] - a[1] + 1) // 8)
    assert in_front > M32, in_front
    assert got[:TRACE_DISTINCT].tolist() == want.tolist()
    assert ops[:offs[TRACE_DISTINCT]].tolist() == wops.tolist() and offs[:TRACE_DISTINCT + 1].tolist() == woffs.tolist()
    per_copy = int(offs[TRACE_DISTINCT])
    assert len(ops) == copies * per_copy and (np.diff(offs).reshape(copies, TRACE_DISTINCT) == np.diff(woffs)).all()
    assert (got.reshape(copies, -1) == got[:TRACE_DISTINCT].reshape(1, -1)).all()
    assert (ops.reshape(copies, per_copy) == ops[:per_copy]).all()
