"""Helpers of tests/test_large_offsets_stages_cpu.py and tests/test_large_offsets_stages_gpu.py: the layouts, the constants and the
written-out expectations of the large-offset cases of the stages that came after tests/large_offsets.py — base qualities, weighted
votes, variant sites, homopolymer compression and the correction's own bases.  Both files import every constant from here, so the
layout the CPU file proves is the layout the GPU file runs.

Part A puts marks into device tables: fillers that take no record alias one small host buffer and only push offsets, the test reads
carry every record (tests/large_offsets.py places them).  A filler's result is written out here from the contracts: its corrected
bytes are its own, its quality bytes follow from a lookup by byte, weight class and last position that the restatement's own call
makes on voteless reads of two bytes, and the variant stage gives it depth 1, no site and the row (0, 0).

Part B puts marks into the caller's bases: the same small reads laid into one buffer of a little over 2^32 bytes at five places, every
copy a read of its own id, the records repeated per place and carried across the marks; the restatements run on the same reads and
ids laid back to back.  The homopolymer table adds reads of zeros that alias each other and one read of 2^31 - 9 bases whose result
is the composition of its two windows."""
import numpy as np

import consensus_ref as cref
import hpc_cases as hc
import hpc_ref
import large_offsets as lo
import quality_ref as qref
import weighted_vote_ref as wref

M30, M31, M32 = lo.MARKS


# ---- part A: the workload and the three layouts --------------------------------------------------------------------------------------------
WORKLOAD = dict(seed=9, n_reads=24, error=0.10)          # the reads of test_read_correction_across_words_2_30_2_31_and_2_32
FILLER_BASES = 1 << 26
PHRED = (0, 5, 6, 7, 14, 19, 20, 30, 93)                 # Phred values on both sides of the default thresholds: every weight class
VOTE_STRADDLERS = {M30: 4, M31: 11, M32: 18}
VOTE_FRACTION = {M30: 2.5 / 12, M31: 6.5 / 12, M32: 10.5 / 12}        # planes 2, 6 and 10 of the 12
VARIANT_STRADDLERS = {M30: 4, M31: 11, M32: 16}
VARIANT_FRACTION = {M30: 0.5 / 3, M31: 1.5 / 3, M32: 2.5 / 3}         # planes 0, 1 and 2 of the 3
SITE_MARKS = (M31, M32)                                  # positions: the site bytes and read_pos
SITE_STRADDLERS = {M31: 8, M32: 16}
MARGIN = 100
VARIANT_PARAMS = dict(min_depth=4, min_minor=2, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # variant_cases.SMALL, named in full
SITE_TABLE_BYTES = 13 * (M32 + 1)                        # what the session of positions 2^31 and 2^32 takes at the least: 12 + 1 bytes per position


def variant_words(length):
    """A read of the variant stage's vote table owns 3 words per base, plane p lying p L words behind its first word."""
    return 3 * int(length)


def workload():
    """(reads, bases, pairs7, meta) of the part A workload; the caller aligns the pairs.  The generator makes the earlier read of the
    table read A of every pair; every second pair is turned round here, so that read A lies behind read B as often as in front of it:
    a pair (i, j) of a and s2 is the pair (lb - 1 - j, la - 1 - i) of b and the reverse complement of a when to_rc, else (j, i)."""
    reads, _, bases, pairs, meta = cref.quality_workload(WORKLOAD["seed"], n_reads=WORKLOAD["n_reads"], error=WORKLOAD["error"])
    pairs, meta = pairs.copy(), list(meta)
    for q in range(1, len(pairs), 2):
        a_off, la, b_off, lb, rc, diag, band = pairs[q].tolist()
        pairs[q] = (b_off, lb, a_off, la, rc, diag + la - lb if rc else -diag, band)
        meta[q] = (meta[q][1], meta[q][0], rc)
    return reads, bases, pairs, meta


def _planes(lay, found, tlen, straddlers, fraction, planes):
    """The plane every mark lies in, with words of the same read on both sides of it; {mark: (test read, position in the read)}."""
    out = {}
    for mark, (k, o) in found.items():
        assert k == straddlers[mark] and o // tlen[k] == int(planes * fraction[mark]) and MARGIN <= o % tlen[k] < tlen[k] - MARGIN, (mark, k, o)
        out[mark] = (k, o % tlen[k])
    return out


def correction_layout(tlen):
    """(layout, {mark: (test read, position)}) of the vote table of 12 words per base: the marks in planes 2, 6 and 10."""
    lay = lo.place(tlen, VOTE_STRADDLERS, lo.vote_words, FILLER_BASES, VOTE_FRACTION)
    found = lay.marks_inside_test_reads(lo.MARKS, lo.vote_words, MARGIN)
    assert lay.total > M32 and max(lay.lengths[i] for i in lay.fillers) <= FILLER_BASES
    at = _planes(lay, found, tlen, VOTE_STRADDLERS, VOTE_FRACTION, 12)
    assert [found[m][1] // tlen[found[m][0]] for m in lo.MARKS] == [2, 6, 10]
    return lay, at


def variant_layout(tlen):
    """The same for the table of 3 words per base: the marks in planes 0, 1 and 2."""
    lay = lo.place(tlen, VARIANT_STRADDLERS, variant_words, FILLER_BASES, VARIANT_FRACTION)
    found = lay.marks_inside_test_reads(lo.MARKS, variant_words, MARGIN)
    assert lay.total > M32 and max(lay.lengths[i] for i in lay.fillers) <= FILLER_BASES
    at = _planes(lay, found, tlen, VARIANT_STRADDLERS, VARIANT_FRACTION, 3)
    assert [found[m][1] // tlen[found[m][0]] for m in lo.MARKS] == [0, 1, 2]
    return lay, at


def site_layout(tlen):
    """The layout by positions (one site byte per base): a straddler across position 2^31 and one across 2^32, test reads in front of,
    between and behind them, and the table's words past 3 * 2^32."""
    lay = lo.place(tlen, SITE_STRADDLERS, lo.base_bytes, FILLER_BASES)
    found = lay.marks_inside_test_reads(SITE_MARKS, lo.base_bytes, MARGIN)
    assert lay.total > M32 and 3 * lay.total > 3 * M32 and max(lay.lengths[i] for i in lay.fillers) <= FILLER_BASES
    assert [found[m][0] for m in SITE_MARKS] == [SITE_STRADDLERS[m] for m in SITE_MARKS]
    side = [sum(lay.starts[i] + lay.lengths[i] <= M31 for i in lay.test), sum(M31 < lay.starts[i] and lay.starts[i] + lay.lengths[i] <= M32 for i in lay.test),
            sum(lay.starts[i] > M32 for i in lay.test)]
    assert min(side) >= 2, side
    return lay, {m: found[m] for m in SITE_MARKS}


def sites_round(v, at):
    """Asserts from the restatement that every straddler has a site in front of its mark's position and one behind it."""
    for mark, (k, t) in at.items():
        mine = v.sites[int(v.offsets[k]):int(v.offsets[k + 1]), 0]
        assert (mine < t).any() and (mine > t).any(), (mark, k, t, mine.tolist())


def records_across(lay, recs, mark):
    """{(A below the mark and B above it, to_rc)} over the records; ids are 1 + the test read's number, the places those of the layout."""
    seen = set()
    for rec in recs:
        a, b = lay.starts[lay.test[int(rec["from_id"]) - 1]], lay.starts[lay.test[int(rec["to_id"]) - 1]]
        if (a < mark) != (b < mark):
            seen.add((bool(a < mark), int(rec["to_rc"])))
    return seen


def aliased_table(lay, reads, filler):
    """(bases, ids, offsets, lengths) of a layout: the test reads back to back, then the filler buffer, which every filler reads from
    its first byte.  Test read k has the id k + 1, filler u the id 1000 + u."""
    small = np.frombuffer(b"".join(reads), np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    n = len(lay)
    ids, offsets = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k, i in enumerate(lay.test):
        ids[i], offsets[i] = k + 1, starts[k]
    for u, i in enumerate(lay.fillers):
        ids[i], offsets[i] = 1000 + u, len(small)
    return np.concatenate([small, filler]), ids, offsets, np.array(lay.lengths, np.int32)


# ---- part A: what a filler must give --------------------------------------------------------------------------------------------------------

def weight_class(quals, q_lo=wref.DEFAULT_Q_LO, q_hi=wref.DEFAULT_Q_HI):
    """0, 1, 2 for the weights 1, 2, 3."""
    q = np.asarray(quals, np.int64)
    return (q >= q_lo).astype(np.int64) + (q >= q_hi)


def filler_quality_lookup(weighted, min_cov=4, per_vote=15, cap=60, q_lo=wref.DEFAULT_Q_LO, q_hi=wref.DEFAULT_Q_HI):
    """lut[byte, class, last]: the quality byte of a position nobody voted on, by its own byte, its weight class (one class when not
    weighted) and whether it is the read's last.  Made by the restatement's own call on voteless reads of two bytes; such a position
    emits its own byte and nothing else, which is asserted."""
    assert 0 < q_lo < q_hi
    phred = (q_lo - 1, q_lo, q_hi) if weighted else (0,)
    lut = np.zeros((256, len(phred), 2), np.uint8)
    votes = np.zeros((2, cref.NCOUNT), np.int64)
    for b in range(256):
        for c, q in enumerate(phred):
            own = bytes([b, b])
            if weighted:
                seq, quals, counts = wref.call(own, [q, q], votes, min_cov, per_vote, cap, q_lo, q_hi)
                assert counts == (0, 0, 0, 2)
            else:
                seq, quals = qref.call(own, votes, min_cov, per_vote, cap)
            assert seq == own and len(quals) == 2
            lut[b, c] = quals
    return lut


class FillerQualities:
    """The quality bytes of every filler of a layout over one buffer, by the lookup: of(L) is the array of a filler of L bases (a view
    of one expansion with its last byte set), hist(L) its 94 bins."""

    def __init__(self, lut, buf, classes=None):
        self.lut, self.buf = lut, buf
        self.cls = np.zeros(len(buf), np.int64) if classes is None else classes
        self.inner = lut[buf, self.cls, 0]
        self._hist = {}

    def last(self, L):
        return int(self.lut[self.buf[L - 1], self.cls[L - 1], 1])

    def equals(self, got, L):
        return len(got) == L and np.array_equal(got[:L - 1], self.inner[:L - 1]) and int(got[L - 1]) == self.last(L)

    def hist(self, L):
        if L not in self._hist:
            h = np.bincount(self.inner[:L - 1], minlength=qref.BINS).astype(np.int64)
            h[self.last(L)] += 1
            self._hist[L] = h
        return self._hist[L]


def variant_with_fillers(lay, v, counts, params):
    """(counts, rows, offsets, sites) of the whole table from the restatement `v` on the test reads and its counts: nobody voted on a
    filler, so every position of it has depth 1 at the most (its own base), which is not deep for min_depth >= 2; it has no site, the
    row (0, 0) and an empty slice of the list, and its length enters `bases`."""
    assert params["min_depth"] >= 2
    n = len(lay)
    rows = np.zeros((n, 2), np.int32)
    rows[lay.test] = v.rows
    offsets = np.concatenate([[0], np.cumsum(rows[:, 0], dtype=np.int64)]).astype(np.int64)
    c = list(counts)
    c[0] = n
    c[4] = counts[4] + sum(lay.lengths[i] for i in lay.fillers)
    return c, rows, offsets, v.sites


# ---- part B: the same reads at five places of one buffer -------------------------------------------------------------------------------------
B_WORKLOAD = dict(seed=12, genome_len=1500, n_reads=9, error=0.10)
PLACE_FIRSTS = (1000, M31 - 300, M31 + (1 << 30), M32 - 300, M32 + 50000)      # below 2^31, across it, between, across 2^32, above it
CROSS = ((0, 2), (2, 0), (2, 4), (4, 2), (0, 4), (4, 1), (3, 0))                 # (place of read A, place of read B) of the cross-place records
ID_STEP = 1000


def b_workload():
    reads, _, bases, pairs, meta = cref.quality_workload(B_WORKLOAD["seed"], genome_len=B_WORKLOAD["genome_len"], n_reads=B_WORKLOAD["n_reads"],
                                                         error=B_WORKLOAD["error"])
    return reads, bases, pairs, meta


class Places:
    """Reads laid back to back at the five places.  at[p][k]: the offset of read k at place p; ids, offsets, lengths: the session's
    table, place by place (read k of place p has the id k + 1 + 1000 p); small_reads, small_offsets: the same reads and ids back to
    back, for the restatements."""

    def __init__(self, reads):
        self.reads = [bytes(r) for r in reads]
        self.k = len(self.reads)
        assert len(self.reads[0]) > 400 and self.k < ID_STEP
        self.block = np.frombuffer(b"".join(self.reads), np.uint8)
        rel = np.concatenate([[0], np.cumsum([len(r) for r in self.reads])])[:-1].tolist()
        self.at = [[f + o for o in rel] for f in PLACE_FIRSTS]
        self.size = PLACE_FIRSTS[-1] + len(self.block) + 1000
        assert self.size <= M32 + (1 << 17)
        self.ids = np.array([k + 1 + ID_STEP * p for p in range(5) for k in range(self.k)], np.int64)
        self.offsets = np.array([self.at[p][k] for p in range(5) for k in range(self.k)], np.int64)
        self.lengths = np.array([len(r) for r in self.reads] * 5, np.int32)
        self.small_reads = self.reads * 5
        self.small_offsets = np.concatenate([[0], np.cumsum(self.lengths[:-1], dtype=np.int64)]).astype(np.int64)
        self.check()

    def check(self):
        """The places are where they are said to be: a read's stored bytes lie across each mark."""
        a, n = self.at, [len(r) for r in self.reads]
        assert a[0][-1] + n[-1] < M31 and a[1][0] < M31 < a[1][0] + n[0] and a[1][1] > M31
        assert M31 < a[2][0] and a[2][-1] + n[-1] < M32
        assert a[3][0] < M32 < a[3][0] + n[0] and a[3][1] > M32 and a[4][0] > M32 and self.size > M32

    def lay(self, big, values=None):
        """Write the reads (or `values`, one array as long as the block: the qualities) into the buffer at the five places."""
        block = self.block if values is None else np.asarray(values, np.uint8)
        assert len(big) >= self.size and len(block) == len(self.block)
        for f in PLACE_FIRSTS:
            big[f:f + len(block)] = block

    def records(self, recs, op_offsets, ops, cross_every=1):
        """(records, op_offsets, ops, [(place A, place B)]) of the session: every small record at each place, and every
        cross_every-th one with its two reads at the places of CROSS; a copy keeps its record's runs."""
        out, paths, where = [], [], []
        for q in range(len(recs)):
            runs = ops[int(op_offsets[q]):int(op_offsets[q + 1])]
            for pa, pb in [(p, p) for p in range(5)] + (list(CROSS) if q % cross_every == 0 else []):
                r = recs[q:q + 1].copy()
                r["from_id"] += ID_STEP * pa
                r["to_id"] += ID_STEP * pb
                out.append(r)
                paths.append(runs)
                where.append((pa, pb))
        off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
        return np.concatenate(out), off, np.concatenate(paths).astype(np.uint32), where

    def records_across(self, recs, where):
        """Asserts that some record has its A read below 2^31 and its B read above 2^32, and the reverse, on both strands."""
        seen = set()
        for rec, (pa, pb) in zip(recs, where):
            a = self.at[pa][int(rec["from_id"]) % ID_STEP - 1]
            b = self.at[pb][int(rec["to_id"]) % ID_STEP - 1]
            la, lb = len(self.reads[int(rec["from_id"]) % ID_STEP - 1]), len(self.reads[int(rec["to_id"]) % ID_STEP - 1])
            if a + la <= M31 and b >= M32:
                seen.add(("A below", int(rec["to_rc"])))
            if b + lb <= M31 and a >= M32:
                seen.add(("B below", int(rec["to_rc"])))
        assert seen == {("A below", 0), ("A below", 1), ("B below", 0), ("B below", 1)}, seen


# ---- part B: the homopolymer table ------------------------------------------------------------------------------------------------------------
HPC_W = 20000                                            # a window of the long read, and the length of a block of crafted reads
HPC_MARK_AT = 9984                                       # where a mark lies in the block laid across it (a multiple of 16)
HPC_LONG_AT = M31 - HPC_MARK_AT                          # the long read begins with the block across 2^31 and ends with the block between the marks
HPC_FIRSTS = (1008, HPC_LONG_AT, HPC_LONG_AT + lo.LONGEST - HPC_W, M32 - HPC_MARK_AT, M32 + 50000)
HPC_ZERO_READS, HPC_ZERO_LEN = 18, (1 << 28) - 5         # reads of zeros below 2^31 that share bytes with each other: each a group of its own
HPC_SIZE = HPC_FIRSTS[-1] + HPC_W + 1000
HPC_GROUP_DEFAULT = 1 << 28
BIG_SIZE = M32 + (1 << 17)                               # the one host buffer of the part B cases
assert HPC_SIZE <= BIG_SIZE


def hpc_block(T, seed=41):
    """(content, rows): HPC_W bytes of runs over A, C, G, T, N, a, 0x00 and 0xFF, and the crafted reads as (offset, length) into them.
    Sixteen reads of two tiles begin at every offset modulo 16, a read of three tiles, reads round the wave's 64 positions, an empty
    read, a read that ends with the block; the bytes round HPC_MARK_AT are one run, reads begin on that position and on the next, and
    the byte in front of every one of these reads equals the read's first."""
    rng = np.random.default_rng(seed)
    content = hc.runs_of(rng, HPC_W, list(b"ACGT") * 3 + [ord("N"), ord("a"), 0, 255]).copy()
    assert T + 1 + 45 < HPC_W // 4
    rows = [(16 * (1 + 56 * m) + m, T + 1 + 3 * m) for m in range(16)]
    rows += [(5, 2 * T + 5), (HPC_W - T - 9, T + 9)]
    rows += [(18000 + 70 * i, n) for i, n in enumerate((0, 1, 2, 63, 64, 65))]
    content[HPC_MARK_AT - 2:HPC_MARK_AT + 3] = ord("C")
    rows += [(HPC_MARK_AT, T + 3), (HPC_MARK_AT + 1, 700)]
    for o, n in rows:
        if n and o:
            content[o - 1] = content[o]
    assert content[HPC_MARK_AT - 1] == content[HPC_MARK_AT] == content[HPC_MARK_AT + 1] == content[HPC_MARK_AT + 2]
    assert {o % 16 for o, _ in rows[:16]} == set(range(16)) and all(o + n <= HPC_W for o, n in rows)
    return content, rows


def hpc_filling(content):
    """The byte of the long read between its windows: one of A, C, G, T that neither the last byte of the first window nor the first
    byte of the second is (both windows are the block)."""
    return next(c for c in b"GTAC" if c != content[-1] and c != content[0])


class HpcTable:
    """The table of the homopolymer case over one buffer of HPC_SIZE bytes, zero outside the reads: kinds[r] is ("small", place, row),
    ("zero",) or ("long",); offsets, lengths, ids (1 ..) in table order."""

    def __init__(self, T):
        self.T = T
        self.content, self.rows = hpc_block(T)
        self.c = hpc_filling(self.content)
        zero0, zero1 = HPC_FIRSTS[0] + HPC_W, HPC_LONG_AT
        step = (zero1 - zero0 - HPC_ZERO_LEN - HPC_ZERO_READS) // (HPC_ZERO_READS - 1)
        zeros = [(zero0 + j * step + j, HPC_ZERO_LEN) for j in range(HPC_ZERO_READS)]
        assert all(zero0 <= o and o + n <= zero1 for o, n in zeros) and len({o % 16 for o, _ in zeros}) >= 4
        kinds, where = [], []

        def small(p):
            for u, (o, n) in enumerate(self.rows):
                kinds.append(("small", p, u))
                where.append((HPC_FIRSTS[p] + o, n))

        def zero(some):
            for z in some:
                kinds.append(("zero",))
                where.append(z)
        small(0)
        zero(zeros[:9])
        small(1)
        kinds.append(("long",))
        where.append((HPC_LONG_AT, lo.LONGEST))
        small(2)
        zero(zeros[9:])
        small(3)
        small(4)
        self.kinds = kinds
        self.offsets = np.array([o for o, _ in where], np.int64)
        self.lengths = np.array([n for _, n in where], np.int32)
        self.ids = np.arange(1, len(kinds) + 1, dtype=np.int64)
        self.long = kinds.index(("long",))
        self.check()

    def check(self):
        """From the layout alone: the blocks lie below, across, between, across and above the marks, the long read's windows are two
        of them and its second window reaches into its last tile, a read of more than one tile lies across each mark with the mark
        inside it, reads begin on the mark and just above it, every misalignment occurs above 2^32, and the default cap gives more
        than 16 groups."""
        f, T = HPC_FIRSTS, self.T
        assert f[0] + HPC_W < M31 and f[1] < M31 < f[1] + HPC_W and M31 < f[2] and f[2] + HPC_W < M32 and f[3] < M32 < f[3] + HPC_W and f[4] > M32
        assert f[1] == HPC_LONG_AT and f[2] + HPC_W == HPC_LONG_AT + lo.LONGEST and f[2] + HPC_W <= f[3] and HPC_SIZE > M32
        last_tile = (lo.LONGEST - 1) // T * T
        assert lo.LONGEST - HPC_W < last_tile and last_tile + 16 * 255 + 16 > (1 << 31) - 32
        for mark in (M31, M32):
            inside = [r for r in range(len(self.kinds)) if self.kinds[r][0] == "small" and self.offsets[r] < mark - 2 and mark + 2 < self.offsets[r] + self.lengths[r]]
            assert any(self.lengths[r] > T for r in inside), mark
            assert any(self.offsets[r] == mark for r in range(len(self.kinds))) and any(self.offsets[r] == mark + 1 for r in range(len(self.kinds)))
        above = [r for r in range(len(self.kinds)) if self.kinds[r][0] == "small" and self.offsets[r] > M32 and self.lengths[r] > T]
        assert {int(self.offsets[r]) % 16 for r in above} == set(range(16))
        assert len(plan_groups(self.lengths, HPC_GROUP_DEFAULT)) > 16 and int(self.lengths.astype(np.int64).sum()) > 16 * HPC_GROUP_DEFAULT
        assert len(plan_groups(self.lengths, 1 << 30)) < len(plan_groups(self.lengths, HPC_GROUP_DEFAULT))

    def lay(self, big):
        assert len(big) >= HPC_SIZE
        big[HPC_LONG_AT:HPC_LONG_AT + lo.LONGEST] = self.c
        for f in HPC_FIRSTS:
            big[f:f + HPC_W] = self.content

    def expected(self, big):
        """The dict of hpc_ref.compress for the table over `big`: the small reads by hpc_ref.compress_read on their own bytes, a read
        of zeros as one byte with the map (0, L), the long read as the composition of its windows."""
        parts = []
        for r, kind in enumerate(self.kinds):
            o, n = int(self.offsets[r]), int(self.lengths[r])
            if kind[0] == "small":
                parts.append(hpc_ref.compress_read(big[o:o + n]))
            elif kind[0] == "zero":
                parts.append((np.zeros(1, np.uint8), np.array([0, n], np.int32)))
            else:
                parts.append(hpc_compose(big[o:o + HPC_W], self.c, n - 2 * HPC_W, big[o + n - HPC_W:o + n]))
        return hpc_assemble(parts, self.lengths, self.ids)

    def rows_of(self, *places):
        return [r for r, kind in enumerate(self.kinds) if kind[0] == "small" and kind[1] in places and self.lengths[r] > 0]


def plan_groups(lengths, cap):
    """The header's rule once more: whole reads in table order, a group closed in front of the read that would take it past `cap` raw
    bases, a longer read a group of its own.  [(first read, end, bases)]."""
    groups, r0, bases = [], 0, 0
    for r, n in enumerate(np.asarray(lengths).tolist()):
        if r > r0 and bases + n > cap:
            groups.append((r0, r, bases))
            r0, bases = r, 0
        bases += n
    if len(lengths) > r0:
        groups.append((r0, len(lengths), bases))
    return groups


def hpc_compose(A, c, fill, B):
    """(head bytes, start) of the read A ++ c * fill ++ B from hpc_ref.compress_read on the two windows: comp(A) ++ [c] ++ comp(B), the
    map entries of B moved up by len(A) + fill and the sentinel the whole length.  c differs from A's last byte and from B's first,
    so the filling is one run of its own and breaks no run of a window."""
    A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
    assert fill >= 1 and len(A) and len(B) and c != A[-1] and c != B[0]
    ha, sa = hpc_ref.compress_read(A)
    hb, sb = hpc_ref.compress_read(B)
    shift = len(A) + int(fill)
    start = np.concatenate([sa[:-1].astype(np.int64), [len(A)], sb[:-1].astype(np.int64) + shift, [shift + len(B)]])
    assert int(start[-1]) <= lo.LONGEST
    return np.concatenate([ha, [c], hb]).astype(np.uint8), start.astype(np.int32)


def hpc_assemble(parts, lengths, ids):
    """hpc_ref.compress's dict from every read's (head bytes, start)."""
    from mhap_amd import api
    n = len(parts)
    clen = np.array([len(h) for h, _ in parts], np.int32)
    coff = np.zeros(n + 1, np.int64)
    np.cumsum(clen, out=coff[1:])
    runs = [np.diff(s.astype(np.int64)) for _, s in parts]
    counts = dict(zip(api.HPC_COUNTS, [n, int(np.asarray(lengths, np.int64).sum()), int(coff[n]), sum(int((d > 1).sum()) for d in runs),
                                       max([int(d.max()) for d in runs if len(d)], default=0), int((np.asarray(lengths) == 0).sum())]))
    cbases = np.concatenate([h for h, _ in parts]).astype(np.uint8)
    return dict(cbases=cbases, coff=coff, clen=clen, starts=np.concatenate([s for _, s in parts]).astype(np.int32), counts=counts,
                fasta=api.FastaData(cbases, coff[:n], clen, ids), raw_lengths=np.asarray(lengths, np.int32))


def hpc_records(rng, want, pairs, n):
    """n records in compressed coordinates between the reads of `pairs` = [(read A, read B)] (rows of the table), drawn in turn: the
    ends from -1, 0, clen - 1, clen and anywhere, both values of to_rc (hpc_cases.random_records' draw)."""
    out = np.zeros(n, hc.api.RECORD_DTYPE)
    for q in range(n):
        ends = []
        for r in pairs[q % len(pairs)]:
            c = int(want["clen"][r])
            pick = lambda: int(rng.choice([-1, 0, c - 1, c, int(rng.integers(-1, c + 1))]))   # noqa: E731
            ends.append((int(want["fasta"].ids[r]), pick(), pick(), c))
        (f, a1, a2, alen), (t, b1, b2, blen) = ends
        out[q] = hc.rec(f, t, a1, a2, alen, b1, b2, blen, q & 1, score=float(rng.random()), raw=float(rng.integers(0, 500)))
    return out
