"""Helpers of tests/test_large_offsets_cpu.py and tests/test_large_offsets_gpu.py: tables of reads whose per-base device arrays cross
element 2^30 (byte 2^32 of a 4-byte element), 2^31 and 2^32 while the host and the restatements stay small.

Filler reads take no record and only push the offsets of the reads behind them; small test reads carry every record and are placed
so that a mark falls inside a test read's own range.  The documented layouts are mirrored here only to place reads, in Python
integers: a read of the pile-up owns lengths[r] + 1 slots rounded up to four (pileup_common.hpp), a read of the vote table 12 words
per base, plane p of a read of L bases lying p L words behind its first word (correct_kernels.hip), a read of the bases one byte
per base.  What a filler's result must be follows from the contracts and is written out here, not taken from the library; the
restatements run on the test reads alone, which works because records name ids, not indices.

The second half is the shift argument of the longest read a table takes: a read whose records lie in two windows, one at each end,
is the two windows judged apart and put together again, because the coverage between them is 0."""
import numpy as np

import repeat_ref
import trim_ref

M30, M31, M32 = 1 << 30, 1 << 31, 1 << 32
MARKS = (M30, M31, M32)
MIN_DEVICE_BYTES = 48 << 30     # a case may skip below this much device memory in total; an MI355X has 288 GB
LONGEST = (1 << 31) - 9         # the longest read the trimming and the repeat marking take


def pile_slots(length):
    return (int(length) + 4) & ~3


def pile_used(length):
    return int(length) + 1


def vote_words(length):
    return 12 * int(length)


def base_bytes(length):
    return int(length)


def largest_length(size_of, room, limit):
    """The greatest length in [0, limit] whose size is at most `room`, or -1."""
    if size_of(0) > room:
        return -1
    lo, hi = 0, int(limit)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if size_of(mid) <= room:
            lo = mid
        else:
            hi = mid - 1
    return lo


class Layout:
    """A table of reads: `lengths` of every entry in order, `filler[i]`, `starts[i]` (elements, Python integers), `total`, and
    `test[k]`: the entry of test read k."""

    def __init__(self, lengths, filler, size_of):
        self.lengths = [int(n) for n in lengths]
        self.filler = [bool(f) for f in filler]
        self.starts, at = [], 0
        for n in self.lengths:
            self.starts.append(at)
            at += size_of(n)
        self.total = at
        self.test = [i for i, f in enumerate(self.filler) if not f]
        self.fillers = [i for i, f in enumerate(self.filler) if f]

    def __len__(self):
        return len(self.lengths)

    def holder(self, mark, used_of):
        """(entry, offset of `mark` in the entry's own range), or None when the mark lies in no entry's used elements."""
        for i, (s, n) in enumerate(zip(self.starts, self.lengths)):
            if s <= mark < s + used_of(n):
                return i, mark - s
        return None

    def marks_inside_test_reads(self, marks, used_of, margin):
        """{mark: (test read k, offset)}; raises unless every mark lies in a test read's own range, `margin` elements from both of its
        ends.  A case that no longer crosses a mark fails here."""
        out = {}
        for mark in marks:
            hit = self.holder(mark, used_of)
            assert hit is not None, f"element {mark} lies in no read"
            i, o = hit
            assert not self.filler[i], f"element {mark} lies in filler entry {i}"
            assert margin <= o < used_of(self.lengths[i]) - margin, f"element {mark} lies {o} elements into entry {i}, too near an end"
            out[mark] = (self.test.index(i), o)
        return out


def place(test_lengths, straddlers, size_of, filler_max, fraction=0.5):
    """The layout of test reads and fillers: test read straddlers[mark] starts about `fraction` (one number, or {mark: number}) of its size in front of `mark`, the
    test reads between two straddlers follow the earlier one directly, those in front of the first stand at element 0 and those
    behind the last at the end.  Fillers of at most filler_max bases, as few as fit and about equally long, fill each gap."""
    lengths, filler, at, k = [], [], 0, 0

    def put(n, f):
        nonlocal at
        lengths.append(int(n))
        filler.append(f)
        at += size_of(n)

    for mark in sorted(straddlers):
        s = straddlers[mark]
        assert s >= k, "straddlers must ascend with their marks"
        while k < s:
            put(test_lengths[k], False)
            k += 1
        want = mark - int((fraction[mark] if isinstance(fraction, dict) else fraction) * size_of(test_lengths[s]))
        assert want >= at, f"no room in front of element {mark}"
        count = -(-(want - at) // size_of(filler_max))
        for i in range(count):
            n = largest_length(size_of, (want - at) // (count - i), filler_max)
            if n >= 1:
                put(n, True)
        put(test_lengths[s], False)
        k = s + 1
    while k < len(test_lengths):
        put(test_lengths[k], False)
        k += 1
    return Layout(lengths, filler, size_of)


# ---- what a table with fillers must give, from the restatement on the test reads alone -------------------------------------------------

def trim_with_fillers(layout, rows, flags, counts):
    """(rows, flags, counts) of the whole table: a filler has no eligible record, so its row is (0, 0, 0, 0) and it is deleted."""
    n = len(layout)
    full_rows, full_flags = np.zeros((n, 4), np.int32), np.full(n, trim_ref.DELETED, np.uint8)
    full_rows[layout.test], full_flags[layout.test] = rows, flags
    c = dict(counts)
    c["reads"] = n
    c["deleted"] = counts["deleted"] + len(layout.fillers)
    c["bases_in"] = counts["bases_in"] + sum(layout.lengths[i] for i in layout.fillers)
    return full_rows, full_flags, c


def repeat_with_fillers(layout, m):
    """The dict of repeat_ref.mark for the whole table: a filler has depth 0 everywhere, so no interval, flags 0, the row
    (0, 0, 0, -1), and its positions in bin 0, which the depth does not look at."""
    n = len(layout)
    rows, flags = np.zeros((n, 4), np.int32), np.zeros(n, np.uint8)
    rows[:, 3] = -1
    rows[layout.test], flags[layout.test] = m["rows"], m["flags"]
    per_read = np.zeros(n, np.int64)
    per_read[layout.test] = np.diff(m["offsets"])
    offsets = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64)
    filler_bases = sum(layout.lengths[i] for i in layout.fillers)
    hist = m["hist"].copy()
    hist[0] += filler_bases
    c = dict(m["counts"])
    c["reads"] = n
    c["bases"] = m["counts"]["bases"] + filler_bases
    return dict(rows=rows, flags=flags, offsets=offsets, intervals=m["intervals"], hist=hist, counts=c)


def correct_filler(read):
    """(sequence, stats) of a read nobody votes on: its own bytes, every position below any min_cov >= 1."""
    n = len(read)
    return bytes(read), [n, n, 0, 0, 0, n]


# ---- the shift argument: one long read as two windows ----------------------------------------------------------------------------------
# The folded table has three reads: window A (id A_ID, the long read's first W bases), window B (id B_ID, its last W bases, moved
# down by shift = long length - W) and the partner (id P_ID), which every record pairs a window with.  In the real table the long
# read has id A_ID and the partner P_ID.

A_ID, B_ID, P_ID = 1, 2, 3


def unfold(folded, long_len, W):
    """The folded records as records of the real table."""
    shift = int(long_len) - int(W)
    real = folded.copy()
    for idf, x1, x2, xl in (("from_id", "a1", "a2", "alen"), ("to_id", "b1", "b2", "blen")):
        in_a, in_b = folded[idf] == A_ID, folded[idf] == B_ID
        real[xl][in_a | in_b] = long_len
        real[x1][in_b] += shift
        real[x2][in_b] += shift
        real[idf][in_b] = A_ID
    return real


def trim_unfolded(folded, long_len, W, partner_len, P):
    """(rows, flags, counts) of the real table [long read, partner] from the restatement on the folded one.  The coverage between
    the windows is 0 and a window's slot behind its last base is the difference array's own: runs and covered positions add, the
    best run is the longer one, window A's on a tie (it comes first), and the flags follow from the clear range in the long read."""
    shift = int(long_len) - int(W)
    r3, f3, c3, _ = trim_ref.trim([A_ID, B_ID, P_ID], [W, W, partner_len], folded, P)
    live = [(int(r3[k, 1] - r3[k, 0]), -k, k) for k in (0, 1) if not f3[k] & trim_ref.DELETED]
    rows, flags = np.zeros((2, 4), np.int32), np.zeros(2, np.uint8)
    rows[1], flags[1] = r3[2], f3[2]
    if not live:
        flags[0] = trim_ref.DELETED
    else:
        k = max(live)[2]
        begin, end = int(r3[k, 0]) + (shift if k else 0), int(r3[k, 1]) + (shift if k else 0)
        runs = int(r3[0, 2] + r3[1, 2])
        rows[0] = (begin, end, runs, int(r3[0, 3] + r3[1, 3]))
        flags[0] = ((trim_ref.CUT5 if begin > 0 else 0) | (trim_ref.CUT3 if end < long_len else 0) | (trim_ref.GAPPED if runs > 1 else 0))
    c = dict(reads=2, deleted=int(((flags & trim_ref.DELETED) != 0).sum()), cut5=int(((flags & trim_ref.CUT5) != 0).sum()),
             cut3=int(((flags & trim_ref.CUT3) != 0).sum()), gapped=int(((flags & trim_ref.GAPPED) != 0).sum()),
             bases_in=int(long_len) + int(partner_len), bases_kept=int((rows[:, 1].astype(np.int64) - rows[:, 0]).sum()),
             eligible_records=c3["eligible_records"])
    return rows, flags, c


def repeat_unfolded(folded, long_len, W, partner_len, P):
    """The dict of repeat_ref.mark for the real table [long read, partner] from the restatement on the folded one: the positions
    between the windows have depth 0 and go into bin 0, which neither D nor T looks at; the long read's intervals are window A's
    followed by window B's moved up, and no interval is the whole read, which is longer than both windows."""
    assert 2 * int(W) < int(long_len)
    shift = int(long_len) - int(W)
    m = repeat_ref.mark([A_ID, B_ID, P_ID], [W, W, partner_len], folded, P)
    o = m["offsets"]
    iv_a, iv_b, iv_p = m["intervals"][o[0]:o[1]], m["intervals"][o[1]:o[2]] + shift, m["intervals"][o[2]:o[3]]
    n_long = len(iv_a) + len(iv_b)
    rows, flags = np.zeros((2, 4), np.int32), np.zeros(2, np.uint8)
    first = int(iv_a[0, 0]) if len(iv_a) else int(iv_b[0, 0]) if len(iv_b) else -1
    rows[0] = (n_long, int(m["rows"][0, 1] + m["rows"][1, 1]), int(max(m["rows"][0, 2], m["rows"][1, 2])), first)
    rows[1] = m["rows"][2]
    flags[0], flags[1] = (repeat_ref.SOME if n_long else 0), m["flags"][2]
    hist = m["hist"].copy()
    hist[0] += int(long_len) - 2 * int(W)
    c = dict(m["counts"])
    c.update(reads=2, reads_with_interval=int((flags & repeat_ref.SOME != 0).sum()), whole_reads=int((flags & repeat_ref.WHOLE != 0).sum()),
             bases=int(long_len) + int(partner_len))
    return dict(rows=rows, flags=flags, offsets=np.array([0, n_long, n_long + len(iv_p)], np.int64),
                intervals=np.concatenate([iv_a, iv_b, iv_p]).astype(np.int32).reshape(-1, 2), hist=hist, counts=c)


def window_records(rng, W, partner_len, runs, make, noise=0):
    """Folded records: runs = [(window id, begin, end, depth)]: `depth` records whose window side is [begin, end) and whose partner
    side is a random interval, identity 0.9; `noise` more with random intervals inside a random window and any identity.  make(from, to, a1, a2, alen, b1, b2, blen,
    to_rc, score) builds one record."""
    runs = [(wid, s, e, depth, 0.9) for wid, s, e, depth in runs]
    for _ in range(noise):     # (a score of 0 is no alignment, one of 0.4 lies below the min_identity the tests use)
        n = int(rng.integers(1, W // 3))
        s = int(rng.integers(0, W - n + 1))
        runs.append((int(rng.choice([A_ID, B_ID])), s, s + n, 1, float(rng.choice([0.0, 0.4, 0.9, 0.9]))))
    out = []
    for wid, s, e, depth, score in runs:
        for _ in range(depth):
            n = int(rng.integers(1, partner_len + 1))
            t = int(rng.integers(0, partner_len - n + 1))
            rc = int(rng.integers(0, 2))
            if rng.integers(0, 2):
                out.append(make(wid, P_ID, s, e - 1, W, t, t + n - 1, partner_len, rc, score))
            else:
                out.append(make(P_ID, wid, t, t + n - 1, partner_len, s, e - 1, W, rc, score))
    return out
