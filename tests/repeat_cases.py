"""Inputs of the "repeat marking" contract: hand-computed tables, crafted judgement cases, and a generator of exact records over a
genome with a planted repeat, which also says which records are false.  Shared by tests/test_repeat_cpu.py (the restatement
tests/repeat_ref.py and the host entry point) and tests/test_repeat_gpu.py (the GPU)."""
import numpy as np

from trim_cases import rec, recs


# ---- hand-computed tables: (lengths, [(read, begin, end) intervals piled up], parameters) -> depth, threshold, intervals per read ----
def pile(lengths, intervals, partner_len=None):
    """(ids, lengths, records): one record per (read, s, e) against a partner read appended to the table, which gets [0, 1) each
    time.  The partner is the last read; its pile-up is one position of depth len(intervals)."""
    lengths = list(lengths) + [partner_len or 1]
    ids = np.arange(1, len(lengths) + 1, dtype=np.int64)
    partner = len(lengths)
    out = [rec(r + 1, partner, s, e - 1, lengths[r], 0, 0, lengths[-1], k & 1, 1.0) for k, (r, s, e) in enumerate(intervals)]
    return ids, np.array(lengths, np.int32), recs(out)


def stack(r, s, e, depth):
    return [(r, s, e)] * depth


# Every table has the partner's single position on top: one position of depth len(intervals), which the expectations count.
HAND = {
    # depths 1 x 10, 2 x 10 on read 0 and the partner's 1 position at depth 2: N1 = 21, hist[1] = 10 -> 20 < 21, + hist[2] = 21 -> D = 2
    "median above a tie": dict(lengths=[30], iv=[(0, 0, 20), (0, 10, 20)], P=dict(min_run=1), D=2, T=4, intervals=[[], []]),
    # depths 1 x 11 (read 0), 3 x 10 (read 1), partner 1 position at depth 4 -> N1 = 22, 2 * 11 >= 22 at c = 1: the lower median
    "a tie of the lower median": dict(lengths=[30, 30], iv=[(0, 0, 11)] + stack(1, 0, 10, 3), P=dict(min_run=1), D=1, T=2,
                                      intervals=[[], [(0, 10)], [(0, 1)]]),
    # D = 2 (41 positions at 2, 6 at 4, 6 at 5, partner at 13), factor 200 -> T = 4: depth 4 is not a repeat, depth 5 is
    "cov == T against T + 1": dict(lengths=[100], iv=stack(0, 0, 40, 2) + stack(0, 50, 56, 4) + stack(0, 60, 66, 5) + stack(0, 90, 91, 2),
                                   P=dict(min_run=1), D=2, T=4, intervals=[[(60, 66)], [(0, 1)]]),
    # runs of 5, 4 and (open at the read's end) 4 positions at depth 3 over depth 1, min_run 5; the partner's run of 1 is too short
    "min_run exact and min_run - 1": dict(lengths=[100], iv=[(0, 0, 100)] + stack(0, 10, 15, 2) + stack(0, 20, 24, 2) + stack(0, 96, 100, 2),
                                          P=dict(min_run=5), D=1, T=2, intervals=[[(10, 15)], []]),
    # the same pile with max_cov 2 given: what the derived T = 2 gives; with max_cov 3 nothing on read 0 is above it
    "max_cov 2 given": dict(lengths=[100], iv=[(0, 0, 100)] + stack(0, 10, 15, 2) + stack(0, 20, 24, 2), P=dict(min_run=4, max_cov=2, factor_pct=400),
                            D=1, T=2, intervals=[[(10, 15), (20, 24)], []]),
    "max_cov 3 given": dict(lengths=[100], iv=[(0, 0, 100)] + stack(0, 10, 15, 2) + stack(0, 20, 24, 2), P=dict(min_run=1, max_cov=3),
                            D=1, T=3, intervals=[[], [(0, 1)]]),
    "derived against given": dict(lengths=[100], iv=[(0, 0, 100)] + stack(0, 10, 15, 2) + stack(0, 20, 24, 2), P=dict(min_run=1, factor_pct=400),
                                  D=1, T=4, intervals=[[], [(0, 1)]]),
    "no record at all": dict(lengths=[10, 0], iv=[], P=dict(min_run=1), D=0, T=0, intervals=[[], [], []]),
    # the whole of a read above T
    "the whole read": dict(lengths=[8, 50], iv=stack(0, 0, 8, 5) + [(1, 0, 50)], P=dict(min_run=8), D=1, T=2, intervals=[[(0, 8)], [], []]),
}


def hand_case(name):
    c = HAND[name]
    ids, lengths, records = pile(c["lengths"], c["iv"])
    return ids, lengths, records, c


def clamp_case(depth=5000):
    """One read whose 3 positions all have `depth` intervals: every covered position falls into the last bin."""
    ids, lengths = np.array([1, 2], np.int64), np.array([3, 3], np.int32)
    return ids, lengths, np.repeat(recs([rec(1, 2, 0, 2, 3, 0, 2, 3, 0, 1.0)]), depth)


# ---- crafted judgements: explicit interval lists, records laid against their edges ----
JUDGE_P = dict(max_cov=1, min_run=10, min_unique=100, min_identity=0.5)
JUDGE_IDS = np.array([1, 2, 3, 4], np.int64)                    # A, B, the fillers' partner, a read with 1 000 intervals
JUDGE_LEN = np.array([20000, 20000, 30000, 20010], np.int32)
JUDGE_IV = {
    1: [(1000, 2000), (3000, 3500), (8000, 12000)],
    2: [(0, 700), (19000, 20000)],
    4: [(20 * i + 5, 20 * i + 15) for i in range(1000)],
}


def judge_fillers():
    """Records that pile depth 2 onto exactly the intervals of JUDGE_IV (and onto read 3, whose intervals are what they are)."""
    out, at = [], 0
    for rid, ivs in JUDGE_IV.items():
        L = int(JUDGE_LEN[rid - 1])
        for s, e in ivs:
            out += [rec(rid, 3, s, e - 1, L, at, at + e - s - 1, 30000, 0, 0.9)] * 2
            at = (at + e - s + 7) % 20000
    return recs(out)


def judge_records():
    """[(record, keep, uA, uB)]: the expectations are worked out by hand from JUDGE_IV with min_unique 100."""
    A, B, K = 20000, 20000, 20010
    out = []
    for o in (0, 1):
        out += [
            (rec(1, 2, 2000, 2999, A, 5000, 5999, B, o), 1, 1000, 1000),        # abuts the end of one interval and the begin of the next
            (rec(1, 2, 1999, 3000, A, 5000, 6001, B, o), 1, 1000, 1002),        # one position into both
            (rec(1, 2, 500, 12999, A, 700, 13199, B, o), 1, 12500 - 5500, 12500),   # spans all three of A; abuts B's first
            (rec(1, 2, 8000, 11999, A, 3000, 6999, B, o), 0, 0, 4000),          # an interval exactly
            (rec(1, 2, 4000, 4999, A, 0, 799, B, o), 1, 1000, 100),             # u == min_unique
            (rec(1, 2, 4000, 4999, A, 0, 798, B, o), 0, 1000, 99),              # min_unique - 1
            (rec(2, 1, 18901, 19999, B, 7901, 8999, A, o), 0, 99, 99),          # both sides one short
            (rec(2, 1, 18900, 19999, B, 7900, 8999, A, o), 1, 100, 100),
            (rec(4, 2, 0, 20009, K, 1000, 18999, B, o), 1, 10010, 18000),       # all 1 000 intervals
            (rec(4, 2, 10, 10009, K, 1000, 10999, B, o), 1, 5000, 10000),       # from inside the first (5 of it) to 10 010: 5 + 499 * 10 + 5 inside
            (rec(4, 2, 19985, 20004, K, 1000, 1019, B, o), 0, 10, 20),          # the last interval and its flanks
        ]
    out += [
        (rec(1, 1, 8000, 11999, A, 8000, 11999, A), 1, -1, -1),                 # a read against itself
        (rec(1, 2, 8000, 11999, A, 0, 699, B, 0, 0.0), 1, -1, -1),              # no alignment
        (rec(1, 2, 8000, 11999, A, 0, 699, B, 0, 0.4), 1, -1, -1),              # below min_identity
    ]
    return out


# ---- the generator: exact records over a genome with one repeat family, and which of them are false ----
def generate(seed, G=200000, copies=(20000, 70000, 120000, 170000), repeat=4000, depth=20, min_overlap=1000):
    """(ids, lengths, records, false, anchor): error-free forward records between every two reads that share at least min_overlap
    genome bases (true), and between every read on one copy of the repeat and every read on another whose spans of the repeat, in
    the repeat's coordinates, share at least min_overlap (false).  anchor[q], for a true record, is the lesser over its two reads
    of the aligned bases outside every copy (both reads align the same genome bases, so the two are equal); -1 for a false one."""
    rng = np.random.default_rng(seed)
    n = depth * G // 8000
    start = rng.integers(0, G - 8000, n)
    length = np.clip(rng.normal(8000, 1500, n).astype(np.int64), 3000, G - start)
    end = start + length
    ids = np.arange(1, n + 1, dtype=np.int64)
    out, false, anchor = [], [], []
    order = np.argsort(start, kind="stable")
    for x in range(n):
        i = int(order[x])
        for y in range(x + 1, n):
            j = int(order[y])
            if start[j] >= end[i]:
                break
            lo, hi = int(max(start[i], start[j])), int(min(end[i], end[j]))
            if hi - lo < min_overlap:
                continue
            a, b = (i, j) if i < j else (j, i)
            out.append(rec(int(ids[a]), int(ids[b]), lo - int(start[a]), hi - 1 - int(start[a]), int(length[a]), lo - int(start[b]),
                           hi - 1 - int(start[b]), int(length[b]), 0, 1.0))
            false.append(False)
            anchor.append((hi - lo) - sum(max(0, min(hi, c + repeat) - max(lo, c)) for c in copies))
    on = []     # (read, copy, the read's span of the repeat in the repeat's coordinates)
    for i in range(n):
        for k, c in enumerate(copies):
            s, e = max(int(start[i]), c), min(int(end[i]), c + repeat)
            if e > s:
                on.append((i, k, s - c, e - c))
    for i, ki, si, ei in on:
        for j, kj, sj, ej in on:
            if ki == kj or i >= j:
                continue
            lo, hi = max(si, sj), min(ei, ej)
            if hi - lo < min_overlap:
                continue
            pa, pb = copies[ki] + lo - int(start[i]), copies[kj] + lo - int(start[j])
            out.append(rec(int(ids[i]), int(ids[j]), pa, pa + hi - lo - 1, int(length[i]), pb, pb + hi - lo - 1, int(length[j]), 0, 1.0))
            false.append(True)
            anchor.append(-1)
    return ids, length.astype(np.int32), recs(out), np.array(false, bool), np.array(anchor, np.int64)
