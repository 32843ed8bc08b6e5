"""The "repeat marking" contract of include/mhap_hip.h restated in plain Python / numpy, from the prose: eligible records, coverage
by cumulative sum, the histogram and the typical depth, the threshold, the repeat intervals, the rows, flags and counts, and a
record's judgement.  Python integers throughout (the header's int64), `//` on non-negative values for div.  Nothing here calls the
library."""
import numpy as np

SOME, WHOLE = 1, 2
BINS = 4096
COUNTS = ("reads", "reads_with_interval", "whole_reads", "intervals", "repeat_bases", "bases", "eligible_records", "depth", "threshold")
DEFAULTS = dict(factor_pct=200, max_cov=0, min_run=500, min_unique=500, min_identity=0.0)


class NeedMaxCov(Exception):
    """The typical depth sits in the last bin and no max_cov was given."""


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["factor_pct"] < 100 or p["max_cov"] < 0 or p["min_run"] < 1 or p["min_unique"] < 0:
        raise ValueError("factor_pct >= 100, max_cov >= 0, min_run >= 1, min_unique >= 0")
    return p


def eligible(rec, P):
    return int(rec["from_id"]) != int(rec["to_id"]) and float(rec["score"]) != 0.0 and not float(rec["score"]) < P["min_identity"]


def index_of(read_ids):
    index = {}
    for r, i in enumerate(np.asarray(read_ids).tolist()):
        index.setdefault(i, r)     # the first read of an id is the read
    return index


def coverage(read_ids, lengths, records, P):
    """(cov, eligible records): cov[r] is an int64 array of lengths[r] positions."""
    index = index_of(read_ids)
    diff = [np.zeros(int(n) + 1, np.int64) for n in lengths]
    el = np.array([eligible(rec, P) for rec in records], bool) if len(records) else np.zeros(0, bool)
    for idf, x1, x2 in (("from_id", "a1", "a2"), ("to_id", "b1", "b2")):
        for i, s, e in zip(records[idf][el].tolist(), records[x1][el].tolist(), records[x2][el].tolist()):
            d = diff[index[i]]
            d[s] += 1
            d[e + 1] -= 1
    return [np.cumsum(d)[:-1] for d in diff], int(el.sum())


def histogram(cov):
    hist = np.zeros(BINS, np.int64)
    for c in cov:
        if len(c):
            hist += np.bincount(np.minimum(c, BINS - 1), minlength=BINS)
    return hist


def depth(hist):
    """D: the smallest c >= 1 with 2 (hist[1] + ... + hist[c]) >= N1; 0 when N1 == 0."""
    n1 = int(hist[1:].sum())
    if n1 == 0:
        return 0
    acc = 0
    for c in range(1, BINS):
        acc += int(hist[c])
        if 2 * acc >= n1:
            return c
    raise AssertionError("unreachable")


def threshold(D, P):
    if P["max_cov"] > 0:
        return P["max_cov"]
    if D == BINS - 1:
        raise NeedMaxCov()
    return D * P["factor_pct"] // 100


def intervals_of(cov, T, min_run):
    """The maximal runs [s, e) of positions with cov > T that have at least min_run positions, ascending."""
    inside = np.concatenate([[False], np.asarray(cov) > T, [False]])
    edges = np.flatnonzero(inside[1:] != inside[:-1])
    return [(s, e) for s, e in zip(edges[0::2].tolist(), edges[1::2].tolist()) if e - s >= min_run]


def mark(read_ids, lengths, records, P):
    """A dict: rows int32 (n, 4), flags uint8 (n), offsets int64 (n + 1), intervals int32 (m, 2), hist int64 (BINS), counts, cov."""
    cov, n_el = coverage(read_ids, lengths, records, P)
    hist = histogram(cov)
    D = depth(hist)
    T = threshold(D, P)
    n = len(lengths)
    rows, flags, offsets, ivs = np.zeros((n, 4), np.int32), np.zeros(n, np.uint8), np.zeros(n + 1, np.int64), []
    for r, L in enumerate(np.asarray(lengths).tolist()):
        iv = intervals_of(cov[r], T, P["min_run"])
        ivs += iv
        offsets[r + 1] = offsets[r] + len(iv)
        rows[r] = (len(iv), sum(e - s for s, e in iv), int(cov[r].max()) if L else 0, iv[0][0] if iv else -1)
        flags[r] = (SOME if iv else 0) | (WHOLE if iv == [(0, L)] else 0)
    c = dict(reads=n, reads_with_interval=int((flags & SOME != 0).sum()), whole_reads=int((flags & WHOLE != 0).sum()), intervals=len(ivs),
             repeat_bases=int(rows[:, 1].astype(np.int64).sum()), bases=int(np.asarray(lengths, np.int64).sum()), eligible_records=n_el,
             depth=D, threshold=T)
    return dict(rows=rows, flags=flags, offsets=offsets, intervals=np.array(ivs, np.int32).reshape(-1, 2), hist=hist, counts=c, cov=cov)


def unique_bases(x1, x2, intervals):
    """The positions of [x1, x2 + 1) outside every interval."""
    s, e = int(x1), int(x2) + 1
    return (e - s) - sum(max(0, min(e, int(b)) - max(s, int(a))) for a, b in intervals)


def judge_record(rec, intervals_a, intervals_b, P):
    """(keep, uA, uB)."""
    if not eligible(rec, P):
        return 1, -1, -1
    ua, ub = unique_bases(rec["a1"], rec["a2"], intervals_a), unique_bases(rec["b1"], rec["b2"], intervals_b)
    return int(ua >= P["min_unique"] and ub >= P["min_unique"]), ua, ub


def apply(read_ids, offsets, intervals, records, P):
    """(keep uint8 (n), unique int32 (n, 2)) of mhap_repeat_apply; vectorised: the inside of [s, e) is F(e) - F(s) with F the
    running count of interval positions of the read."""
    index = index_of(read_ids)
    keep, unique = np.ones(len(records), np.uint8), np.full((len(records), 2), -1, np.int32)
    per_read = {}
    for q, rec in enumerate(records):
        if not eligible(rec, P):
            continue
        for f, (idf, x1, x2) in enumerate((("from_id", "a1", "a2"), ("to_id", "b1", "b2"))):
            r = index[int(rec[idf])]
            if r not in per_read:
                per_read[r] = intervals[offsets[r]:offsets[r + 1]].tolist()
            iv = per_read[r]
            unique[q, f] = unique_bases(rec[x1], rec[x2], iv) if len(iv) < 8 else _unique_many(rec[x1], rec[x2], iv)
        keep[q] = int(unique[q, 0] >= P["min_unique"] and unique[q, 1] >= P["min_unique"])
    return keep, unique


def _unique_many(x1, x2, iv):
    a = np.asarray(iv, np.int64)
    s, e = int(x1), int(x2) + 1
    return int((e - s) - np.clip(np.minimum(e, a[:, 1]) - np.maximum(s, a[:, 0]), 0, None).sum())
