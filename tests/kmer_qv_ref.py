"""Sequence assessment restated from its contract (include/mhap_hip.h, "Sequence assessment without a reference") on Python sets and
lists: the count histogram's valley, the set of solid k-mers, a sequence's row and intervals against a set, the two files, the set
comparison and the QV arithmetic.  Written from the contract, one window and one position at a time; nothing here knows about tiles,
lanes or bitmaps."""
import collections
import math

_RC = str.maketrans("ACGT", "TGCA")


def window_key(seq, i, k, canonical):
    """The k-mer of window [i, i + k) as a string (canonical: the smaller of it and its reverse complement), or None when one of its
    k bytes is not A, C, G or T (upper case)."""
    w = seq[i:i + k]
    if len(w) != k or any(c not in "ACGT" for c in w):
        return None
    if canonical:
        r = w.translate(_RC)[::-1]
        return min(w, r)   # (string order = value order: A < C < G < T, first base most significant)
    return w


def key_value(key):
    v = 0
    for c in key:
        v = v * 4 + "ACGT".index(c)
    return v


def count(seqs, k, canonical):
    cnt = collections.Counter()
    for s in seqs:
        for i in range(len(s) - k + 1):
            key = window_key(s, i, k, canonical)
            if key is not None:
                cnt[key] += 1
    return cnt


def valley(hist):
    """hist: {count: number of distinct k-mers with that count}.  The smallest c >= 1 with n[c + 1] >= n[c] (n = 0 where absent)."""
    c = 1
    while not hist.get(c + 1, 0) >= hist.get(c, 0):
        c += 1
    return c


def histogram(cnt):
    return dict(collections.Counter(cnt.values()))


def solid(cnt, min_count):
    """(the set, the min_count used): the keys counted at least min_count times; min_count 0 = the valley of the histogram."""
    if min_count == 0:
        min_count = valley(histogram(cnt))
    return {key for key, c in cnt.items() if c >= min_count}, min_count


def evaluate(seq, kset, k, canonical):
    """(row, intervals) of one sequence: row = [bases, windows, missing, runs, unsupported], intervals = [(begin, end), ...]."""
    n = len(seq)
    nw = max(n - k + 1, 0)
    valid, present, missing = [False] * nw, [False] * nw, [False] * nw
    for i in range(nw):
        key = window_key(seq, i, k, canonical)
        valid[i] = key is not None
        present[i] = valid[i] and key in kset
        missing[i] = valid[i] and key not in kset
    runs = sum(1 for i in range(nw) if missing[i] and (i == 0 or not missing[i - 1]))
    # windows [0, i) that are valid / present, so that "some window in [a, b] is ..." is one subtraction
    nvalid, npresent = [0], [0]
    for i in range(nw):
        nvalid.append(nvalid[-1] + valid[i])
        npresent.append(npresent[-1] + present[i])
    unsupported = []
    for p in range(n):
        a, b = max(0, p - k + 1), min(p, nw - 1)   # the windows that contain p (none when a > b)
        some_valid = a <= b and nvalid[b + 1] - nvalid[a] > 0
        some_present = a <= b and npresent[b + 1] - npresent[a] > 0
        unsupported.append(some_valid and not some_present)
    intervals, p = [], 0
    while p < n:
        if unsupported[p]:
            b = p
            while p < n and unsupported[p]:
                p += 1
            intervals.append((b, p))
        else:
            p += 1
    return [n, sum(valid), sum(missing), runs, sum(unsupported)], intervals


def evaluate_all(seqs, kset, k, canonical):
    """(rows, intervals as (sequence index, begin, end))"""
    rows, ivs = [], []
    for j, s in enumerate(seqs):
        r, iv = evaluate(s, kset, k, canonical)
        rows.append(r)
        ivs += [(j, b, e) for b, e in iv]
    return rows, ivs


def qv(windows, missing, k):
    """(error, qv): error = 1 - (1 - missing / windows)^(1 / k), qv = -10 log10(error); no windows: NaN; nothing missing: (0, inf)."""
    if windows == 0:
        return math.nan, math.nan
    if missing == 0:
        return 0.0, math.inf
    e = 1.0 - (1.0 - missing / windows) ** (1.0 / k)
    return e, 0.0 - 10.0 * math.log10(e)


def _line(name, r, k):
    e, q = qv(r[1], r[2], k)
    return "%s\t%d\t%d\t%d\t%d\t%d\t%.6e\t%.2f\n" % (name, r[0], r[1], r[2], r[3], r[4], e, q)


def table(rows, k, names=None):
    names = names if names is not None else ["seq%d" % (i + 1) for i in range(len(rows))]
    tot = [sum(r[f] for r in rows) for f in range(5)]
    return "".join(_line(nm, r, k) for nm, r in zip(names, rows)) + _line("total", tot, k)


def bed(intervals, nseq, names=None):
    names = names if names is not None else ["seq%d" % (i + 1) for i in range(nseq)]
    return "".join("%s\t%d\t%d\n" % (names[j], b, e) for j, b, e in intervals)


def compare(a, b):
    return len(a), len(b), len(a & b)
