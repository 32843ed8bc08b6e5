"""The "overlap selection" contract of include/mhap_hip.h restated in plain Python / numpy, from the prose: eligible records, the two
views of a record and their keys, the per-read threshold with ties kept, the rows, the counts and a record's view byte.  The key is
IEEE double arithmetic (one multiply of an exact integer by min(score, 1) and one floor), which numpy's float64 does as C does.
Nothing here calls the library."""
import math

import numpy as np

SELECT_A, SELECT_B = 1, 2
COUNTS = ("reads", "reads_with_entry", "reads_over", "entries", "kept", "eligible_records")
DEFAULTS = dict(best_n=40, min_span=500, min_identity=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["best_n"] < 1 or p["min_span"] < 0:
        raise ValueError("best_n >= 1, min_span >= 0")
    return p


def eligible(rec, P):
    s = float(rec["score"])
    return int(rec["from_id"]) != int(rec["to_id"]) and s != 0.0 and not s < P["min_identity"] and s == s


def key(x1, x2, score, P):
    """The key of the view that spans x1 .. x2 of its read under `score`; 0: no such view."""
    span = int(x2) + 1 - int(x1)
    if span < P["min_span"]:
        return 0
    m = math.floor(float(span) * min(float(score), 1.0))   # (a product of two doubles: Python's float is C's double)
    return 1 + max(int(m), 0)


def judge_record(rec, P):
    """(kA, kB), both 0 for an ineligible record."""
    if not eligible(rec, P):
        return 0, 0
    return key(rec["a1"], rec["a2"], rec["score"], P), key(rec["b1"], rec["b2"], rec["score"], P)


def index_of(read_ids):
    index = {}
    for r, i in enumerate(np.asarray(read_ids).tolist()):
        index.setdefault(i, r)     # the first read of an id is the read
    return index


def keys_of(records, P):
    """(eligible, kA, kB) of every record, vectorised: bool and two int64 arrays (0: no such view)."""
    n = len(records)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, np.int64)
    s = records["score"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        el = (records["from_id"] != records["to_id"]) & (s != 0.0) & ~(s < P["min_identity"]) & (s == s)
        out = []
        for x1, x2 in (("a1", "a2"), ("b1", "b2")):
            span = records[x2].astype(np.int64) + 1 - records[x1].astype(np.int64)
            m = np.floor(span.astype(np.float64) * np.minimum(s, 1.0))
            k = 1 + np.maximum(np.where(m == m, m, 0.0), 0.0).astype(np.int64)
            out.append(np.where(el & (span >= P["min_span"]), k, 0))
    return el, out[0], out[1]


def select(read_ids, lengths, records, P):
    """A dict of rows (int32, n x 4: entries, kept, thr, greatest key), counts (a dict of COUNTS) and thr (int64 per read)."""
    n = len(read_ids)
    index = index_of(read_ids)
    el, ka, kb = keys_of(records, P)
    per = [[] for _ in range(n)]
    for ids, k in ((records["from_id"] if len(records) else [], ka), (records["to_id"] if len(records) else [], kb)):
        have = np.flatnonzero(k > 0)
        for i, key_ in zip(np.asarray(ids)[have].tolist(), k[have].tolist()):
            per[index[i]].append(key_)
    rows = np.zeros((n, 4), np.int32)
    thr = np.ones(n, np.int64)
    over = 0
    for r, ks in enumerate(per):
        E = len(ks)
        if E == 0:
            rows[r] = (0, 0, 1, 0)
            continue
        a = np.sort(np.array(ks, np.int64))[::-1]
        if E > P["best_n"]:
            thr[r] = int(a[P["best_n"] - 1])     # the best_n-th greatest, with multiplicity
            over += 1
        rows[r] = (E, int((a >= thr[r]).sum()), thr[r], int(a[0]))
    counts = dict(reads=n, reads_with_entry=int((rows[:, 0] > 0).sum()), reads_over=over, entries=int(rows[:, 0].sum()),
                  kept=int(rows[:, 1].sum()), eligible_records=int(el.sum()))
    return dict(rows=rows, counts=counts, thr=thr)


def apply(read_ids, thr, records, P):
    """One byte per record: bit 0 view A kept, bit 1 view B kept."""
    index = index_of(read_ids)
    el, ka, kb = keys_of(records, P)
    out = np.zeros(len(records), np.uint8)
    if len(records) == 0:
        return out
    ta = np.array([thr[index[i]] for i in records["from_id"].tolist()], np.int64)
    tb = np.array([thr[index[i]] for i in records["to_id"].tolist()], np.int64)
    out |= np.where((ka > 0) & (ka >= ta), SELECT_A, 0).astype(np.uint8)
    out |= np.where((kb > 0) & (kb >= tb), SELECT_B, 0).astype(np.uint8)
    return out


def table_text(read_ids, rows):
    """The --table / --best-table file: one line per read, `read_id entries kept threshold`."""
    return "".join(f"{int(i)} {int(r[0])} {int(r[1])} {int(r[2])}\n" for i, r in zip(np.asarray(read_ids).tolist(), rows))


def counts_line(c):
    """The one stderr line of a selection; c: a dict of COUNTS."""
    return (f"Best overlaps: {c['reads']} reads, {c['reads_with_entry']} with a view, {c['reads_over']} cut; "
            f"{c['kept']} of {c['entries']} views kept; {c['eligible_records']} eligible overlaps")
