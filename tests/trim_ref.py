"""The "read trimming" contract of include/mhap_hip.h restated in plain Python / numpy, from the prose: eligible records, the
intervals they contribute, coverage by cumulative sum, runs, the clear range, the row and flags, the counts, and a record
rewritten onto the trimmed reads.  Python integers throughout (the header's int64), `//` on non-negative values for div."""
import numpy as np

DELETED, CUT5, CUT3, GAPPED = 1, 2, 4, 8
COUNTS = ("reads", "deleted", "cut5", "cut3", "gapped", "bases_in", "bases_kept", "eligible_records")
DEFAULTS = dict(min_cov=3, end_clip=500, min_span=2000, min_identity=0.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def eligible(rec, P):
    return int(rec["from_id"]) != int(rec["to_id"]) and float(rec["score"]) != 0.0 and not float(rec["score"]) < P["min_identity"]


def interval(x1, x2, P):
    """The interval one side contributes, or None."""
    s, e = int(x1) + P["end_clip"], int(x2) + 1 - P["end_clip"]
    return (s, e) if int(x2) + 1 - int(x1) >= P["min_span"] and e > s else None


def coverage(read_ids, lengths, records, P):
    """(cov, eligible records): cov[r] is an int64 array of lengths[r] positions.  The first read of an id is the read."""
    index = {}
    for r, i in enumerate(np.asarray(read_ids).tolist()):
        index.setdefault(i, r)
    diff = [np.zeros(int(n) + 1, np.int64) for n in lengths]
    n_el = 0
    for rec in records:
        if not eligible(rec, P):
            continue
        n_el += 1
        for idf, x1, x2 in (("from_id", "a1", "a2"), ("to_id", "b1", "b2")):
            iv = interval(rec[x1], rec[x2], P)
            if iv is not None:
                d = diff[index[int(rec[idf])]]
                d[iv[0]] += 1
                d[iv[1]] -= 1
    return [np.cumsum(d)[:-1] for d in diff], n_el


def runs_of(cov, min_cov):
    """The maximal stretches [s, e) with cov >= min_cov, in order."""
    inside = np.concatenate([[False], np.asarray(cov) >= min_cov, [False]])
    edges = np.flatnonzero(inside[1:] != inside[:-1])
    return list(zip(edges[0::2].tolist(), edges[1::2].tolist()))


def row_of(cov, length, P):
    """((begin, end, runs, covered), flags) of one read."""
    runs = runs_of(cov, P["min_cov"])
    if not runs:
        return (0, 0, 0, 0), DELETED
    s, e = max(runs, key=lambda r: (r[1] - r[0], -r[0]))
    begin, end = s - P["end_clip"], e + P["end_clip"]
    flags = (CUT5 if begin > 0 else 0) | (CUT3 if end < length else 0) | (GAPPED if len(runs) > 1 else 0)
    return (begin, end, len(runs), sum(b - a for a, b in runs)), flags


def trim(read_ids, lengths, records, P):
    """(rows int32 (n, 4), flags uint8 (n), counts dict, cov list)."""
    cov, n_el = coverage(read_ids, lengths, records, P)
    rows, flags = np.zeros((len(lengths), 4), np.int32), np.zeros(len(lengths), np.uint8)
    for r, n in enumerate(np.asarray(lengths).tolist()):
        rows[r], flags[r] = row_of(cov[r], n, P)
    c = dict(reads=len(lengths), deleted=int(((flags & DELETED) != 0).sum()), cut5=int(((flags & CUT5) != 0).sum()),
             cut3=int(((flags & CUT3) != 0).sum()), gapped=int(((flags & GAPPED) != 0).sum()),
             bases_in=int(np.asarray(lengths, np.int64).sum()), bases_kept=int((rows[:, 1].astype(np.int64) - rows[:, 0]).sum()),
             eligible_records=n_el)
    return rows, flags, c, cov


def clip_record(rec, clear_a, clear_b, P):
    """(kept, record): the record rewritten onto the clear ranges (begin, end) of its two reads; a void record comes back as it is."""
    out = rec.copy()
    ca, ea = int(clear_a[0]), int(clear_a[1])
    bb, be = int(clear_b[0]), int(clear_b[1])
    if not eligible(rec, P) or ea <= ca or be <= bb:
        return False, out
    a1, a2, b1, b2, blen, o = (int(rec[k]) for k in ("a1", "a2", "b1", "b2", "blen", "to_rc"))
    o = o != 0
    qs, qe = a1, a2 + 1
    ts, te = (blen - b2 - 1, blen - b1) if o else (b1, b2 + 1)
    cb, eb = (blen - be, blen - bb) if o else (bb, be)
    SQ, ST = qe - qs, te - ts
    if SQ <= 0 or ST <= 0:
        return False, out
    d5q, d5t, d3q, d3t = max(0, ca - qs), max(0, cb - ts), max(0, qe - ea), max(0, te - eb)
    s5q, s5t = max(d5q, d5t * SQ // ST), max(d5t, d5q * ST // SQ)
    s3q, s3t = max(d3q, d3t * SQ // ST), max(d3t, d3q * ST // SQ)
    qs2, qe2, ts2, te2 = qs + s5q, qe - s3q, ts + s5t, te - s3t
    if qe2 <= qs2 or te2 <= ts2:
        return False, out
    u, v, nb = ts2 - cb, te2 - cb, eb - cb
    out["a1"], out["a2"], out["alen"] = qs2 - ca, qe2 - 1 - ca, ea - ca
    out["b1"], out["b2"] = (nb - v, nb - u - 1) if o else (u, v - 1)
    out["blen"] = nb
    return True, out


def apply(read_ids, rows, flags, records, P):
    """(out, keep) of mhap_trim_apply."""
    index = {}
    for r, i in enumerate(np.asarray(read_ids).tolist()):
        index.setdefault(i, r)
    out, keep = records.copy(), np.zeros(len(records), np.uint8)
    for q, rec in enumerate(records):
        A, B = index[int(rec["from_id"])], index[int(rec["to_id"])]
        if (flags[A] | flags[B]) & DELETED:
            continue
        k, o = clip_record(rec, rows[A, :2], rows[B, :2], P)
        if k:
            out[q], keep[q] = o, 1
    return out, keep


def refine_record(rec, ops, penalty=2):
    """(refined, record): the record cut to the best stretch of its path under +1 per '=' column and -penalty per X, I or D column."""
    out = rec.copy()
    blen, o = int(rec["blen"]), int(rec["to_rc"]) != 0
    i, j = int(rec["a1"]), (blen - int(rec["b2"]) - 1 if o else int(rec["b1"]))
    cols = errs = total = best = 0
    start, found = None, None
    for op in np.asarray(ops).tolist():
        n, code = op >> 4, op & 15
        if code == 7:
            if total <= 0:
                total, start = 0, (i, j, cols, errs)
            total, i, j, cols = total + n, i + n, j + n, cols + n
            if total > best:
                best, found = total, (start[0], i, start[1], j, cols - start[2], errs - start[3])
        else:
            total, cols, errs = total - penalty * n, cols + n, errs + n
            i += n if code in (8, 1) else 0
            j += n if code in (8, 2) else 0
    if found is None:
        return False, out
    qs, qe, ts, te, c, e = found
    out["a1"], out["a2"] = qs, qe - 1
    out["b1"], out["b2"] = (blen - te, blen - ts - 1) if o else (ts, te - 1)
    out["score"] = 1.0 - e / c
    return True, out


def refine(records, op_offsets, ops, penalty=2):
    out = records.copy()
    for q in range(len(records)):
        out[q] = refine_record(records[q], ops[op_offsets[q]:op_offsets[q + 1]], penalty)[1]
    return out
