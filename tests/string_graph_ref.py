"""The string-graph contract restated in Python from the prose of include/mhap_hip.h ("string graph"): the class of a realigned record,
the two arcs of a dovetail, contained reads, the de-duplicated arc list, the per-vertex reduction and the final arcs, with the GFA text.
Plain loops over Python integers; nothing here calls the library.  Also the fabricated inputs of the tests: records made from reads
placed on a line (no bases are needed), and hand-made records."""
import numpy as np

RECORD_DTYPE = np.dtype([("from_id", "<i8"), ("to_id", "<i8"), ("score", "<f8"), ("raw", "<f8"), ("a1", "<i4"), ("a2", "<i4"),
                         ("alen", "<i4"), ("b1", "<i4"), ("b2", "<i4"), ("blen", "<i4"), ("to_rc", "<i4"), ("pad", "<i4")])

NONE, INTERNAL, A_CONTAINED, B_CONTAINED, SHORT, DOVETAIL = range(6)
CLASS_NAMES = ("none", "internal", "a_contained", "b_contained", "short", "dovetail")
IN_PLAY, ELIMINATED = 1, 2


class Params:
    def __init__(self, max_hang=1000, int_frac_permille=800, min_ovlp=2000, fuzz=1000, min_identity=0.0):
        self.max_hang, self.int_frac_permille, self.min_ovlp, self.fuzz, self.min_identity = max_hang, int_frac_permille, min_ovlp, fuzz, min_identity


def classify(r, A, B, p):
    """(class, arcs) of one record whose reads have the indices A and B: arcs is [] or the two (u, v, len) of a dovetail."""
    if int(r["from_id"]) == int(r["to_id"]) or float(r["score"]) == 0.0 or float(r["score"]) < p.min_identity:
        return NONE, []
    qs, qe, ql, tl, o = int(r["a1"]), int(r["a2"]) + 1, int(r["alen"]), int(r["blen"]), 1 if int(r["to_rc"]) else 0
    b1, b2 = int(r["b1"]), int(r["b2"])
    ts, te = (b1, b2 + 1) if not o else (tl - b2 - 1, tl - b1)
    tl5, tl3 = ts, tl - te
    ext5, ext3 = min(qs, tl5), min(ql - qe, tl3)
    if ext5 > p.max_hang or ext3 > p.max_hang or (qe - qs) * 1000 < (qe - qs + ext5 + ext3) * p.int_frac_permille:
        return INTERNAL, []
    if qs <= tl5 and ql - qe <= tl3:
        return A_CONTAINED, []
    if qs >= tl5 and ql - qe >= tl3:
        return B_CONTAINED, []
    if qe - qs + ext5 + ext3 < p.min_ovlp or te - ts + ext5 + ext3 < p.min_ovlp:
        return SHORT, []
    if qs > tl5:
        return DOVETAIL, [(2 * A, 2 * B + o, qs - tl5), (2 * B + (1 - o), 2 * A + 1, tl3 - (ql - qe))]
    return DOVETAIL, [(2 * B + o, 2 * A, tl5 - qs), (2 * A + 1, 2 * B + (1 - o), (ql - qe) - tl3)]


class Graph:
    """read_ids, lengths: the table of reads.  add() any number of times, then finish(); both may be repeated."""

    def __init__(self, read_ids, lengths, params=None):
        self.ids = [int(x) for x in read_ids]
        self.lengths = [int(x) for x in lengths]
        self.p = params or Params()
        self.by_id = {}
        for i, x in enumerate(self.ids):
            self.by_id.setdefault(x, i)          # the first read of an id wins
        self.classes = []
        self.contained = [0] * len(self.ids)
        self.raw = []                            # (u, v, len, q) of every dovetail so far

    def add(self, recs):
        recs = np.asarray(recs, dtype=RECORD_DTYPE)
        idx = []
        for q, r in enumerate(recs):
            pair = []
            for fid, flen in ((int(r["from_id"]), int(r["alen"])), (int(r["to_id"]), int(r["blen"]))):
                if fid not in self.by_id:
                    raise ValueError(f"record {q} names read {fid}, which is not among the reads")
                if self.lengths[self.by_id[fid]] != flen:
                    raise ValueError(f"record {q} gives read {fid} the length {flen}, the reads say {self.lengths[self.by_id[fid]]}")
                pair.append(self.by_id[fid])
            idx.append(pair)
        for r, (A, B) in zip(recs, idx):
            q = len(self.classes)
            c, arcs = classify(r, A, B, self.p)
            self.classes.append(c)
            if c == A_CONTAINED:
                self.contained[A] = 1
            if c == B_CONTAINED:
                self.contained[B] = 1
            self.raw += [(u, v, ln, q) for u, v, ln in arcs]

    def finish(self):
        """rows: the de-duplicated arc list as [u, v, len, ol, q, reduced, final]; counts: a dict."""
        live = [a for a in self.raw if not self.contained[a[0] >> 1] and not self.contained[a[1] >> 1]]
        live.sort(key=lambda a: (a[0], a[2], a[1]))
        arcs, seen = [], set()
        for u, v, ln, q in live:
            if (u, v) not in seen:
                seen.add((u, v))
                arcs.append((u, v, ln, q))
        out = {}                                  # u -> [(v, len, index in arcs)] in list order
        for i, (u, v, ln, q) in enumerate(arcs):
            out.setdefault(u, []).append((v, ln, i))
        reduced = [0] * len(arcs)
        fuzz = self.p.fuzz
        for v, ws in out.items():
            mark = {w: IN_PLAY for w, _, _ in ws}
            longest = ws[-1][1] + fuzz
            for w, ln, _ in ws:                   # pass 1
                if mark[w] != IN_PLAY:
                    continue
                for x, l2, _ in out.get(w, []):
                    if ln + l2 > longest:
                        break
                    if mark.get(x) == IN_PLAY:
                        mark[x] = ELIMINATED
            for w, ln, _ in ws:                   # pass 2
                for k, (x, l2, _) in enumerate(out.get(w, [])):
                    if k > 0 and l2 >= fuzz:
                        break
                    if mark.get(x) == IN_PLAY:
                        mark[x] = ELIMINATED
            for w, _, i in ws:
                if mark[w] == ELIMINATED:
                    reduced[i] = 1
        where = {(u, v): i for i, (u, v, _, _) in enumerate(arcs)}
        rows = []
        for i, (u, v, ln, q) in enumerate(arcs):
            comp = where[(v ^ 1, u ^ 1)]          # always there
            rows.append([u, v, ln, self.lengths[u >> 1] - ln, q, reduced[i], int(not reduced[i] and not reduced[comp])])
        self.rows = rows
        counts = {"records": len(self.classes)}
        for c, name in enumerate(CLASS_NAMES):
            counts[name] = self.classes.count(c)
        counts.update(contained_reads=sum(self.contained), arcs=len(rows), reduced=sum(r[5] for r in rows), final=sum(r[6] for r in rows))
        self.counts = counts
        return rows, counts

    def gfa(self):
        return gfa_text(self.ids, self.lengths, self.contained, self.rows)


COUNT_NAMES = ("records",) + CLASS_NAMES + ("contained_reads", "arcs", "reduced", "final")


def gfa_link(row, ids):
    u, v, ol = row[0], row[1], row[3]
    return f"L\t{ids[u >> 1]}\t{'-' if u & 1 else '+'}\t{ids[v >> 1]}\t{'-' if v & 1 else '+'}\t{ol}M"


def gfa_text(ids, lengths, contained, rows):
    out = ["H\tVN:Z:1.0"]
    out += [f"S\t{i}\t*\tLN:i:{n}" for i, n, c in zip(ids, lengths, contained) if not c]
    out += [gfa_link(r, ids) for r in rows if r[6]]
    return "".join(line + "\n" for line in out)


def strip_q(rows):
    """The arc table without its labels."""
    return [[r[0], r[1], r[2], r[3], r[5], r[6]] for r in np.asarray(rows, dtype=np.int64).reshape(-1, 7).tolist()]


# ---- fabricated inputs ------------------------------------------------------------------------------------------------------------------

def record(fid, tid, a1, a2, alen, b1, b2, blen, rc, score=0.9):
    """One realigned record; b1, b2 on the `to` read's own strand, as the realignment stage leaves them."""
    r = np.zeros(1, RECORD_DTYPE)
    r[0] = (fid, tid, score, 0.0, a1, a2, alen, b1, b2, blen, rc, 0)
    return r


def placed(fid, tid, A, B, trim=(0, 0, 0, 0), score=0.9):
    """The record of two reads placed on a line: A, B = (start, end, strand) with strand 0 forward, 1 reverse; the alignment is the
    shared interval, shortened by trim = (A's left, A's right, B's left, B's right) line positions.  None when nothing is shared."""
    (sa, ea, fa), (sb, eb, fb) = A, B
    lo, hi = max(sa, sb), min(ea, eb)
    alo, ahi, blo, bhi = lo + trim[0], hi - trim[1], lo + trim[2], hi - trim[3]
    if ahi - alo < 1 or bhi - blo < 1:
        return None
    a1, a2 = (alo - sa, ahi - sa - 1) if not fa else (ea - ahi, ea - alo - 1)
    b1, b2 = (blo - sb, bhi - sb - 1) if not fb else (eb - bhi, eb - blo - 1)
    return record(fid, tid, a1, a2, ea - sa, b1, b2, eb - sb, int(fa != fb), score)


def layout(seed, n_reads=150, genome=120000, lo=3000, hi=9000, jitter=0):
    """Reads on a line, both strands, and one record for every two reads that share at least 500 positions: which read is `from`
    is drawn, and the alignment falls short of the shared interval by 0 .. jitter positions at either end.
    Returns (read_ids, lengths, reads [(start, end, strand)], records)."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        ln = int(rng.integers(lo, hi + 1))
        s = int(rng.integers(0, genome - ln + 1))
        reads.append((s, s + ln, int(rng.integers(0, 2))))
    recs = []
    for i in range(n_reads):
        for j in range(i + 1, n_reads):
            if min(reads[i][1], reads[j][1]) - max(reads[i][0], reads[j][0]) < 500:
                continue
            x, y = (i, j) if rng.integers(0, 2) else (j, i)
            left, right = (int(t) for t in rng.integers(0, jitter + 1, 2))    # an alignment ends at one column for both reads
            r = placed(x + 1, y + 1, reads[x], reads[y], (left, right, left, right))
            if r is not None:
                recs.append(r)
    recs = np.concatenate(recs) if recs else np.zeros(0, RECORD_DTYPE)
    return list(range(1, n_reads + 1)), [e - s for s, e, _ in reads], reads, recs


def hub(degree, w_degree=0, step=10, w_step=1, read_len=20000):
    """A vertex of out-degree `degree`: read 1 (the hub, forward) and reads 2 .. degree + 1 beginning step, 2 step, ... after it, all of
    one length, so that none contains another; with w_degree > 0 the last of them gets w_degree further reads that begin 2 100 before its
    end, w_step apart (with step >= 100 they share less than 2 000 positions with the hub).  One record per pair that shares at least 2 000 positions.  Returns (ids, lengths, records)."""
    reads = [(0, read_len, 0)] + [(step * (k + 1), step * (k + 1) + read_len, 0) for k in range(degree)]
    if w_degree:
        s0 = reads[-1][0]
        reads += [(s0 + read_len - 2100 + w_step * k, s0 + 2 * read_len - 2100 + w_step * k, 0) for k in range(w_degree)]
    recs = []
    for i in range(len(reads)):
        for j in range(i + 1, len(reads)):
            if min(reads[i][1], reads[j][1]) - max(reads[i][0], reads[j][0]) >= 2000:
                recs.append(placed(i + 1, j + 1, reads[i], reads[j]))
    return list(range(1, len(reads) + 1)), [e - s for s, e, _ in reads], (np.concatenate(recs) if recs else np.zeros(0, RECORD_DTYPE))


def dove(fid, tid, ln, read_len=20000, rc=0):
    """The dovetail record of two reads of read_len whose arc (2 A -> 2 B + rc) has the length ln: lengths need not add up over a path."""
    span = read_len - ln
    b1, b2 = (0, span - 1) if not rc else (read_len - span, read_len - 1)
    return record(fid, tid, ln, read_len - 1, read_len, b1, b2, read_len, rc)
