"""Expected records of a search over precomputed sketch tables (the `.dat` path), pair by pair, from the oracle's literal
getOverlapInfo — plus a builder of ordered rows a Java `.dat` could hold and the crafted corpora of
tests/test_second_stage_crafted.py.  A helper module, not a test file: tests/test_sketch_search_ref.py pins it to orc_run_self.

Tables are laid out as MinHashSearch.export() returns them (ids, is_fwd, seq_length, minhash, ordered, ordered_size,
ordered_seqlen), without the status column: every entry given is stored.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def _candidates(q_mh, e_mh, num_min_matches):
    """Per-slot equality counts of the MinHash rows (MinHashSearch.java:166-181): (query, entry) index pairs with >= num_min_matches."""
    out = []
    for q0 in range(0, q_mh.shape[0], 256):
        hits = (q_mh[q0:q0 + 256, None, :] == e_mh[None, :, :]).sum(axis=2)
        qi, ei = np.nonzero(hits >= num_min_matches)
        out.append(np.stack([qi + q0, ei], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def expected_pairs(entries, queries=None, *, num_min_matches, min_store_length, pairs=None):
    """The (query, entry) pairs MinHashSearch.findMatches compares.  queries=None: self mode (toSelf, orc_run_self's loop, every
    forward entry is a query); else -q mode (toSelf false: only "never short to short", MinHashSearch.java:197-229).
    pairs: the (query row, entry row) pairs whose MinHash rows share at least num_min_matches slots, where the caller built the tables
    so that it knows them all (in self mode every query row a forward entry): the all-pairs scan is skipped, the filters still apply."""
    to_self = queries is None
    q = entries if to_self else queries
    if pairs is None:
        qsel = np.nonzero(np.asarray(entries["is_fwd"]) != 0)[0] if to_self else np.arange(len(q["ids"]))
        cand = [(int(qsel[qi_]), int(m)) for qi_, m in _candidates(np.asarray(q["minhash"])[qsel], np.asarray(entries["minhash"]), num_min_matches)]
    else:
        cand = sorted((int(qi), int(m)) for qi, m in pairs)
        assert not to_self or all(entries["is_fwd"][qi] for qi, _ in cand), "a query row of self mode that is no forward entry"
    pairs = []
    for qi, m in cand:
        qid, mid = int(q["ids"][qi]), int(entries["ids"][m])
        ql, ml = int(q["seq_length"][qi]), int(entries["seq_length"][m])
        if to_self and mid == qid:
            continue
        if ml < min_store_length and ql < min_store_length:
            continue
        if to_self and mid > qid and ml >= min_store_length and ql >= min_store_length:
            continue
        if to_self and ml < min_store_length and ql >= min_store_length:
            continue
        pairs.append((qi, int(m)))
    return pairs


def _row(t, i):
    return np.asarray(t["ordered"][i][:int(t["ordered_size"][i])])


def expected_records(entries, queries=None, *, H, k2, num_min_matches, min_store_length, threshold, max_shift, nthreads=16,
                     return_compared=False, pairs=None):
    """MinHashSearch.findMatches over the tables: sorted record lines (O.format_record), as orc_run_self builds its records —
    alen / blen the read lengths, the b1 / b2 flip of a reverse-strand entry (MatchResult.java:56-57), and at threshold 0 an EMPTY
    overlap is a record too.  return_compared: also the number of pairs given to getOverlapInfo (stats' candidates_compared).
    pairs: the candidate pairs, where the caller knows them (expected_pairs)."""
    assert np.asarray(entries["minhash"]).shape[1] == max(1, H)
    q = entries if queries is None else queries
    pairs = expected_pairs(entries, queries, num_min_matches=num_min_matches, min_store_length=min_store_length, pairs=pairs)

    def one(p):
        qi, m = p
        r = O.overlap(_row(q, qi), int(q["ordered_seqlen"][qi]), _row(entries, m), int(entries["ordered_seqlen"][m]), k2, max_shift)
        if not r["score"] >= threshold:
            return None
        alen, blen = int(q["seq_length"][qi]), int(entries["seq_length"][m])
        fwd = bool(entries["is_fwd"][m])
        b1, b2 = (r["b1"], r["b2"]) if fwd else (blen - r["b2"] - 1, blen - r["b1"] - 1)
        return O.format_record({"from_id": int(q["ids"][qi]), "to_id": int(entries["ids"][m]), "score": r["score"], "raw": r["raw"],
                                "a1": r["a1"], "a2": r["a2"], "alen": alen, "b1": b1, "b2": b2, "blen": blen, "to_rc": 0 if fwd else 1})

    with ThreadPoolExecutor(nthreads) as ex:   # (the ctypes calls release the GIL)
        lines = sorted(x for x in ex.map(one, pairs, chunksize=64) if x is not None)
    return (lines, len(pairs)) if return_compared else lines


def oracle_tables(fa, *, H, S, k=16, k2=12, min_olap_length=116, repeat_weight=0.9, both_strands=True, nthreads=16):
    """The sketch tables of the reads of `fa` from the oracle's primitives (O.minhash, O.ordered), laid out as export() returns them,
    WITH the status column: entry 2 i = read i forward, 2 i + 1 = its reverse complement (both_strands=False: forward rows only, entry
    i = read i).  Statuses as orc_run_self sets them (SequenceSketchStreamer.java:129-133, 235-238): 2 for both strands of a read
    shorter than min_olap_length, 1 for both when the forward strand has no k-mers, 1 for a reverse strand that fails alone.  Rows
    whose status is not 0 keep seq_length and are zero elsewhere."""
    n, per = len(fa), 2 if both_strands else 1

    def one(i):
        s = fa.sequence(i)
        if len(s) < min_olap_length:
            return [(2, None, None, 0)] * per
        out = []
        for t in ((s, O.rc(s)) if both_strands else (s,)):
            rc1, mh = O.minhash(t, k, H, repeat_weight)
            rc2, od, olen = O.ordered(t, k2, S)
            out.append((1, None, None, 0) if (rc1 or rc2) else (0, mh, od, olen))
        if out[0][0] != 0:
            out = [(1, None, None, 0)] * per
        return out

    with ThreadPoolExecutor(nthreads) as ex:
        rows = list(ex.map(one, range(n)))
    m = per * n
    t = {"ids": np.repeat(np.asarray(fa.ids, np.int64), per), "is_fwd": np.tile(np.array([1, 0][:per], np.uint8), n),
         "seq_length": np.repeat(np.asarray(fa.lengths, np.int32), per), "minhash": np.zeros((m, max(1, H)), np.int32),
         "ordered": np.zeros((m, S, 2), np.int32), "ordered_size": np.zeros(m, np.int32), "ordered_seqlen": np.zeros(m, np.int32),
         "status": np.zeros(m, np.uint8)}
    for i, r in enumerate(rows):
        for j, (st, mh, od, olen) in enumerate(r):
            e = per * i + j
            t["status"][e] = st
            if st == 0:
                t["minhash"][e] = mh
                t["ordered"][e, :len(od)] = od
                t["ordered_size"][e], t["ordered_seqlen"][e] = len(od), olen
    return t


def stored_rows(t, forward_only=False):
    """The rows of oracle_tables / export() that are stored (status 0), without the status column: what add_sketches and
    expected_records take."""
    keep = np.asarray(t["status"]) == 0
    if forward_only:
        keep &= np.asarray(t["is_fwd"]) != 0
    return {k: np.asarray(v)[keep] for k, v in t.items() if k != "status"}


# ---- rows a Java .dat could hold ------------------------------------------------------------------------------------------------
def check_row(row, seqlen, S):
    """Assert the invariants of an ordered row as OrderedNGramHashes leaves it: sorted by (signed hash, position), distinct
    positions in [0, seqlen), size min(S, seqlen)."""
    row = np.asarray(row, dtype=np.int64).reshape(-1, 2)
    assert row.shape[0] == min(S, seqlen), ("ordered size", row.shape[0], S, seqlen)
    assert np.all((row[:, 0] >= INT32_MIN) & (row[:, 0] <= INT32_MAX)), "hash outside int32"
    pos = row[:, 1]
    assert np.all((pos >= 0) & (pos < seqlen)), "position outside [0, seqlen)"
    assert len(np.unique(pos)) == len(pos), "duplicated position"
    order = np.lexsort((pos, row[:, 0]))
    assert np.array_equal(order, np.arange(len(pos))), "row not sorted by (hash, position)"


class TableBuilder:
    """Entries of one table.  add() checks every row and sets seq_length = ordered_seqlen + k2 - 1."""

    def __init__(self, S, H, k2=12):
        self.S, self.H, self.k2 = S, H, k2
        self.rows = []

    def add(self, rid, hashes, positions, seqlen, minhash, fwd=True):
        h = np.asarray(hashes, dtype=np.int64)
        p = np.asarray(positions, dtype=np.int64)
        o = np.lexsort((p, h))
        row = np.stack([h[o], p[o]], axis=1)
        check_row(row, seqlen, self.S)
        assert seqlen + self.k2 - 1 <= 1 << 30
        mh = np.asarray(minhash, dtype=np.int64)
        assert mh.shape == (self.H,)
        self.rows.append((int(rid), 1 if fwd else 0, int(seqlen) + self.k2 - 1, mh, row, int(seqlen)))
        return len(self.rows) - 1

    def table(self):
        n = len(self.rows)
        t = {"ids": np.zeros(n, np.int64), "is_fwd": np.zeros(n, np.uint8), "seq_length": np.zeros(n, np.int32),
             "minhash": np.zeros((n, self.H), np.int32), "ordered": np.zeros((n, self.S, 2), np.int32),
             "ordered_size": np.zeros(n, np.int32), "ordered_seqlen": np.zeros(n, np.int32)}
        for i, (rid, fwd, sl, mh, row, osl) in enumerate(self.rows):
            t["ids"][i], t["is_fwd"][i], t["seq_length"][i], t["ordered_seqlen"][i] = rid, fwd, sl, osl
            t["minhash"][i] = mh.astype(np.int32)
            t["ordered"][i, :row.shape[0]] = row.astype(np.int32)   # (hashes >= 2^31 do not occur: check_row)
            t["ordered_size"][i] = row.shape[0]
        return t


# ---- crafted corpora ------------------------------------------------------------------------------------------------------------
class _Hashes:
    """Distinct random int32 hashes, never reused, avoiding the values a corpus sets aside."""

    def __init__(self, rng, reserved=()):
        self.rng, self.used = rng, set(int(x) for x in reserved)

    def take(self, n, lo=INT32_MIN, hi=INT32_MAX):
        out = []
        while len(out) < n:
            x = self.rng.integers(lo, hi, size=2 * (n - len(out)) + 8, endpoint=True, dtype=np.int64)
            for v in x.tolist():
                if v not in self.used and lo <= v <= hi:
                    self.used.add(v); out.append(v)
                    if len(out) == n:
                        break
        return out


def _positions(rng, n, seqlen, lo=0, hi=None):
    hi = seqlen if hi is None else hi
    return (rng.choice(hi - lo, size=n, replace=False) + lo).tolist()


class Corpus:
    """Entries (self mode: every forward entry is also a query) and forward query rows (-q mode) that reach the second stage in
    known pairs.  Pairs that are meant to be compared share one MinHash row; every other row is independent random values."""

    def __init__(self, S, H=16, k2=12, seed=0, reserved=()):
        self.S, self.H, self.k2 = S, H, k2
        self.rng = np.random.default_rng(seed)
        self.hs = _Hashes(self.rng, reserved)
        self.entries = TableBuilder(S, H, k2)
        self.queries = TableBuilder(S, H, k2)
        self.next_id = 1
        self.notes = {}   # name -> what a pair hits (for failure messages)
        self.pair_joined = []   # (joined k-mers, entries of the duplicated-hash groups, group-capped) of every crafted pair

    def minhash(self):
        return self.hs.take(self.H)

    def _fill(self, taken, n, seqlen, lo=INT32_MIN, hi=INT32_MAX):
        """n more (hash, position) entries with fresh hashes and positions not in `taken`."""
        free = n
        pos = []
        if free > 0:
            avail = np.setdiff1d(np.arange(seqlen) if seqlen <= 4 * n + 4096 else self.rng.choice(seqlen, size=4 * n + 4096, replace=False),
                                 np.asarray(sorted(taken), dtype=np.int64))
            pos = self.rng.choice(avail, size=free, replace=False).tolist()
        return self.hs.take(free, lo, hi), pos

    def pair(self, name, *, joined, size_a=None, size_b=None, seqlen_a=None, seqlen_b=None, shift=0, groups=(), rev_b=False,
             spread=None, start_a=0, filter_noise=0, hash_range=None, fixed=(), ties=0):
        """One crafted pair A (query) / B (entry) sharing a MinHash row.  `joined` hashes occur once in either row, at A position
        p and B position p + shift; every group (m, n) is a hash m times in A and n times in B; the rest of either row is filler
        with hashes of its own.  filter_noise: that many filler hashes of B equal a filler hash of A in the low 16 bits only.
        fixed: hashes (e.g. INT32_MIN) that the pair shares as joined k-mers.  ties: groups whose two records tie in optimizeShifts."""
        S = self.S
        size_a = S if size_a is None else size_a
        size_b = S if size_b is None else size_b
        seqlen_a = size_a if seqlen_a is None else seqlen_a
        seqlen_b = size_b if seqlen_b is None else seqlen_b
        assert size_a == min(S, seqlen_a) and size_b == min(S, seqlen_b)
        lo, hi = (INT32_MIN, INT32_MAX) if hash_range is None else hash_range
        gsum_a = sum(m for m, _ in groups); gsum_b = sum(n for _, n in groups)
        nj = joined + len(fixed)
        assert nj + gsum_a <= size_a and nj + gsum_b <= size_b, (name, nj, gsum_a, gsum_b, size_a, size_b)
        # joined + group positions: A positions inside [start_a, start_a + spread), B = A + shift (clipped into B)
        ncore = nj + max(gsum_a, gsum_b)
        spread = spread or max(ncore * 2 + 8 * ties + 8, 8)
        lo_a = max(start_a, -shift, 0)
        hi_a = min(seqlen_a, lo_a + spread, seqlen_b - shift)
        top_tie = hi_a - 4
        hi_a -= 8 * ties + 4 if ties else 0
        assert hi_a - lo_a >= nj + gsum_a, (name, lo_a, hi_a, ncore)
        assert not ties or top_tie + shift + 2 < seqlen_b
        pa = sorted(self.rng.choice(hi_a - lo_a, size=nj + gsum_a, replace=False) + lo_a)
        pa = self.rng.permutation(pa).tolist()
        hj = list(fixed) + self.hs.take(joined, lo, hi)
        A_h, A_p, B_h, B_p = list(hj), pa[:nj], list(hj), [p + shift for p in pa[:nj]]
        rest = pa[nj:]
        for t in range(ties):
            # a hash once in A, twice in B at shift -2 / +2: the two records tie on |shift - median| (optimizeShifts keeps the first);
            # at the top of the joined range, so the one kept is the window's end in B
            g = self.hs.take(1, lo, hi)[0]
            p = top_tie - 8 * t
            A_h += [g]; A_p += [p]; B_h += [g, g]; B_p += [p + shift - 2, p + shift + 2]
        for (m, n) in groups:
            g = self.hs.take(1, lo, hi)[0]
            ga, rest = rest[:m], rest[m:]
            A_h += [g] * m; A_p += ga
            # B positions next to the first A one (+ shift) so the group's records stay inside the shift window
            gb, k, taken = [], 0, set(B_p)
            while len(gb) < n:
                assert k <= 2 * seqlen_b + 2, (name, "no room for a group in B")
                c = ga[0] + shift + ((k + 1) // 2) * (1 if k % 2 else -1)
                k += 1
                if 0 <= c < seqlen_b and c not in taken:
                    gb.append(c); taken.add(c)
            B_h += [g] * n; B_p += gb
        fa_h, fa_p = self._fill(set(A_p), size_a - len(A_p), seqlen_a, lo, hi)
        A_h += fa_h; A_p += fa_p
        nb_fill = size_b - len(B_p)
        if filter_noise:
            k = min(filter_noise, nb_fill, len(fa_h))
            low = np.asarray(fa_h[:k], dtype=np.int64) & 0xFFFF
            noise = []
            for v in low.tolist():
                while True:
                    x = int(self.rng.integers(-(1 << 15), (1 << 15) - 1)) * 65536 + v
                    if x not in self.hs.used and INT32_MIN <= x <= INT32_MAX:
                        self.hs.used.add(x); noise.append(x); break
            _, npos = self._fill(set(B_p), k, seqlen_b)
            B_h += noise; B_p += npos; nb_fill -= k
        fb_h, fb_p = self._fill(set(B_p), nb_fill, seqlen_b, lo, hi)
        B_h += fb_h; B_p += fb_p
        mh = self.minhash()
        qid, eid = self.next_id + 1, self.next_id       # self mode keeps the pair (larger id asks, smaller id is stored)
        self.next_id += 2
        ia = self.entries.add(qid, A_h, A_p, seqlen_a, mh)
        ib = self.entries.add(eid, B_h, B_p, seqlen_b, mh, fwd=not rev_b)
        self.queries.add(qid, A_h, A_p, seqlen_a, mh)
        self.notes[name] = (ia, ib)
        capped = len(groups) + ties > 16 or any(m > 8 or n > 8 for m, n in groups)
        self.pair_joined.append((joined + len(fixed), sum(m + n for m, n in groups) + 3 * ties, capped))
        return ia, ib

    def group(self, name, n, size, seqlen=None, shared=0.5):
        """n entries with one MinHash row: every ordered pair among them is compared (n (n - 1) / 2 in self mode).  The rows share
        a pool of hashes, each entry keeping a random `shared` fraction of it (positions from one common layout)."""
        seqlen = size if seqlen is None else seqlen
        pool = self.hs.take(2 * size)
        ppos = _positions(self.rng, 2 * size, max(seqlen, 2 * size))
        mh = self.minhash()
        ids = []
        for _ in range(n):
            keep = self.rng.choice(2 * size, size=int(size * shared), replace=False)
            h = [pool[i] for i in keep]
            p = [min(ppos[i], seqlen - 1) for i in keep]
            # distinct positions inside [0, seqlen): collisions from the clip move to free ones
            seen, pp = set(), []
            for x in p:
                while x in seen:
                    x = (x + 1) % seqlen
                seen.add(x); pp.append(x)
            fh, fp = self._fill(seen, size - len(h), seqlen)
            rid = self.next_id; self.next_id += 1
            self.entries.add(rid, h + fh, pp + fp, seqlen, mh)
            self.queries.add(rid, h + fh, pp + fp, seqlen, mh)
            ids.append(rid)
        self.notes[name] = tuple(ids)

    def loner(self, size, seqlen=None, fwd=True):
        """An entry nobody is compared with (its MinHash row is its own)."""
        seqlen = size if seqlen is None else seqlen
        h, p = self._fill(set(), size, seqlen)
        rid = self.next_id; self.next_id += 1
        self.entries.add(rid, h, p, seqlen, self.minhash(), fwd=fwd)

    def tables(self):
        return self.entries.table(), self.queries.table()


def wrap_edges(nvalid, le, re):
    """computeEdges' start and end of a window (OverlapInfo :131-134) with Java's int products, and without the wrap."""
    def i32(x):
        x &= 0xFFFFFFFF
        return x - (1 << 32) if x >= 1 << 31 else x
    den = nvalid - 1
    wrapped = (O.java_round(i32(nvalid * le - re) / den), O.java_round(i32(nvalid * re - le) / den))
    exact = (O.java_round((nvalid * le - re) / den), O.java_round((nvalid * re - le) / den))
    return wrapped, exact


def slow_pairs_model(pairs, join_wide, S):
    """Pairs the join path leaves to the per-lane kernel (mhap_capi.hip's pass loop): `pairs` = (joined k-mers, group entries,
    group-capped) of every compared pair; a pair fits a pass when it is not group-capped and joined + group entries <= its cap.
    Assumes one query chunk and S small enough for the join kernel."""
    caps = [128, 512, 1536]
    slow = [p for p in pairs if p[2] or p[0] + p[1] > caps[0]]
    group_bad = sum(1 for p in slow if p[2])
    for level in range(join_wide):
        if not slow or group_bad * 10 > len(slow) * 9:
            break
        if level == 1 and 2 * (((S + 3) & ~3) + 3 * 1536 + 16 * 22) * 4 > 65536:
            break
        before = len(slow)
        slow = [p for p in slow if p[2] or p[0] + p[1] > caps[level + 1]]
        group_bad = sum(1 for p in slow if p[2])
        if len(slow) * 10 > before * 9:
            break
    return len(slow)
