"""Cases for the variant-site tests: hand-computed pile-ups at the edges of the site rule, hand-made judgements, builders that put
sites and informative columns where the kernels change tile or chunk, and the planted diploid.  Plain Python over numpy; nothing here
calls the library.  Every case names its six parameters."""
import numpy as np

import consensus_ref as cr
import handmade_paths as hp
from align_ref import rc_bytes

ACGT = b"ACGT"
P = dict(min_depth=8, min_minor=3, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # the hand cases' parameters, named in full


def with_(**changes):
    return dict(P, **changes)


# ---- the site rule, position by position: (name, votes A C G T del, own byte, parameters, expected site, expected fields or None) ----
SITE_CASES = [
    # depth: 7 votes and the own base make 8
    ("depth min_depth - 1", (3, 3, 0, 0, 0), ord("A"), P, False, dict(depth=7, deep=False)),
    ("depth min_depth", (4, 3, 0, 0, 0), ord("A"), P, True, dict(depth=8, deep=True, major=0, minor=1, n_major=5, n_minor=3)),
    # the minor count
    ("minor min_minor - 1", (7, 2, 0, 0, 0), ord("A"), P, False, dict(depth=10, n_minor=2)),
    ("minor min_minor", (6, 3, 0, 0, 0), ord("A"), P, True, dict(depth=10, n_minor=3)),
    # 100 c[minor] == min_pct depth exactly: 3 of 12; one vote under it: 3 of 13
    ("percentage at equality", (8, 3, 0, 0, 0), ord("A"), P, True, dict(depth=12, n_minor=3)),
    ("percentage one under", (9, 3, 0, 0, 0), ord("A"), P, False, dict(depth=13, n_minor=3)),
    # 100 del == max_del_pct depth exactly: 3 of 12; one over: 4 of 13 (and the minor still at its share: 4 of 13)
    ("deletions at the bound", (4, 4, 0, 0, 3), ord("A"), P, True, dict(depth=12, n_minor=4)),
    ("deletions one over", (4, 4, 0, 0, 4), ord("A"), P, False, dict(depth=13, n_minor=4)),
    # a three-way tie of counts: the lower codes win, the own base breaks it
    ("three-way tie", (3, 4, 4, 0, 0), ord("A"), with_(min_depth=4), True, dict(major=0, minor=1, n_major=4, n_minor=4, depth=12)),
    ("three-way tie, own G", (4, 4, 3, 0, 0), ord("G"), with_(min_depth=4), True, dict(major=0, minor=1, n_major=4, n_minor=4, depth=12)),
    ("tie of C, G, T", (0, 3, 3, 3, 0), ord("N"), with_(min_depth=4), False, dict(major=1, minor=2, depth=9)),
    # the own base makes the difference: depth 8 only with it; the minor 3 only with it
    ("own base makes the depth", (4, 3, 0, 0, 0), ord("C"), P, True, dict(depth=8, n_major=4, n_minor=4, major=0, minor=1)),
    ("own base makes the minor", (6, 2, 0, 0, 0), ord("C"), P, True, dict(depth=9, n_minor=3, minor=1)),
    ("without it, no minor", (6, 2, 0, 0, 0), ord("A"), P, False, dict(depth=9, n_minor=2)),
    # own base N: deep, well supported, and no site
    ("own N", (5, 5, 0, 0, 0), ord("N"), P, False, dict(depth=10, deep=True, n_minor=5)),
    ("nobody voted", (0, 0, 0, 0, 0), ord("T"), P, False, dict(depth=1, major=3, minor=0, n_major=1, n_minor=0)),
]

# ---- one column's class: (name, a, b, site of A, site of B in its own orientation, to_rc, expected) ----------------------------------
A_, C_, G_, T_ = 0, 1, 2, 3
CLASS_CASES = [
    ("no site", b"A", b"A", None, None, 0, None),
    ("agree on A's site", b"A", b"A", (A_, C_), None, 0, "agree"),
    ("disagree on A's site", b"A", b"C", (A_, C_), None, 0, "disagree"),
    ("disagree on B's site", b"C", b"A", None, (C_, A_), 0, "disagree"),
    ("both sites, equal pairs", b"A", b"C", (A_, C_), (C_, A_), 0, "disagree"),
    ("both sites, unequal pairs", b"A", b"C", (A_, C_), (C_, G_), 0, "other"),
    ("b outside the pair", b"A", b"G", (A_, C_), None, 0, "other"),
    ("a outside the pair", b"T", b"C", (A_, C_), None, 0, "other"),
    ("N in read B", b"A", b"N", (A_, C_), None, 0, "other"),
    ("N in read A", b"N", b"C", None, (A_, C_), 0, "other"),
    # a reverse record: B's own site (T, G) is (A, C) in the aligner's orientation
    ("reverse, B's site complemented", b"A", b"C", None, (T_, G_), 1, "disagree"),
    ("reverse, both sites, equal after the complement", b"C", b"C", (C_, A_), (T_, G_), 1, "agree"),
    ("reverse, both sites, unequal after the complement", b"A", b"C", (A_, C_), (A_, C_), 1, "other"),
]

# ---- keep: (agree, disagree, parameters, expected keep) --------------------------------------------------------------------------------
KEEP_CASES = [
    (0, 1, P, True),                          # disagree == min_diff - 1
    (0, 2, P, False),                         # disagree == min_diff
    (2, 2, P, False),                         # the percentage at equality: 2 of 4 is 50 %
    (3, 2, P, True),                          # one agreeing column more: 40 %
    (5, 3, with_(min_diff=3, diff_pct=38), True),    # 300 < 38 * 8
    (5, 3, with_(min_diff=3, diff_pct=37), False),
    (9, 0, P, True),
]


# ---- builders for the GPU cases ---------------------------------------------------------------------------------------------------------

def other_base(c, step=1):
    """Another of A, C, G, T than byte c."""
    return ACGT[(ACGT.index(c) + step) % 4]


class Table:
    """Reads, records and paths for one session.  pile(x, alts) gives read x a pile-up of three records against a copy of itself and
    two against a copy that carries alts[t] at the positions t: with the parameters SMALL those positions are sites of read x."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.recs, self.paths = [], [], []

    def read(self, seq):
        self.reads.append(bytes(seq))
        return len(self.reads) - 1

    def random_read(self, n):
        return self.read(bytes(int(x) for x in self.rng.choice(list(ACGT), n)))

    def record(self, x, y, s2, fa, fb, runs, to_rc, copies=1):
        assert self.reads[y] == (rc_bytes(s2) if to_rc else s2)
        rec = hp.record_for(x + 1, y + 1, self.reads[x], s2, fa, fb, runs, to_rc)
        for _ in range(copies):
            self.recs.append(rec)
            self.paths.append([int(r) for r in runs])
        return rec

    def pile(self, x, alts, to_rc=0):
        seq = self.reads[x]
        alt = bytearray(seq)
        for t, c in alts.items():
            alt[t] = c
        same = self.read(rc_bytes(seq) if to_rc else seq)
        self.record(x, same, seq, 0, 0, [hp.run("=", len(seq))], to_rc, copies=3)
        y = self.read(rc_bytes(bytes(alt)) if to_rc else bytes(alt))
        self.record(x, y, bytes(alt), 0, 0, [hp.run("=", len(seq))], to_rc, copies=2)
        return y

    @property
    def ids(self):
        return list(range(1, len(self.reads) + 1))

    def add(self, order=None):
        order = range(len(self.recs)) if order is None else order
        paths = [self.paths[q] for q in order]
        off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
        ops = np.array([r for p in paths for r in p], np.uint32)
        recs = np.concatenate([self.recs[q] for q in order]) if len(paths) else np.zeros(0, cr.RECORD_DTYPE)
        return recs, off, ops


SMALL = dict(min_depth=4, min_minor=2, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # own + 3 equal + 2 other: depth 6, minor 2


def alternating_runs(rng, n, long_run=None):
    """A canonical path of n runs: '=' (1 to 3 columns) and 'X' (1 column) in turn, with one 'D' behind the first 'X' when n is even so
    that the last run is '='.  long_run: (index, columns) lengthens that run."""
    codes = ["=" if u % 2 == 0 else "X" for u in range(n if n % 2 else n - 1)]
    if n % 2 == 0:
        codes.insert(2, "D")
    runs = [hp.run(c, int(rng.integers(1, 4)) if c == "=" else 1) for c in codes]
    if long_run:
        runs[long_run[0]] = hp.run(codes[long_run[0]], long_run[1])
    assert len(runs) == n
    return hp.check_canonical(runs)


def chunk_edge_columns(runs, fa, fb):
    """The (i, j, code) of the first and the last column of every chunk of 64 runs of a path from (fa, fb)."""
    out, i, j = [], fa, fb
    for u, r in enumerate(runs):
        length, code = int(r) >> 4, int(r) & 15
        di = length if code != cr.OP_D else 0
        dj = length if code != cr.OP_I else 0
        if u % 64 == 0:
            out.append((i, j, code))
        if u % 64 == 63 or u == len(runs) - 1:
            out.append((i + max(di - 1, 0), j + max(dj - 1, 0), code))
        i, j = i + di, j + dj
    return out


# ---- the planted diploid ----------------------------------------------------------------------------------------------------------------

def planted_diploid(seed=11, genome_len=20000, every=400, read_len=4000, error=0.0, mix=(0.79, 0.12, 0.09), repeat=None, copies=1):
    """Two haplotypes of one random sequence, the second with a substitution at every position `every` m + every / 2; 15 reads of
    read_len per haplotype at staggered starts (multiples of `every`, so that no read and no overlap ends within every / 2 of a planted
    position), every second one stored reverse-complemented.  error: the reads' error rate, split into insertions, deletions and
    substitutions by mix.  copies: that many reads per start (the measurements' deeper pile-ups).  repeat: (first, second, length, every)
    makes the genome haploid with a second copy of a stretch, diverged by a substitution every `every` bases.  Returns a dict: reads (as stored), ids (1-based), place [(haplotype, start, end, strand)], planted (genome
    positions), haps, and true_len (per read, the length before errors)."""
    rng = np.random.default_rng(seed)
    hap0 = bytearray(int(x) for x in rng.choice(list(ACGT), genome_len))
    if repeat:   # (first, second, length, every): the second copy of a stretch of hap0, diverged by a substitution every `every` bases
        first, second, length, div = repeat
        hap0[second:second + length] = hap0[first:first + length]
        for t in range(second + div // 2, second + length, div):
            hap0[t] = other_base(hap0[t])
    planted = list(range(every // 2, genome_len, every)) if every else []
    hap1 = bytearray(hap0)
    for t in planted:
        hap1[t] = other_base(hap0[t], 1 + t % 3)
    step = 3 * (every or 400)
    last = genome_len - read_len
    starts = ([k * step for k in range(14)] + [last], [0] + [(every or 400) + k * step for k in range(13)] + [last])
    p_ins, p_del, p_sub = (error * m for m in mix)
    reads, place, true_len = [], [], []
    for h, hap in enumerate((hap0, hap1)):
        if repeat and h == 1:
            break   # a haploid genome
        for k, start in enumerate(s for s in starts[h] for _ in range(copies)):
            assert 0 <= start <= last
            seg = bytes(hap[start:start + read_len])
            strand = k % 2
            src = rc_bytes(seg) if strand else seg
            out = bytearray()
            for c in src:
                u = rng.random() if error else 1.0
                while u < p_ins:
                    out.append(int(rng.choice(list(ACGT))))
                    u = rng.random()
                if u < p_ins + p_del:
                    continue
                out.append(other_base(c, int(rng.integers(1, 4))) if u < p_ins + p_del + p_sub else c)
            reads.append(bytes(out))
            place.append((h, start, start + read_len, strand))
            true_len.append(read_len)
    return dict(reads=reads, ids=list(range(1, len(reads) + 1)), place=place, planted=planted, haps=(bytes(hap0), bytes(hap1)), true_len=true_len)


def layout_records(d, min_shared=1000):
    """One record per two reads whose placements share at least min_shared genome bases (same and cross haplotype), its coordinates
    from the layout, scaled to the stored lengths when the reads have errors."""
    reads, place = d["reads"], d["place"]
    recs = []
    for x in range(len(reads)):
        for y in range(x + 1, len(reads)):
            (_, sa, ea, ta), (_, sb, eb, tb) = place[x], place[y]
            lo, hi = max(sa, sb), min(ea, eb)
            if hi - lo < min_shared:
                continue

            def own(s, e, strand, n):   # the shared interval in the stored read's coordinates, both ends included
                b, f = (e - hi, e - 1 - lo) if strand else (lo - s, hi - 1 - s)
                scale = n / (e - s)
                return min(int(b * scale), n - 1), min(int(f * scale), n - 1)
            a1, a2 = own(sa, ea, ta, len(reads[x]))
            b1, b2 = own(sb, eb, tb, len(reads[y]))
            rec = np.zeros(1, cr.RECORD_DTYPE)
            rec[0] = (x + 1, y + 1, 0.9, 100.0, a1, a2, len(reads[x]), b1, b2, len(reads[y]), int(ta != tb), 0)
            recs.append(rec)
    return np.concatenate(recs)


def genome_position(place, r, t):
    """The genome position of position t of stored read r (error-free reads)."""
    _, s, e, strand = place[r]
    return e - 1 - t if strand else s + t


def layout_counters(d, recs):
    """Per read an int array (len, 5) of the votes A C G T del the error-free layout gives: every record's other read votes its own
    haplotype's base at every shared position, in the stored read's orientation."""
    reads, place, haps = d["reads"], d["place"], d["haps"]
    out = [np.zeros((len(r), 5), np.int64) for r in reads]
    for rec in recs:
        x, y = int(rec["from_id"]) - 1, int(rec["to_id"]) - 1
        for target, ev, t1, t2 in ((x, y, int(rec["a1"]), int(rec["a2"])), (y, x, int(rec["b1"]), int(rec["b2"]))):
            for t in range(t1, t2 + 1):
                g = genome_position(place, target, t)
                base = haps[place[ev][0]][g]
                if place[target][3]:
                    base = rc_bytes(bytes([base]))[0]
                out[target][t, ACGT.index(base)] += 1
    return out


def diagonal_paths(d, recs):
    """(op_offsets, ops) of error-free layout records: the one diagonal the layout gives, '=' where the two reads agree, 'X' where not."""
    paths = []
    for rec in recs:
        s1, own_b = d["reads"][int(rec["from_id"]) - 1], d["reads"][int(rec["to_id"]) - 1]
        s2 = rc_bytes(own_b) if int(rec["to_rc"]) else own_b
        i0, n = int(rec["a1"]), int(rec["a2"]) - int(rec["a1"]) + 1
        j0 = len(own_b) - int(rec["b2"]) - 1 if int(rec["to_rc"]) else int(rec["b1"])
        same = np.frombuffer(s1[i0:i0 + n], np.uint8) == np.frombuffer(s2[j0:j0 + n], np.uint8)
        cuts = np.flatnonzero(np.diff(same.astype(np.int8))) + 1
        edges = np.concatenate([[0], cuts, [n]])
        paths.append([hp.run("=" if same[edges[k]] else "X", edges[k + 1] - edges[k]) for k in range(len(edges) - 1)])
    off = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    return off, np.array([r for p in paths for r in p], np.uint32)


def check_truth(d, recs, offsets, sites, keep, p, site_of):
    """The four statements of the error-free planted diploid, asserted exactly.  recs: the records as realigned, with keep; offsets and
    sites: the site list; site_of: the restatement's rule for one position.  Returns (cross-haplotype records, those set aside)."""
    reads, place, planted = d["reads"], d["place"], set(d["planted"])
    listed = [set(int(t) for t in sites[int(offsets[r]):int(offsets[r + 1]), 0]) for r in range(len(reads))]
    for r in range(len(reads)):                                     # 1: every listed site lies on a planted position
        for t in listed[r]:
            assert genome_position(place, r, t) in planted, (r, t)
    counters = layout_counters(d, recs)
    for r in range(len(reads)):                                     # 2: every planted position whose layout counters meet the rule is listed
        for t in range(len(reads[r])):
            if genome_position(place, r, t) in planted and site_of(counters[r][t], reads[r][t], p)["site"]:
                assert t in listed[r], (r, t)
    cross = aside = 0
    for q, rec in enumerate(recs):
        x, y = int(rec["from_id"]) - 1, int(rec["to_id"]) - 1
        if place[x][0] == place[y][0]:                               # 3: no same-haplotype overlap is set aside
            assert keep[q], q
            continue
        cross += 1
        aside += not keep[q]
        n = 0                                                        # the listed sites its aligned interval holds, column by column
        for i in range(int(rec["a1"]), int(rec["a2"]) + 1):
            g = genome_position(place, x, i)
            if g in planted:
                _, sb, eb, tb = place[y]
                n += i in listed[x] or (eb - 1 - g if tb else g - sb) in listed[y]
        if n >= p["min_diff"]:                                       # 4: such a cross-haplotype overlap is set aside
            assert not keep[q], (q, n)
    return cross, aside
