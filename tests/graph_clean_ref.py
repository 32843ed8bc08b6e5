"""The graph-cleaning contract restated in Python from the prose of include/mhap_hip.h ("graph cleaning", in the string-graph
section): tip candidates and their holders, bubble branches and their siblings, the rounds, the dropped and removed bytes, the counts
and the GFA text of the cleaned read graph.  Built on string_graph_ref.Graph (the arc rows) and unitig_ref.Unitigs (the unitig graph of
a round); plain loops over Python integers, and nothing here calls the library.  Also the hand-made shapes of the cleaning tests."""
import numpy as np

import string_graph_ref as sg
import unitig_ref as ur

COUNT_NAMES = ("rounds", "tip_unitigs", "tip_reads", "bubble_unitigs", "bubble_reads", "arcs_removed")
TIP, BUBBLE = 1, 2


def masked_unitigs(rows, contained, lengths, dropped, removed):
    """The unitigs of a round: dropped reads have no vertices, removed arcs do not count.  The rows keep their places, so a link's
    `arc` is the index in the unchanged list."""
    rows = [list(r[:6]) + [1 if r[6] and not removed[i] else 0] for i, r in enumerate(rows)]
    return ur.Unitigs(rows, [1 if c or d else 0 for c, d in zip(contained, dropped)], lengths)


class Verdicts:
    """The verdict of every unitig of one snapshot: 0 stays, TIP, BUBBLE."""

    def __init__(self, U, tip_reads, bubble_bases):
        n = len(U.unitig_len)
        self.members = [U.unitig_start[k + 1] - U.unitig_start[k] for k in range(n)]
        self.bases, self.circular = list(U.unitig_len), list(U.circular)
        self.tip_reads, self.bubble_bases = tip_reads, bubble_bases
        self.out = {}
        table = {(fu, fo, tu, to) for fu, fo, tu, to, _, _ in U.links}
        assert len(table) == len(U.links)                               # one link between two oriented unitigs
        for fu, fo, tu, to, _, _ in U.links:
            assert (tu, 1 - to, fu, 1 - fo) in table                    # every link's complement is in the table
            self.out.setdefault((fu, fo), []).append((tu, to))
        self.verdict = [0] * n
        for X in range(n):
            cand = [o for o in (0, 1) if self.candidate(X, o)]
            assert len(cand) <= 1                                       # a candidate in at most one orientation
            tip = bool(cand) and self.tip_removed(X, cand[0])
            pops = [self.popped(X, o) for o in (0, 1)]
            assert pops[0] == pops[1]                                   # the verdict is the same seen from the twin side
            assert not (tip and pops[0])
            self.verdict[X] = TIP if tip else BUBBLE if pops[0] else 0

    def outs(self, X, o):
        return self.out.get((X, o), [])

    def ins(self, X, o):
        return [(W, 1 - w) for W, w in self.outs(X, 1 - o)]

    def rank(self, X):
        return (self.members[X], self.bases[X], -X)

    def candidate(self, T, o):
        return not self.circular[T] and self.members[T] <= self.tip_reads and not self.ins(T, o) and len(self.outs(T, o)) >= 1

    def tip_removed(self, T, o):
        for J, j in self.outs(T, o):
            if not any(W != T and (not self.candidate(W, w) or self.rank(W) > self.rank(T)) for W, w in self.ins(J, j)):
                return False
        return True

    def branch(self, B, o):
        """((S, s), (E, e)) when (B, o) is a bubble branch between them, else None."""
        if self.circular[B] or self.bases[B] > self.bubble_bases or len(self.ins(B, o)) != 1 or len(self.outs(B, o)) != 1:
            return None
        S, E = self.ins(B, o)[0], self.outs(B, o)[0]
        return None if B in (S[0], E[0]) else (S, E)

    def popped(self, B, o):
        ends = self.branch(B, o)
        if ends is None:
            return False
        return any(B2 != B and self.branch(B2, o2) == ends and self.rank(B2) > self.rank(B) for B2, o2 in self.outs(*ends[0]))


class Cleaned:
    """The cleaning of a finished string_graph_ref.Graph: dropped (per read), removed (per arc), counts (a dict of COUNT_NAMES),
    unitigs (the unitig_ref.Unitigs of the cleaned graph) and `history`, per round the (Unitigs, verdicts) it decided on."""

    def __init__(self, g, tip_reads=4, bubble_bases=50000, max_rounds=16):
        assert tip_reads >= 0 and bubble_bases >= 0 and max_rounds >= 1
        self.g = g
        self.dropped, self.removed = [0] * len(g.lengths), [0] * len(g.rows)
        c = dict.fromkeys(COUNT_NAMES, 0)
        self.history = []
        while c["rounds"] < max_rounds:
            U = masked_unitigs(g.rows, g.contained, g.lengths, self.dropped, self.removed)
            verdict = Verdicts(U, tip_reads, bubble_bases).verdict
            self.history.append((U, verdict))
            c["rounds"] += 1
            if not any(verdict):
                break
            for X, what in enumerate(verdict):
                if what:
                    reads = [U.vertex[m] >> 1 for m in range(U.unitig_start[X], U.unitig_start[X + 1])]
                    for r in reads:
                        assert not self.dropped[r] and not g.contained[r]
                        self.dropped[r] = what
                    c["tip_unitigs" if what == TIP else "bubble_unitigs"] += 1
                    c["tip_reads" if what == TIP else "bubble_reads"] += len(reads)
            self.removed = [1 if r[6] and (self.dropped[r[0] >> 1] or self.dropped[r[1] >> 1]) else 0 for r in g.rows]
        c["arcs_removed"] = sum(self.removed)
        self.counts = c
        self.unitigs = masked_unitigs(g.rows, g.contained, g.lengths, self.dropped, self.removed)

    def gfa(self):
        """The GFA 1 text of the cleaned read graph: no S line for a dropped read, no L line for a removed arc."""
        g = self.g
        out = ["H\tVN:Z:1.0"]
        out += [f"S\t{i}\t*\tLN:i:{n}" for i, n, c, d in zip(g.ids, g.lengths, g.contained, self.dropped) if not c and not d]
        out += [sg.gfa_link(r, g.ids) for r, x in zip(g.rows, self.removed) if r[6] and not x]
        return "".join(line + "\n" for line in out)


# ---- hand-made shapes: (ids, lengths, records), every read 20 000 long unless said -------------------------------------------------------

L = 20000


def line(ids, first=2000):
    """dove(ids[i], ids[i + 1]) for a chain through `ids`, all forward, with arc lengths first, first + 10, ..."""
    return [sg.dove(a, b, first + 10 * i) for i, (a, b) in enumerate(zip(ids[:-1], ids[1:]))]


def side_chain(k, mode, at=6, first_id=101, arc=3000):
    """The records of a side chain of k reads attached to read `at`: mode "out" leaves it (at -> 101 -> 102 ...), "in" enters it
    (... 102 -> 101 -> at), "rc" leaves it with the side chain's reads reverse-complemented."""
    t = list(range(first_id, first_id + k))
    if mode == "out":
        return [sg.dove(at, t[0], arc)] + line(t, 2500)
    if mode == "in":
        return [sg.dove(t[0], at, arc)] + line(t[::-1], 2500)
    assert mode == "rc"
    return [sg.dove(at, t[0], arc, rc=1)] + [sg.dove(b, a, 2500 + 10 * i) for i, (a, b) in enumerate(zip(t[:-1], t[1:]))]


def tip_on_backbone(k, mode):
    """A backbone chain of 12 reads (1 .. 12) with a side chain of k reads (101 ...) attached at read 6."""
    ids = list(range(1, 13)) + list(range(101, 101 + k))
    return ids, [L] * len(ids), np.concatenate(line(list(range(1, 13))) + side_chain(k, mode))


def terminal_fork(arm_a=2, arm_b=3, in_a=2500, in_b=2500, extras=False):
    """A chain 1 .. 8 ending in two arms, reads 11 ... (arm_a of them, the first arc inside the arm in_a long) and 21 ... (arm_b, in_b); with extras an
    isolated chain of 3 reads (ur.chain, ids 31 .. 33), the lone reads 41 and 42 and a cycle 51 .. 55 in the same table."""
    a, b = list(range(11, 11 + arm_a)), list(range(21, 21 + arm_b))
    ids, lengths = list(range(1, 9)) + a + b, [L] * (8 + arm_a + arm_b)
    recs = line(list(range(1, 9))) + [sg.dove(8, a[0], 3000)] + line(a, in_a) + [sg.dove(8, b[0], 4000)] + line(b, in_b)
    if extras:
        _, clen, _, crecs = ur.chain(3, 5, ids=[31, 32, 33])
        ids, lengths = ids + [31, 32, 33, 41, 42] + list(range(51, 56)), lengths + clen + [L, 7000] + [L] * 5
        recs += [crecs, ur.cycle(list(range(51, 56)), 9)]
    return ids, lengths, np.concatenate(recs)


def star(n_tips=70, at=1):
    """n_tips one-read tips (201 ...) entering read `at` of a backbone chain 1 .. 12."""
    ids = list(range(1, 13)) + list(range(201, 201 + n_tips))
    recs = line(list(range(1, 13))) + [sg.dove(201 + i, at, 3000 + i) for i in range(n_tips)]
    return ids, [L] * len(ids), np.concatenate(recs)


def bubble(branches=(2, 3), second_in=False, base=0, inner=None):
    """S = 1 .. 6, E = 7 .. 12 and between read 6 and read 7 one branch per entry of `branches`, of that many reads (101 ..., 111 ...,
    121 ...); second_in: read 40 enters the first read of the first branch as well.  `base` is added to every id; inner: per branch the length
    of the first arc inside it (2 500)."""
    ids, recs = list(range(1, 13)), line(list(range(1, 7))) + line(list(range(7, 13)))
    for b, k in enumerate(branches):
        t = list(range(101 + 10 * b, 101 + 10 * b + k))
        ids += t
        recs += [sg.dove(6, t[0], 3000 + 100 * b)] + line(t, inner[b] if inner else 2500) + [sg.dove(t[-1], 7, 3500)]
    if second_in:
        ids.append(40)
        recs.append(sg.dove(40, 101, 4000))
    recs = np.concatenate(recs)
    recs["from_id"] += base
    recs["to_id"] += base
    return [i + base for i in ids], [L] * len(ids), recs


def tiles():
    """1 100 reads (1 .. 1100), most of them lone; low, in the middle and high in the table a backbone of 12 with a two-read tip at
    its read 6 and, 20 reads on, a bubble with branches of 2 and 3 reads (22 reads of 40)."""
    recs = []
    for lo in (5, 540, 1030):
        b = list(range(lo, lo + 12))
        recs += line(b) + [sg.dove(b[5], lo + 12, 3000), sg.dove(lo + 12, lo + 13, 2500)]
        s, e, b2, b3 = list(range(lo + 20, lo + 26)), list(range(lo + 26, lo + 32)), [lo + 32, lo + 33], [lo + 34, lo + 35, lo + 36]
        recs += line(s) + line(e)
        for t in (b2, b3):
            recs += [sg.dove(s[-1], t[0], 3000 + t[0] % 7)] + line(t, 2500) + [sg.dove(t[-1], e[0], 3500)]
    return list(range(1, 1101)), [L] * 1100, np.concatenate(recs)


def thinned_layout(seed=2, n_reads=1100, genome=880000):
    """sg.layout with jitter 300, thinned to 60 % of its records as the unitig test thins it: (ids, lengths, reads, records)."""
    ids, lengths, reads, recs = sg.layout(seed, n_reads=n_reads, genome=genome, jitter=300)
    return ids, lengths, reads, recs[np.random.default_rng(len(recs)).random(len(recs)) < 0.6]


def cleaned_of(ids, lengths, recs, params=None, **clean):
    """(the finished graph of one add, its Cleaned)."""
    g = ur.graph_of(ids, lengths, recs, **(params or {}))
    return g, Cleaned(g, **clean)
