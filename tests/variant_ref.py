"""CPU restatement of the variant-site contract (include/mhap_hip.h, "variant sites"): the six counters per position, the site rule,
the site list and a record's judgement.  Written from the header's prose in plain Python; the views and their tally are the read
correction's (consensus_ref.py), whose counters 0 .. 5 are this stage's six.  Nothing here follows the kernels' layout or schedule.

    v = Variants(reads, ids, min_depth=.., min_minor=.., min_pct=.., max_del_pct=.., min_diff=.., diff_pct=..)
    v.add(records, op_offsets, ops)
    counts = v.finish()                      # the seven counts, in the header's order
    v.rows, v.offsets, v.sites               # int32 (n, 2), int64 (n + 1), int32 (sites, 6)
    keep, tallies = v.apply(records, op_offsets, ops)
"""
import numpy as np

import consensus_ref as cr
from align_ref import rc_bytes

ACGT = b"ACGT"
PARAMETERS = ("min_depth", "min_minor", "min_pct", "max_del_pct", "min_diff", "diff_pct")


def site_of(counters, own, p):
    """One position: counters = (A, C, G, T, del[, span]) of the votes, own = the read's byte.  Returns a dict: site, deep, major,
    minor, n_major, n_minor, depth."""
    c = [int(x) for x in counters[:4]]
    dele = int(counters[4])
    if own in ACGT:
        c[ACGT.index(own)] += 1
    depth = sum(c) + dele
    major = max(range(4), key=lambda b: (c[b], -b))                              # the greatest count, the lowest code at a tie
    minor = max((b for b in range(4) if b != major), key=lambda b: (c[b], -b))   # the same over the other three
    deep = depth >= p["min_depth"]
    site = (own in ACGT and deep and c[minor] >= p["min_minor"] and 100 * c[minor] >= p["min_pct"] * depth
            and 100 * dele <= p["max_del_pct"] * depth)
    return dict(site=bool(site), deep=bool(deep), major=major, minor=minor, n_major=c[major], n_minor=c[minor], depth=depth)


def class_of(a, b, site_a, site_b, to_rc):
    """One '=' / 'X' column: a = s1[i], b = s2[j] (the aligner's orientation), site_a / site_b = None or the (major, minor) codes of
    the site of A at i / of B at its own position.  Returns None (not informative), "agree", "disagree" or "other"."""
    if site_b is not None and to_rc:
        site_b = (3 - site_b[0], 3 - site_b[1])
    if site_a is None and site_b is None:
        return None
    if site_a is not None and site_b is not None and set(site_a) != set(site_b):
        return "other"
    pair = set(site_a if site_a is not None else site_b)
    ca = ACGT.index(a) if a in ACGT else -1
    cb = ACGT.index(b) if b in ACGT else -1
    if ca not in pair or cb not in pair:
        return "other"
    return "agree" if ca == cb else "disagree"


def keep_of(agree, disagree, p):
    return not (disagree >= p["min_diff"] and 100 * disagree >= p["diff_pct"] * (agree + disagree))


class Variants:
    def __init__(self, reads, ids, **params):
        assert set(params) == set(PARAMETERS), "every test names the six parameters"
        self.p = params
        self.reads = [bytes(r) for r in reads]
        self.cons = cr.Consensus(reads, ids)
        self.row = self.cons.row
        self.accepted = 0
        self.byte = None

    def add(self, records, op_offsets, ops):
        before = sum(self.cons.views)
        self.cons.add(records, op_offsets, ops)
        self.accepted += sum(self.cons.views) - before

    def votes(self, r):
        return self.cons.votes[r][:, :6]

    def finish(self):
        rows, sites, self.byte = [], [], []
        for r, seq in enumerate(self.reads):
            v = self.cons.votes[r]
            n_sites = n_deep = 0
            by = [None] * len(seq)
            for t in range(len(seq)):
                s = site_of(v[t, :6], seq[t], self.p)
                n_deep += s["deep"]
                if s["site"]:
                    n_sites += 1
                    by[t] = (s["major"], s["minor"])
                    sites.append((t, s["major"], s["minor"], s["n_major"], s["n_minor"], s["depth"]))
            rows.append((n_sites, n_deep))
            self.byte.append(by)
        self.rows = np.array(rows, np.int32).reshape(-1, 2)
        self.offsets = np.concatenate([[0], np.cumsum(self.rows[:, 0])]).astype(np.int64)
        self.sites = np.array(sites, np.int32).reshape(-1, 6)
        return [len(self.reads), int((self.rows[:, 0] > 0).sum()), len(sites), int(self.rows[:, 1].sum()), sum(len(r) for r in self.reads),
                self.accepted, self.cons.skipped_views]

    def judge(self, rec, runs):
        """(informative, agree, disagree, other) of one record and its runs."""
        fid, tid = int(rec["from_id"]), int(rec["to_id"])
        if not len(runs) or fid == tid:
            return (0, 0, 0, 0)
        ia, ib = self.row[fid], self.row[tid]
        to_rc = int(rec["to_rc"]) != 0
        s1, own_b = self.reads[ia], self.reads[ib]
        blen = len(own_b)
        s2 = rc_bytes(own_b) if to_rc else own_b
        i = int(rec["a1"])
        j = blen - int(rec["b2"]) - 1 if to_rc else int(rec["b1"])
        n = dict(agree=0, disagree=0, other=0)
        for r in runs:
            length, code = int(r) >> 4, int(r) & 15
            if code in (cr.OP_EQ, cr.OP_X):
                for _ in range(length):
                    k = class_of(s1[i], s2[j], self.byte[ia][i], self.byte[ib][blen - 1 - j if to_rc else j], to_rc)
                    if k is not None:
                        n[k] += 1
                    i, j = i + 1, j + 1
            elif code == cr.OP_I:
                i += length
            else:
                j += length
        return (n["agree"] + n["disagree"] + n["other"], n["agree"], n["disagree"], n["other"])

    def apply(self, records, op_offsets, ops):
        assert self.byte is not None, "finish first"
        tallies = np.zeros((len(records), 4), np.int32)
        keep = np.zeros(len(records), np.uint8)
        for q in range(len(records)):
            tallies[q] = self.judge(records[q], ops[int(op_offsets[q]):int(op_offsets[q + 1])])
            keep[q] = keep_of(int(tallies[q, 1]), int(tallies[q, 2]), self.p)
        return keep, tallies
