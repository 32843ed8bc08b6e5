"""CPU restatement of the "quality-weighted votes" contract of include/mhap_hip.h, on top of consensus_ref's views and tally: the
weight of a base, the weighted votes of a view, the 21 845-view cap, the call and the output qualities in weighted units.  Plain loops
over Python integers, written from the header's prose.

    c = WeightedConsensus(reads, quals, ids, q_lo, q_hi)     # quals: one Phred array per read
    c.add(records, op_offsets, ops)
    seqs, stats = c.call(min_cov=4)                          # c.votes[r]: int64 (len, 24), the weighted counters
    seq, q = call(own_seq, own_q, votes, min_cov, per_vote, cap, q_lo, q_hi)     # own_q None: the unitig consensus (own weighs 2)

weighted_workload(seed) is consensus_ref.quality_workload's generator with a per-base error model and reported qualities."""
import numpy as np

import consensus_ref as cref
from align_ref import rc_bytes
from consensus_ref import ACGT, DEL, INS0, KI, NCOUNT, SPAN

NEUTRAL = 2
CAP = 65535 // 3                          # 21 845 accepted views per target
CANDIDATES = ((5, 15), (7, 20), (10, 20), (10, 30))   # the (q_lo, q_hi) pairs the defaults were chosen among
DEFAULT_Q_LO, DEFAULT_Q_HI = 7, 20


def check_weights(q_lo, q_hi):
    if not 0 <= q_lo <= q_hi <= 93:
        raise ValueError(f"the weights need 0 <= q_lo <= q_hi <= 93 ({q_lo}, {q_hi})")


def weight(q, q_lo, q_hi):
    """1 below q_lo, 2 from q_lo up to q_hi, 3 from q_hi on."""
    return 1 if q < q_lo else 2 if q < q_hi else 3


def views_with_qualities(s1, q1, sb, qb, i0, j0, runs, to_rc):
    """consensus_ref.views_of's two views with the quality of every evidence byte appended to its column: ("M", t, e, q),
    ("Ins", e, q), ("Del", t).  s1, sb: reads A and B as stored; q1, qb: their qualities.  The quality is that of the stored byte the
    evidence came from: a second walk of views_of over stored positions instead of bytes finds it."""
    blen = len(sb)
    va, vb = cref.views_of(s1, rc_bytes(sb) if to_rc else sb, i0, j0, runs, to_rc, blen)
    stored_b = [blen - 1 - j for j in range(blen)] if to_rc else list(range(blen))   # column j of s2 is this byte of B
    pa, pb = cref.views_of(list(range(len(s1))), stored_b, i0, j0, runs, False, blen)
    if to_rc:
        pb = pb[::-1]

    def attach(view, where, quals):
        out = []
        for col, pos in zip(view, where):
            assert col[0] == pos[0]
            out.append(col if col[0] == "Del" else col + (int(quals[pos[-1]]),))
        return out
    return attach(va, pa, qb), attach(vb, pb, q1)


def tally_weighted(view, q_lo, q_hi):
    """The (t, counter, weight) increments of one view with qualities: consensus_ref.tally's votes, each with its weight."""
    out = []
    t_prev, k = None, 0
    for col in view:
        if col[0] == "Ins":
            if k < KI and col[1] in ACGT:
                out.append((t_prev, INS0 + 4 * k + ACGT.index(col[1]), weight(col[2], q_lo, q_hi)))
            k += 1
            continue
        t = col[1]
        if t_prev is not None:
            out.append((t_prev, SPAN, NEUTRAL))
        if col[0] == "M":
            if col[2] in ACGT:
                out.append((t, ACGT.index(col[2]), weight(col[3], q_lo, q_hi)))
        else:
            out.append((t, DEL, NEUTRAL))
        t_prev, k = t, 0
    return out


def position(row, own, own_w, t, L, min_cov):
    """What position t emits under the weighted call: a list of (byte, margin in weighted units, or None for the fixed quality 0)."""
    base = [int(x) for x in row[0:4]]
    dele, span = int(row[DEL]), int(row[SPAN])
    ins = [[int(x) for x in row[INS0 + 4 * k:INS0 + 4 * k + 4]] for k in range(KI)]
    d = sum(base) + dele
    n = d + own_w
    with_own = list(base)
    if own in ACGT:
        with_own[ACGT.index(own)] += own_w
    out = []
    if d < NEUTRAL * min_cov:
        e = own
    elif 2 * dele > n:
        e = None
    else:
        top = max(with_own)
        e = own if top == 0 or (own in ACGT and with_own[ACGT.index(own)] == top) else ACGT[with_own.index(top)]
    if e is not None:
        if e in ACGT:
            s = base[ACGT.index(e)] + (own_w if own == e else 0)
            out.append((e, 2 * s - n))
        else:
            out.append((e, None))
    n_ins = 0
    if t < L - 1 and span >= NEUTRAL * min_cov:
        for k in range(KI):
            m = max(ins[k])
            if 2 * m <= span + NEUTRAL:
                break
            out.append((ACGT[ins[k].index(m)], 2 * m - (span + NEUTRAL)))
            n_ins += 1
    if out and t < L - 1 and n_ins < KI and out[-1][1] is not None:
        m_stop = (span + NEUTRAL) - 2 * max(ins[n_ins])
        out[-1] = (out[-1][0], min(out[-1][1], m_stop))
    return out


def q_of(m, per_vote=15, cap=60):
    """Q = min(cap, per_vote * max(m, 0) / 20), C integer division."""
    return min(cap, per_vote * max(m, 0) // 20)


def call(own_seq, own_q, votes, min_cov=4, per_vote=15, cap=60, q_lo=DEFAULT_Q_LO, q_hi=DEFAULT_Q_HI):
    """(bytes, qualities as uint8, the four counts sub, del, ins, low) of one read (own_q: its Phred values) or unitig (own_q None)."""
    check_weights(q_lo, q_hi)
    L = len(own_seq)
    seq, quals = bytearray(), []
    n_sub = n_del = n_ins = n_low = 0
    for t in range(L):
        own_w = NEUTRAL if own_q is None else weight(int(own_q[t]), q_lo, q_hi)
        row = votes[t]
        out = position(row, own_seq[t], own_w, t, L, min_cov)
        d = int(sum(row[0:4])) + int(row[DEL])
        low = d < NEUTRAL * min_cov
        called = (not low) and 2 * int(row[DEL]) > d + own_w
        n_low += low
        n_del += called
        n_base = 0 if called else 1
        n_ins += len(out) - n_base
        if n_base:
            n_sub += out[0][0] != own_seq[t]
        for e, m in out:
            seq.append(e)
            quals.append(0 if m is None else q_of(m, per_vote, cap))
    return bytes(seq), np.array(quals, np.uint8), (n_sub, n_del, n_ins, n_low)


class WeightedConsensus:
    """consensus_ref.Consensus with qualities: the same records, views and arrival order, weighted votes, the cap of 21 845."""

    def __init__(self, reads, quals, ids, q_lo=DEFAULT_Q_LO, q_hi=DEFAULT_Q_HI):
        check_weights(q_lo, q_hi)
        self.reads = [bytes(r) for r in reads]
        self.quals = [np.asarray(q, np.uint8) for q in quals]
        assert [len(r) for r in self.reads] == [len(q) for q in self.quals]
        self.q_lo, self.q_hi = q_lo, q_hi
        self.row = {}
        for k, i in enumerate(ids):
            self.row.setdefault(int(i), k)
        self.votes = [np.zeros((len(r), NCOUNT), np.int64) for r in self.reads]
        self.views = [0] * len(self.reads)
        self.skipped_views = 0

    def add_view(self, target, view):
        """One view with qualities (views_with_qualities' columns) on read `target`, through the cap."""
        if self.views[target] >= CAP:
            self.skipped_views += 1
            return
        self.views[target] += 1
        incs = np.array(tally_weighted(view, self.q_lo, self.q_hi), np.int64).reshape(-1, 3)
        np.add.at(self.votes[target], (incs[:, 0], incs[:, 1]), incs[:, 2])

    def add(self, records, op_offsets, ops, views=None):
        for q in range(len(records)):
            rec = records[q]
            runs = tuple(int(x) for x in ops[int(op_offsets[q]):int(op_offsets[q + 1])])
            fid, tid = int(rec["from_id"]), int(rec["to_id"])
            if not runs or fid == tid:
                continue
            ia, ib = self.row[fid], self.row[tid]
            to_rc = int(rec["to_rc"]) != 0
            blen = len(self.reads[ib])
            i0 = int(rec["a1"])
            j0 = blen - int(rec["b2"]) - 1 if to_rc else int(rec["b1"])
            va, vb = views_with_qualities(self.reads[ia], self.quals[ia], self.reads[ib], self.quals[ib], i0, j0, runs, to_rc)
            if views is None or views[q] & 1:
                self.add_view(ia, va)
            if views is None or views[q] & 2:
                self.add_view(ib, vb)

    def call_read(self, r, min_cov=4, per_vote=15, cap=60):
        seq, quals, (n_sub, n_del, n_ins, n_low) = call(self.reads[r], self.quals[r], self.votes[r], min_cov, per_vote, cap, self.q_lo, self.q_hi)
        return seq, (len(self.reads[r]), len(seq), n_sub, n_del, n_ins, n_low), quals

    def call(self, min_cov=4):
        seqs, stats = [], np.zeros((len(self.reads), 6), np.int32)
        for r in range(len(self.reads)):
            s, st, _ = self.call_read(r, min_cov)
            seqs.append(s)
            stats[r] = st
        return seqs, stats


# ---- the weighted workload: quality_workload's genome, reads and pairs with a per-base error model --------------------------------------

GOOD_SHARE, GOOD_P, GOOD_Q, BAD_P, BAD_Q = 0.7, 0.04, 14, 0.30, 5


def weighted_workload(seed, genome_len=2500, n_reads=36, mix=(0.79, 0.12, 0.09), min_shared=200, band=150):
    """(reads, quals, truths, bases, pairs7, meta) as consensus_ref.quality_workload gives them, plus one Phred array per read.  Every
    source position of a read is independently good (probability 0.7: error 0.04, reported Q14) or not (error 0.30, reported Q5),
    0.118 overall, split into insertions, deletions and substitutions by `mix`; an inserted byte is reported Q5."""
    rng = np.random.default_rng(seed)
    genome = bytes(rng.choice(list(ACGT), genome_len).tolist())
    reads, quals, truths, place = [], [], [], []
    for _ in range(n_reads):
        want = int(rng.integers(600, 1000))
        start = int(rng.integers(0, genome_len - want))
        seg = genome[start:start + want]
        strand = int(rng.integers(0, 2))
        src = rc_bytes(seg) if strand else seg
        out, q = bytearray(), []
        for c in src:
            good = rng.random() < GOOD_SHARE
            p, rep = (GOOD_P, GOOD_Q) if good else (BAD_P, BAD_Q)
            p_ins, p_del, p_sub = (p * m for m in mix)
            u = rng.random()
            while u < p_ins:                     # an inserted base, then the same source base again
                out.append(int(rng.choice(list(ACGT))))
                q.append(BAD_Q)
                u = rng.random()
            if u < p_ins + p_del:
                continue
            if u < p_ins + p_del + p_sub:
                out.append(int(rng.choice([x for x in ACGT if x != c])))
            else:
                out.append(c)
            q.append(rep)
        reads.append(bytes(out))
        quals.append(np.array(q, np.uint8))
        truths.append(bytes(src))
        place.append((start, start + want, strand))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bases = np.frombuffer(b"".join(reads), np.uint8)
    pairs, meta = [], []
    for x in range(n_reads):
        for y in range(x + 1, n_reads):
            (sa, ea, ta), (sb, eb, tb) = place[x], place[y]
            lo, hi = max(sa, sb), min(ea, eb)
            if hi - lo < min_shared:
                continue
            g = (lo + hi) / 2.0
            la, lb = len(reads[x]), len(reads[y])
            i = ((ea - g) if ta else (g - sa)) * la / (ea - sa)
            j = ((eb - g) if ta else (g - sb)) * lb / (eb - sb)
            pairs.append((offsets[x], la, offsets[y], lb, int(ta != tb), int(round(j - i)), band))
            meta.append((x, y, int(ta != tb)))
    return reads, quals, truths, bases, np.array(pairs, np.int64).reshape(-1, 7), meta


# ---- the unitig consensus: unitig_consensus_ref's placement, windows and paths, view A with the reads' qualities ------------------------

def unitig_votes(ids, lengths, reads, quals, records, tables, drafts, params, band=0, max_shift=0.2, q_lo=DEFAULT_Q_LO, q_hi=DEFAULT_Q_HI):
    """The weighted counters of every served unitig, int64 (len, 24) each: every placed read aligned to its window of the draft as
    unitig_consensus_ref.consensus aligns it, voting as view A with its own qualities."""
    import align_paths_ref as apr
    import unitig_consensus_ref as ucr
    pl = ucr.place(ids, lengths, records, tables, params)
    pile = WeightedConsensus(drafts, [np.zeros(len(d), np.uint8) for d in drafts], range(len(drafts)), q_lo, q_hi)
    for x in range(len(ids)):
        k, strand, p, how, _ = pl[x].tolist()
        if how == ucr.UNPLACED:
            continue
        bd, w0, w1 = ucr.window(p, int(lengths[x]), len(drafts[k]), band, max_shift)
        s2 = rc_bytes(reads[x]) if strand else bytes(reads[x])
        fields, runs = apr.align_path(drafts[k][w0:w1], s2, w0 - p, bd) if w1 > w0 else (apr.NONE, [])
        if not runs:
            continue
        va, _ = views_with_qualities(drafts[k], pile.quals[k], bytes(reads[x]), quals[x], w0 + int(fields[1]), int(fields[3]), runs, bool(strand))
        pile.add_view(k, va)
    return pile.votes
