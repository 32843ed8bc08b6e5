"""The "base qualities" paragraph of include/mhap_hip.h restated in Python: one quality byte per byte that the call of the read
correction or of the unitig consensus emits, from the position's 24 counters, the own byte, min_cov and (per_vote, cap).  Plain loops
over Python integers, written from the header's prose; the call itself is restated here too, so that the bytes the qualities go
with are this file's own, and the tests compare them with consensus_ref's and unitig_consensus_ref's.

    seq, quals = call(own_seq, votes, min_cov=4, per_vote=15, cap=60)     # votes: int (len, 24), the order of mhap_correct_votes
    hist = histogram([quals, ...])                                        # int64 (94)
    wrong = wrong_bytes(seq, truth)                                       # bool per byte of seq, by difflib's matching blocks
"""
import difflib

import numpy as np

ACGT = b"ACGT"
KI = 4
DEL, SPAN, INS0 = 4, 5, 6
BINS = 94
DEFAULT_PER_VOTE, DEFAULT_CAP = 15, 60


def q_of(m, per_vote=DEFAULT_PER_VOTE, cap=DEFAULT_CAP):
    """Q(m) = min(cap, per_vote * max(m, 0) / 10), C integer division (the operands are never negative)."""
    return min(cap, per_vote * max(m, 0) // 10)


def check_params(per_vote, cap):
    if not (1 <= per_vote <= 1000 and 1 <= cap <= 93):
        raise ValueError(f"per_vote must be 1 .. 1000 and cap 1 .. 93 ({per_vote}, {cap})")


def position(row, own, t, L, min_cov):
    """What position t emits: a list of (byte, margin or None); None is the fixed quality 0 of a byte that is not A, C, G or T."""
    base = [int(x) for x in row[0:4]]
    dele, span = int(row[DEL]), int(row[SPAN])
    ins = [[int(x) for x in row[INS0 + 4 * k:INS0 + 4 * k + 4]] for k in range(KI)]
    d = sum(base) + dele
    n = d + 1
    with_own = list(base)
    if own in ACGT:
        with_own[ACGT.index(own)] += 1
    out = []
    if d < min_cov:
        e = own
    elif 2 * dele > n:
        e = None
    else:
        top = max(with_own)
        e = own if top == 0 or (own in ACGT and with_own[ACGT.index(own)] == top) else ACGT[with_own.index(top)]
    if e is not None:
        if e in ACGT:
            s = base[ACGT.index(e)] + (1 if own == e else 0)
            out.append((e, 2 * s - n))
        else:
            out.append((e, None))
    n_ins = 0
    if t < L - 1 and span >= min_cov:
        for k in range(KI):
            m = max(ins[k])
            if 2 * m <= span + 1:
                break
            out.append((ACGT[ins[k].index(m)], 2 * m - (span + 1)))
            n_ins += 1
    if out and t < L - 1 and n_ins < KI and out[-1][1] is not None:
        m_stop = (span + 1) - 2 * max(ins[n_ins])
        out[-1] = (out[-1][0], min(out[-1][1], m_stop))
    return out


def call(own_seq, votes, min_cov=4, per_vote=DEFAULT_PER_VOTE, cap=DEFAULT_CAP):
    """(the emitted bytes, their qualities as a uint8 array) of one read or one unitig."""
    check_params(per_vote, cap)
    L = len(own_seq)
    seq, quals = bytearray(), []
    for t in range(L):
        for e, m in position(votes[t], own_seq[t], t, L, min_cov):
            seq.append(e)
            quals.append(0 if m is None else q_of(m, per_vote, cap))
    return bytes(seq), np.array(quals, np.uint8)


def histogram(quals):
    h = np.zeros(BINS, np.int64)
    for q in quals:
        h += np.bincount(np.asarray(q, np.int64), minlength=BINS)
    return h


def counts_line(hist):
    """The stderr line of the tools, from the histogram."""
    h = [int(x) for x in hist]
    n = sum(h)
    mean = sum(q * c for q, c in enumerate(h)) / n if n else 0.0
    return f"Qualities: {n} bytes, {sum(h[:10])} below Q10, {sum(h[:20])} below Q20, mean {mean:.1f}"


def wrong_bytes(seq, truth):
    """True for every byte of seq that no matching block of difflib's (autojunk off) pairs with a byte of truth."""
    ok = np.zeros(len(seq), bool)
    for a, _, size in difflib.SequenceMatcher(None, seq, truth, autojunk=False).get_matching_blocks():
        ok[a:a + size] = True
    return ~ok


def ranking(quals, wrongs):
    """(median quality, (wrong, bytes) below the median, (wrong, bytes) at or above it) over all bytes of the given sequences."""
    q = np.concatenate([np.asarray(x, np.int64) for x in quals])
    w = np.concatenate(wrongs)
    med = int(np.median(q))
    lo = q < med
    return med, (int(w[lo].sum()), int(lo.sum())), (int(w[~lo].sum()), int((~lo).sum()))
