"""The unitig-consensus contract restated in Python from the prose of include/mhap_hip.h ("unitig consensus"): which records place a
read, the frame, the candidate and the choice, the guard, the windows, the vote as view A of the correction contract and the call
with its position map.  Plain loops over Python integers; the class of a record is string_graph_ref's, the aligner align_paths_ref's,
the views, the tally and the call consensus_ref's, all imported as they are.  Nothing here calls the library.

    res = consensus(ids, lengths, reads, records, tables, drafts, params)      # tables: unitig_ref.Unitigs.tables() (or the library's)
    res.placements   int64 (reads, 5) {unitig or -1, strand, p, how, aligned}
    res.votes[k]     int64 (ulen[k], 24)        res.seqs[k]  bytes        res.stats  int64 (unitigs, 6)
    res.maps[k]      int64 (ulen[k])            res.counts   dict of COUNT_NAMES
"""
import numpy as np

import align_paths_ref as apr
import consensus_ref as cref
import string_graph_ref as sg
from align_ref import rc_bytes

TILE = 4096
CAP = 65535
MEMBER, RECORD, UNPLACED = 0, 1, 2
COUNT_NAMES = ("members", "placed_by_record", "unplaced", "aligned", "no_alignment", "bases_in", "bases_out", "substitutions", "deletions",
               "insertions", "low")


class Refused(ValueError):
    """The run is refused (MHAP_E_INVALID in the library)."""


class Result:
    pass


def candidate(r, A, B, member, params):
    """None, or (X, xe - xs, vertex of M, p, sX): what the record r over the reads A, B proposes.  member: read -> (unitig, vertex,
    offset) for the members of the served unitigs."""
    c, _ = sg.classify(r, A, B, params)
    if c in (sg.NONE, sg.INTERNAL):
        return None
    if (A in member) == (B in member):
        return None
    ql, tl, o = int(r["alen"]), int(r["blen"]), 1 if int(r["to_rc"]) else 0
    qs, qe = int(r["a1"]), int(r["a2"]) + 1
    b1, b2 = int(r["b1"]), int(r["b2"])
    ts, te = (b1, b2 + 1) if not o else (tl - b2 - 1, tl - b1)
    # the aligner's frame: (interval, strand, length) of A and of B
    fa, fb = [qs, qe, 0, ql], [ts, te, o, tl]
    m_is_a = A in member
    _, vm, off = member[A if m_is_a else B]
    if (fa if m_is_a else fb)[2] != (vm & 1):
        fa, fb = ([f[3] - f[1], f[3] - f[0], f[2] ^ 1, f[3]] for f in (fa, fb))
    fm, fx = (fa, fb) if m_is_a else (fb, fa)
    ms, me, (xs, xe, sx, _) = fm[0], fm[1], fx
    p = ((off + ms) + (off + me) - (xs + xe)) // 2             # Python's // floors toward -infinity
    return (B if m_is_a else A), xe - xs, vm, p, sx


def place(ids, lengths, records, tables, params):
    """The placement table without its `aligned` column: int64 (reads, 5)."""
    by_id = {}
    for i, x in enumerate(ids):
        by_id.setdefault(int(x), i)
    start, ulen, circ = tables["unitig_start"].tolist(), tables["unitig_len"].tolist(), tables["circular"].tolist()
    member = {}
    for k in range(len(ulen)):
        for m in range(start[k], start[k + 1]):
            v = int(tables["vertex"][m])
            member[v >> 1] = (k, v, int(tables["offset"][m]))
    cands = {}
    for r in records:
        for fid, flen in ((int(r["from_id"]), int(r["alen"])), (int(r["to_id"]), int(r["blen"]))):
            if fid not in by_id or int(lengths[by_id[fid]]) != flen:
                raise Refused(f"a record names read {fid} with the length {flen}")
        c = candidate(r, by_id[int(r["from_id"])], by_id[int(r["to_id"])], member, params)
        if c is not None:
            cands.setdefault(c[0], []).append(c[1:])
    out = np.zeros((len(ids), 5), np.int64)
    for x in range(len(ids)):
        if x in member:
            k, v, off = member[x]
            out[x] = (k, v & 1, off, MEMBER, 0)
        elif x in cands:
            span, vm, p, sx = min(cands[x], key=lambda c: (-c[0], c[1], c[2], c[3]))
            k = member[vm >> 1][0]
            out[x] = (k, sx, p % ulen[k] if circ[k] else p, RECORD, 0)
        else:
            out[x] = (-1, 0, 0, UNPLACED, 0)
    return out


def window(p, length, ulen, band, max_shift):
    """(band, w0, w1) of a read of `length` bases placed at p."""
    band = band if band > 0 else max(1, int(length * max_shift))
    return band, max(0, p - band), min(ulen, p + length + band)


def call_unitig(draft, v, min_cov):
    """The six steps for every position of one unitig: (bytes, the six counts, the position map)."""
    L, out, pmap = len(draft), bytearray(), np.zeros(len(draft), np.int64)
    n_sub = n_del = n_ins = n_low = 0
    for t in range(L):
        pmap[t] = len(out)
        own = draft[t]
        base = [int(x) for x in v[t, 0:4]]
        dele, span = int(v[t, cref.DEL]), int(v[t, cref.SPAN])
        d = sum(base) + dele                                        # 1
        if d < min_cov:                                             # 2
            out.append(own)
            n_low += 1
        else:
            if own in cref.ACGT:                                    # 3
                base[cref.ACGT.index(own)] += 1
            total = d + 1
            if 2 * dele > total:                                    # 4
                n_del += 1
            else:                                                   # 5
                top = max(base)
                emit = own if top == 0 or (own in cref.ACGT and base[cref.ACGT.index(own)] == top) else cref.ACGT[base.index(top)]
                out.append(emit)
                n_sub += emit != own
        if t < L - 1 and span >= min_cov:                           # 6
            for k in range(cref.KI):
                ins = [int(x) for x in v[t, cref.INS0 + 4 * k:cref.INS0 + 4 * k + 4]]
                if 2 * max(ins) > span + 1:
                    out.append(cref.ACGT[ins.index(max(ins))])
                    n_ins += 1
                else:
                    break
    return bytes(out), (L, len(out), n_sub, n_del, n_ins, n_low), pmap


def consensus(ids, lengths, reads, records, tables, drafts, params=None, band=0, max_shift=0.2, min_cov=4, tile_cap=CAP):
    """Everything mhap_consensus_run computes.  reads: the stored bytes per read; drafts: the spelled bytes per served unitig."""
    params = params or sg.Params()
    res = Result()
    ulen = [int(x) for x in tables["unitig_len"]]
    assert [len(d) for d in drafts] == ulen
    for k, n in enumerate(ulen):
        if n >= 1 << 31:
            raise Refused(f"unitig {k} has {n} bases")
    pl = place(ids, lengths, records, tables, params)
    # the guard, before any vote
    tiles = [[0] * ((n + TILE - 1) // TILE) for n in ulen]
    wins = {}
    for x in range(len(ids)):
        k, strand, p, how, _ = pl[x].tolist()
        if how == UNPLACED:
            continue
        bd, w0, w1 = window(p, int(lengths[x]), ulen[k], band, max_shift)
        wins[x] = (bd, w0, w1)
        if w1 > w0:
            for j in range(w0 // TILE, (w1 - 1) // TILE + 1):
                tiles[k][j] += 1
    for k, row in enumerate(tiles):
        for j, n in enumerate(row):
            if n > tile_cap:
                raise Refused(f"unitig {k} tile {j} is met by {n} reads, more than {tile_cap}")
    pile = cref.Consensus(drafts, list(range(len(drafts))))
    counts = dict.fromkeys(COUNT_NAMES, 0)
    for x in range(len(ids)):
        k, strand, p, how, _ = pl[x].tolist()
        if how == UNPLACED:
            counts["unplaced"] += 1
            continue
        counts["members" if how == MEMBER else "placed_by_record"] += 1
        bd, w0, w1 = wins[x]
        s2 = rc_bytes(reads[x]) if strand else bytes(reads[x])
        fields, runs = apr.align_path(drafts[k][w0:w1], s2, w0 - p, bd) if w1 > w0 else (apr.NONE, [])
        if not runs:
            counts["no_alignment"] += 1
            continue
        counts["aligned"] += 1
        pl[x, 4] = 1
        view_a, _ = cref.views_of(drafts[k], s2, w0 + int(fields[1]), int(fields[3]), runs, False, len(s2))
        pile.add_view(k, view_a)
    res.placements, res.votes = pl, pile.votes
    res.seqs, res.maps, res.stats = [], [], np.zeros((len(drafts), 6), np.int64)
    for k, d in enumerate(drafts):
        seq, st, pmap = call_unitig(d, pile.votes[k], min_cov)
        assert (seq, tuple(st)) == pile.call_read(k, min_cov)      # the correction reference's own call, on the same votes
        res.seqs.append(seq)
        res.maps.append(pmap)
        res.stats[k] = st
    for name, col in zip(COUNT_NAMES[5:], range(6)):
        counts[name] = int(res.stats[:, col].sum())
    res.counts = counts
    return res


def gfa(ids, tables, seqs, maps):
    """The unitig GFA with consensus: the consensus on the S lines with its length, the `a` offsets through the position map."""
    start, circ = tables["unitig_start"].tolist(), tables["circular"].tolist()
    name = lambda k: f"utg{k + 1:06d}{'c' if circ[k] else 'l'}"
    out = ["H\tVN:Z:1.0"]
    for k, seq in enumerate(seqs):
        out.append(f"S\t{name(k)}\t{seq.decode('latin-1')}\tLN:i:{len(seq)}\tnr:i:{start[k + 1] - start[k]}")
        for m in range(start[k], start[k + 1]):
            v, sp = int(tables["vertex"][m]), int(tables["span"][m])
            out.append(f"a\t{name(k)}\t{int(maps[k][int(tables['offset'][m])])}\t{int(ids[v >> 1])}:1-{sp}\t{'-' if v & 1 else '+'}\t{sp}")
    out += [f"L\t{name(fu)}\t{'-' if fo else '+'}\t{name(tu)}\t{'-' if to else '+'}\t{ol}M" for fu, fo, tu, to, ol, _ in np.asarray(tables["links"]).reshape(-1, 6).tolist()]
    return "".join(line + "\n" for line in out)


# ---- fabricated inputs ------------------------------------------------------------------------------------------------------------------

def line_layout(reads, ids=None, min_shared=200, pairs=None):
    """Records from truth positions: reads = [(start, end, strand)] on a line; one record (string_graph_ref.placed) per pair that
    shares at least min_shared positions (or per pair of `pairs`), the lower index as `from`.  Returns the records."""
    ids = ids or list(range(1, len(reads) + 1))
    recs = []
    for i in range(len(reads)):
        for j in range(i + 1, len(reads)):
            if pairs is not None and (i, j) not in pairs:
                continue
            if min(reads[i][1], reads[j][1]) - max(reads[i][0], reads[j][0]) >= min_shared:
                recs.append(sg.placed(ids[i], ids[j], reads[i], reads[j]))
    return np.concatenate(recs) if recs else np.zeros(0, sg.RECORD_DTYPE)


def cut_reads(genome, reads):
    """The stored bytes of reads = [(start, end, strand)] cut from `genome` without errors."""
    return [rc_bytes(genome[s:e]) if f else bytes(genome[s:e]) for s, e, f in reads]
