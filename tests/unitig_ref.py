"""The unitig contract restated in Python from the prose of include/mhap_hip.h ("unitigs", in the string-graph section): the joined
arcs, the chains and cycles of `next`, the kept orientation and the numbering, the layout, the spelled sequences, the links, the
counts and the GFA text.  The input is the arc rows of string_graph_ref.Graph.finish() with the contained flags and the read lengths;
plain loops over Python integers, and nothing here calls the library.  Also the fabricated inputs of the unitig tests: bases planted
on the reads of a line, chains, cycles and the hand-made forks."""
import numpy as np

import string_graph_ref as sg

COUNT_NAMES = ("unitigs", "circular", "members", "joined_arcs", "links", "longest_bases", "total_bases")


def rc_byte(c):
    """Utils.rc's table on one byte value: a-z are upper-cased, the IUPAC letters complemented, everything else unchanged."""
    if ord("a") <= c <= ord("z"):
        c = c - ord("a") + ord("A")
    pairs = "ATBVCGDHGCHDKMMKNNRYSSTAVBWWYR"
    table = {ord(pairs[i]): ord(pairs[i + 1]) for i in range(0, len(pairs), 2)}
    return table.get(c, c)


RC_TABLE = bytes(rc_byte(c) for c in range(256))


def revcomp(b):
    return bytes(b)[::-1].translate(RC_TABLE)


class Unitigs:
    """rows: [u, v, len, ol, q, reduced, final] per arc; contained, lengths: per read."""

    def __init__(self, rows, contained, lengths):
        rows = [[int(x) for x in r] for r in rows]
        lengths = [int(x) for x in lengths]
        n = len(lengths)
        fin = {}                                            # u -> [(v, len, arc index)] over the final arcs
        for i, r in enumerate(rows):
            if r[6]:
                assert r[0] >> 1 != r[1] >> 1               # no arc joins the strands of one read
                fin.setdefault(r[0], []).append((r[1], r[2], i))
        outdeg = lambda v: len(fin.get(v, []))
        in_play = [v for v in range(2 * n) if not contained[v >> 1]]
        for v, ws in fin.items():
            assert not contained[v >> 1] and all(not contained[w >> 1] for w, _, _ in ws)
        nxt, prev, span, joined = {}, {}, {}, set()
        for v in in_play:
            span[v] = lengths[v >> 1]
            if outdeg(v) == 1:
                w, ln, i = fin[v][0]
                if outdeg(w ^ 1) == 1:
                    assert w not in prev and 1 <= ln < lengths[v >> 1]
                    nxt[v], prev[w], span[v] = w, v, ln
                    joined.add(i)
        for v, w in nxt.items():
            assert nxt.get(w ^ 1) == v ^ 1                  # the twin symmetry of next
        self.next, self.prev = nxt, prev
        chains, seen = [], set()
        for v in in_play:                                   # the maximal chains, from their heads
            if v not in prev:
                c = [v]
                while c[-1] in nxt:
                    c.append(nxt[c[-1]])
                chains.append((c, 0))
                seen.update(c)
        for v in in_play:                                   # what is left lies on cycles; ascending, so v is its cycle's smallest
            if v not in seen:
                c = [v]
                while nxt[c[-1]] != v:
                    c.append(nxt[c[-1]])
                chains.append((c, 1))
                seen.update(c)
        assert len(seen) == len(in_play) and sum(len(c) for c, _ in chains) == len(in_play)
        kept = []
        for c, circ in chains:
            assert len({x >> 1 for x in c}) == len(c)       # a chain and its twin share no read
            if (c[0] < min(x ^ 1 for x in c)) if circ else (c[0] < c[-1] ^ 1):
                kept.append((c, circ))
        assert 2 * len(kept) == len(chains)
        kept.sort(key=lambda t: t[0][0])
        self.unitig_start, self.unitig_len, self.circular = [0], [], []
        self.vertex, self.offset, self.span = [], [], []
        where = {}                                          # vertex -> (unitig, orient, is head, is tail) in that orientation
        for k, (c, circ) in enumerate(kept):
            at = 0
            for i, v in enumerate(c):
                self.vertex.append(v)
                self.offset.append(at)
                self.span.append(span[v])
                at += span[v]
                where[v] = (k, 0, i == 0, i == len(c) - 1)
                where[v ^ 1] = (k, 1, i == len(c) - 1, i == 0)
            self.unitig_start.append(len(self.vertex))
            self.unitig_len.append(at)
            self.circular.append(circ)
        self.links = []
        for i, r in enumerate(rows):
            if r[6] and i not in joined:
                (fu, fo, _, f_tail), (tu, to, t_head, _) = where[r[0]], where[r[1]]
                assert f_tail and t_head and not self.circular[fu] and not self.circular[tu]
                self.links.append([fu, fo, tu, to, r[3], i])
        self.counts = dict(zip(COUNT_NAMES, [len(kept), sum(self.circular), len(self.vertex), len(joined), len(self.links),
                                             max(self.unitig_len, default=0), sum(self.unitig_len)]))

    def tables(self):
        """The arrays as the library returns them."""
        return dict(unitig_start=np.array(self.unitig_start, np.int64), unitig_len=np.array(self.unitig_len, np.int64),
                    circular=np.array(self.circular, np.uint8), vertex=np.array(self.vertex, np.int32), offset=np.array(self.offset, np.int64),
                    span=np.array(self.span, np.int32), links=np.array(self.links, np.int32).reshape(-1, 6), counts=dict(self.counts))

    def sequences(self, bases, offsets, lengths):
        """One bytes per unitig: the first span bytes of every member's read in the member's orientation."""
        bases = bytes(bases)
        out = []
        for k in range(len(self.unitig_len)):
            parts = []
            for m in range(self.unitig_start[k], self.unitig_start[k + 1]):
                v, sp = self.vertex[m], self.span[m]
                read = bases[int(offsets[v >> 1]):int(offsets[v >> 1]) + int(lengths[v >> 1])]
                assert len(read) == int(lengths[v >> 1]) and sp <= len(read)
                parts.append((revcomp(read) if v & 1 else read)[:sp])
            out.append(b"".join(parts))
            assert len(out[-1]) == self.unitig_len[k]
        return out

    def gfa(self, ids, seqs):
        out = ["H\tVN:Z:1.0"]
        name = lambda k: f"utg{k + 1:06d}{'c' if self.circular[k] else 'l'}"
        for k, seq in enumerate(seqs):
            out.append(f"S\t{name(k)}\t{seq.decode('latin-1')}\tLN:i:{self.unitig_len[k]}\tnr:i:{self.unitig_start[k + 1] - self.unitig_start[k]}")
            for m in range(self.unitig_start[k], self.unitig_start[k + 1]):
                v, sp = self.vertex[m], self.span[m]
                out.append(f"a\t{name(k)}\t{self.offset[m]}\t{int(ids[v >> 1])}:1-{sp}\t{'-' if v & 1 else '+'}\t{sp}")
        out += [f"L\t{name(fu)}\t{'-' if fo else '+'}\t{name(tu)}\t{'-' if to else '+'}\t{ol}M" for fu, fo, tu, to, ol, _ in self.links]
        return "".join(line + "\n" for line in out)


def of_graph(g):
    """The unitigs of a string_graph_ref.Graph after its finish()."""
    return Unitigs(g.rows, g.contained, g.lengths)


# ---- fabricated inputs ------------------------------------------------------------------------------------------------------------------

def draw_bases(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def plant(reads, seed, genome_len=None):
    """Bases for reads [(start, end, strand)] placed on a line: a genome is drawn and read i is genome[start:end], reverse-complemented
    for strand 1.  Returns (genome, bases, offsets): the reads back to back in `bases`, read i at offsets[i]."""
    genome = draw_bases(genome_len if genome_len is not None else max((e for _, e, _ in reads), default=0), seed)
    parts = [revcomp(genome[s:e]) if f else genome[s:e] for s, e, f in reads]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])])[:len(parts)].astype(np.int64)
    return genome, np.frombuffer(b"".join(parts), np.uint8), offsets


def random_bases(lengths, seed, pad=0):
    """Unrelated bases for reads of the given lengths (layouts whose overlaps are only claimed): (bases, offsets), `pad` bytes in front."""
    lengths = [int(x) for x in lengths]
    offsets = (pad + np.concatenate([[0], np.cumsum(lengths)])[:len(lengths)]).astype(np.int64)
    return np.frombuffer(draw_bases(pad + sum(lengths), seed), np.uint8), offsets


def chain(n, seed, ids=None):
    """n reads on a line with drawn strands and lengths, each overlapping the next by at least 2 100 positions and no other, none
    contained: one record per consecutive pair, which of the two is `from` drawn.  Returns (ids, lengths, reads, records)."""
    rng = np.random.default_rng(seed)
    ids = list(ids) if ids is not None else list(range(1, n + 1))
    reads, s = [], 0
    for _ in range(n):
        ln = int(rng.integers(5000, 6001))
        reads.append((s, s + ln, int(rng.integers(0, 2))))
        s += int(rng.integers(2000, 2901))
    recs = []
    for i in range(n - 1):
        x, y = (i, i + 1) if rng.integers(0, 2) else (i + 1, i)
        recs.append(sg.placed(ids[x], ids[y], reads[x], reads[y]))
    recs = np.concatenate(recs) if recs else np.zeros(0, sg.RECORD_DTYPE)
    return ids, [e - s for s, e, _ in reads], reads, recs


def cycle(ids, seed, read_len=20000):
    """A cycle through the reads `ids` in the given order, all forward: dove(ids[i], ids[i + 1]) and dove(ids[-1], ids[0]) with drawn
    arc lengths.  Returns the records; every read has the length read_len."""
    rng = np.random.default_rng(seed)
    n = len(ids)
    return np.concatenate([sg.dove(ids[i], ids[(i + 1) % n], int(rng.integers(1000, 15001)), read_len=read_len) for i in range(n)])


def forks():
    """(ids, lengths, records): three two-read unitigs and four links, both orientations on the link ends."""
    recs = np.concatenate([sg.dove(1, 2, 3000), sg.dove(1, 3, 5000), sg.dove(2, 4, 2000), sg.dove(3, 5, 2000, rc=1), sg.dove(6, 1, 2500)])
    return list(range(1, 7)), [20000] * 6, recs


def graph_of(ids, lengths, recs, **params):
    """The finished string_graph_ref.Graph of one add."""
    g = sg.Graph(ids, lengths, sg.Params(**params))
    g.add(recs)
    g.finish()
    return g
