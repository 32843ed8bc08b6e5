"""Inputs of the homopolymer-compression tests: the noisy reads of the motivating figure, random records with the edge positions, and
the tables of crafted reads whose shapes come from the two constants of the kernels (api.HPC_TILE, api.HPC_SCAN_BLOCK)."""
import numpy as np

from mhap_amd import api

import hpc_ref as ref

ACGT = np.frombuffer(b"ACGT", np.uint8)


def rec(f, t, a1, a2, alen, b1, b2, blen, to_rc, score=0.9, raw=40.0):
    r = np.zeros(1, api.RECORD_DTYPE)
    r["from_id"], r["to_id"], r["score"], r["raw"] = f, t, score, raw
    r["a1"], r["a2"], r["alen"], r["b1"], r["b2"], r["blen"], r["to_rc"] = a1, a2, alen, b1, b2, blen, to_rc
    return r[0]


def run_length_noise(x, p, rng):
    """Every run lengthened by one with probability p, and shortened by one with probability p if it is longer than 1."""
    heads, start = ref.compress_read(x)
    runs = np.diff(start).astype(np.int64)
    longer = rng.random(len(runs)) < p
    shorter = (rng.random(len(runs)) < p) & (runs > 1)   # (the two draws are independent: a run may get both and keep its length)
    return np.repeat(heads, runs + longer - shorter)


def noisy_reads(p, seed, n=40, length=4000, genome=30000):
    """n reads of `length` genome bases from a random genome, each with run-length noise of its own at rate p, every second one
    reverse-complemented.  Returns (FastaData with ids 1..n, the set of true pairs (id, id) sharing at least 1 000 genome bases)."""
    rng = np.random.default_rng(seed)
    g = ACGT[rng.integers(0, 4, genome)]
    begin = rng.integers(0, genome - length + 1, n)
    seqs = []
    for r in range(n):
        x = run_length_noise(g[begin[r]:begin[r] + length], p, rng)
        seqs.append(ref.revcomp(x) if r & 1 else x)
    true = {(a + 1, b + 1) for a in range(n) for b in range(a + 1, n)
            if min(begin[a], begin[b]) + length - max(begin[a], begin[b]) >= 1000}
    return table(seqs), true


def table(seqs, ids=None):
    """Reads back to back as a FastaData (empty reads kept, which FastaData.from_strings would drop)."""
    lengths = np.array([len(s) for s in seqs], np.int32)
    offsets = np.zeros(len(seqs), np.int64)
    if len(seqs):
        offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
    bases = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return api.FastaData(bases, offsets, lengths, np.arange(1, len(seqs) + 1, dtype=np.int64) if ids is None else ids)


def pairs_of(records):
    return {(min(a, b), max(a, b)) for a, b in zip(records["from_id"].tolist(), records["to_id"].tolist())}


def pairs_of_lines(lines):
    """The pairs of the driver's 12-column lines (ids as the driver numbers the reads)."""
    return {(min(int(l.split()[0]), int(l.split()[1])), max(int(l.split()[0]), int(l.split()[1]))) for l in lines}


def random_records(rng, ref_from, ref_to, n):
    """Records in compressed coordinates between random reads of the two sides: the ends drawn from -1, 0, clen - 1, clen and anywhere,
    both values of to_rc."""
    out = np.zeros(n, api.RECORD_DTYPE)
    for q in range(n):
        ends = []
        for side in (ref_from, ref_to):
            r = int(rng.integers(0, len(side["clen"])))
            c = int(side["clen"][r])
            pick = lambda: int(rng.choice([-1, 0, c - 1, c, int(rng.integers(-1, c + 1))]))
            ends.append((int(side["fasta"].ids[r]), pick(), pick(), c))
        (f, a1, a2, alen), (t, b1, b2, blen) = ends
        out[q] = rec(f, t, a1, a2, alen, b1, b2, blen, q & 1, score=float(rng.random()), raw=float(rng.integers(0, 500)))
    return out


def alternating(n, phase=0):
    """n bytes of which no two neighbours are equal."""
    return ACGT[(np.arange(n) + phase) & 3]


def with_run(n, begin, end, byte=ord("N")):
    x = alternating(n).copy()
    x[begin:end] = byte
    return x


def runs_of(rng, n, alphabet, mean=3):
    """About n bytes: runs of random lengths over the alphabet, cut to n."""
    k = n // mean + 2
    x = np.repeat(np.asarray(alphabet, np.uint8)[rng.integers(0, len(alphabet), k)], rng.integers(1, 2 * mean, k))
    while len(x) < n:
        x = np.concatenate([x, x])
    return x[:n]


def crafted_table(T, seed=5):
    """The table of crafted reads: every length around the wave, the lane and the tile, runs across every such edge, odd bytes, reads
    at every offset modulo 16 with the byte in front equal to their first, neighbours that share a byte at the seam, rows out of
    order, a row given twice and a row inside another."""
    rng = np.random.default_rng(seed)
    reads = []
    for L in (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1):
        reads.append(np.full(L, ord("A"), np.uint8))          # clen 1: no head in any tile after the first
        reads.append(alternating(L, L))                       # clen L
    for edge in list(range(14, 19)) + list(range(62, 67)) + list(range(T - 2, T + 3)):
        reads.append(with_run(2 * T + 1, edge - 5, edge))     # a run that ends in front of `edge`
        reads.append(with_run(T + 40, edge, edge + 3) if edge + 3 <= T + 40 else with_run(2 * T + 1, edge, edge + 3))   # and one that begins there
    reads.append(with_run(2 * T + 1, T - 1, T + 1))           # from a tile's last base to the next tile's first
    reads.append(with_run(5 * T + 7, T, 4 * T))               # three whole tiles
    reads.append(with_run(5 * T + 7, T - 1, 4 * T + 1))
    odd = [ord("N"), ord("n"), ord("a"), ord("A"), ord("c"), 0x00, 0xFF]
    reads.append(runs_of(rng, T + 37, odd))
    reads.append(runs_of(rng, 3 * T - 1, odd, mean=9))
    for m in range(16):                                       # long enough for two tiles, at every misalignment (placed below)
        reads.append(runs_of(rng, T + 1 + 3 * m, ACGT))
    # placement: read i begins at an offset = i (mod 16), behind a gap filled with its own first byte
    chunks, offsets, at = [], [], 0
    for i, x in enumerate(reads):
        gap = (i - at) % 16 or 16
        chunks.append(np.full(gap, x[0] if len(x) else ord("A"), np.uint8))
        at += gap
        offsets.append(at)
        chunks.append(x)
        at += len(x)
    # two reads with nothing between them, the second beginning with the byte the first ends with
    for x in (np.frombuffer(b"ACCGTTA", np.uint8), np.frombuffer(b"AAGC", np.uint8)):
        offsets.append(at)
        chunks.append(x)
        reads.append(x)
        at += len(x)
    bases = np.concatenate(chunks)
    offsets, lengths = np.array(offsets, np.int64), np.array([len(x) for x in reads], np.int32)
    # a row given twice, and a row that lies inside another read (it begins in the middle of a run or not, as it comes)
    big = int(np.argmax(lengths))
    offsets = np.concatenate([offsets, [offsets[big], offsets[big] + T - 3]])
    lengths = np.concatenate([lengths, [lengths[big], T + 9]]).astype(np.int32)
    order = rng.permutation(len(offsets))
    assert {int(o) % 16 for o in offsets} == set(range(16))
    return api.FastaData(bases, offsets[order], lengths[order], np.arange(1, len(order) + 1, dtype=np.int64))


def scan_table(T, B, seed=6):
    """2 B + 1 tiles: short reads of one tile each, three reads of three tiles, and across each multiple of B a stretch of one-base
    reads with empty reads between them."""
    rng = np.random.default_rng(seed)
    seqs, tiles = [], 0
    while tiles < 2 * B + 1:
        near = min(abs(tiles - B), abs(tiles - 2 * B)) <= 4
        if near:
            seqs += [np.zeros(0, np.uint8), runs_of(rng, 1, ACGT), np.zeros(0, np.uint8)]
            tiles += 1
        elif tiles in (7, 300, B + 900) and 2 * B + 1 - tiles >= 3:
            seqs.append(runs_of(rng, 2 * T + 5, ACGT))
            tiles += 3
        else:
            seqs.append(runs_of(rng, int(rng.integers(1, 41)), ACGT))
            tiles += 1
    assert tiles == 2 * B + 1
    return table(seqs)


def group_table(T, seed=7):
    """Reads for groups of at most 3 T bases: group ends exactly on the cap, a read of exactly the cap, one longer than it, empty reads
    at the seams."""
    rng = np.random.default_rng(seed)
    lengths = [T, 2 * T, 3 * T, 0, 3 * T + 1, 1, 0, 0, 3 * T - 1, T + 5, T, T, 0, 17, 5 * T + 3, 0, 2 * T, T - 1, 1, 1]
    return table([runs_of(rng, L, ACGT) for L in lengths])
