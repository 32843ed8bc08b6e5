"""Hand-made inputs of the "read trimming" contract with their expected results written out, and the ideal-records experiment:
shared by tests/test_trim_cpu.py (against tests/trim_ref.py and the host entry points) and tests/test_trim_gpu.py (against the GPU)."""
import numpy as np

from mhap_amd import api


def rec(frm, to, a1, a2, alen, b1, b2, blen, to_rc=0, score=0.9, raw=50.0):
    r = np.zeros(1, api.RECORD_DTYPE)[0]
    for k, v in dict(from_id=frm, to_id=to, a1=a1, a2=a2, alen=alen, b1=b1, b2=b2, blen=blen, to_rc=to_rc, score=score, raw=raw).items():
        r[k] = v
    return r


def recs(rows):
    return np.array(rows, dtype=api.RECORD_DTYPE) if len(rows) else np.zeros(0, api.RECORD_DTYPE)


# ---- the worked example: three reads, four records, min_cov 2, end_clip 2, min_span 6 ----
HAND_P = dict(min_cov=2, end_clip=2, min_span=6, min_identity=0.0)
HAND_IDS = np.array([1, 2, 3], np.int64)
HAND_LEN = np.array([30, 30, 20], np.int32)


def hand_records(to_rc):
    return recs([rec(1, 2, 0, 19, 30, 10, 29, 30, to_rc),     # read 1 [2, 18)    read 2 [12, 28)
                 rec(1, 3, 4, 29, 30, 0, 19, 20, to_rc),      # read 1 [6, 28)    read 3 [2, 18)
                 rec(2, 1, 0, 9, 30, 10, 25, 30, to_rc),      # read 2 [2, 8)     read 1 [12, 24)
                 rec(3, 2, 0, 19, 20, 8, 29, 30, to_rc)])     # read 3 [2, 18)    read 2 [10, 28)


HAND_COV = [[0] * 2 + [1] * 4 + [2] * 6 + [3] * 6 + [2] * 6 + [1] * 4 + [0] * 2,
            [0] * 2 + [1] * 6 + [0] * 2 + [1] * 2 + [2] * 16 + [0] * 2,
            [0] * 2 + [2] * 16 + [0] * 2]
HAND_ROWS = [[4, 26, 1, 18], [10, 30, 1, 16], [0, 20, 1, 16]]
HAND_FLAGS = [api.TRIM_CUT5 | api.TRIM_CUT3, api.TRIM_CUT5, 0]
HAND_COUNTS = dict(reads=3, deleted=0, cut5=2, cut3=1, gapped=0, bases_in=80, bases_kept=62, eligible_records=4)
# record 0 onto the clear ranges of reads 1 and 2: {a1, a2, alen, b1, b2, blen}, for to_rc 0 and 1
HAND_KEEP = [1, 1, 0, 1]     # record 2 lies on [0, 10) of read 2, in front of its clear range: void
HAND_CLIPPED0 = {0: (0, 15, 22, 4, 19, 20), 1: (0, 15, 22, 0, 15, 20)}


# ---- the ideal-records experiment: a circular genome, reads with known places, two-piece chimeras, noisy interval ends ----
def ideal_experiment(seed, genome=20000, n_reads=170, n_chimeras=12, noise=30, min_overlap=200):
    """(ids, lengths, records, junctions): junctions {read index: j}.  Every pair of pieces of different reads whose places share
    at least min_overlap bases gives one forward record, its four ends moved by up to +-noise and kept inside the reads."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(2500, 3501, n_reads).astype(np.int32)
    starts = rng.integers(0, genome, n_reads)
    chim = np.sort(rng.choice(n_reads, n_chimeras, replace=False))
    pieces, junctions = [], {}     # (read, offset in the read, genome start, length)
    for r in range(n_reads):
        L = int(lengths[r])
        if r in chim:
            j = int(rng.integers(2 * L // 5, 3 * L // 5 + 1))
            s2 = (int(starts[r]) + j + int(rng.integers(4000, genome - 4000))) % genome     # another locus
            pieces += [(r, 0, int(starts[r]), j), (r, j, s2, L - j)]
            junctions[r] = j
        else:
            pieces.append((r, 0, int(starts[r]), L))
    out = []
    for x in range(len(pieces)):
        ra, oa, ga, la = pieces[x]
        for y in range(x + 1, len(pieces)):
            rb, ob, gb, lb = pieces[y]
            if ra == rb:
                continue
            d, d2 = (gb - ga) % genome, (ga - gb) % genome
            if d < la:
                n, sa, sb = min(la - d, lb), oa + d, ob
            elif d2 < lb:
                n, sa, sb = min(lb - d2, la), oa, ob + d2
            else:
                continue
            if n < min_overlap:
                continue
            e = rng.integers(-noise, noise + 1, 4)
            La, Lb = int(lengths[ra]), int(lengths[rb])
            a1, a2 = max(0, sa + int(e[0])), min(La - 1, sa + n - 1 + int(e[1]))
            b1, b2 = max(0, sb + int(e[2])), min(Lb - 1, sb + n - 1 + int(e[3]))
            out.append(rec(ra + 1, rb + 1, a1, a2, La, b1, b2, Lb, 0, 0.9))
    return np.arange(1, n_reads + 1, dtype=np.int64), lengths, recs(out), junctions


def crosses(row, j, end_clip):
    """A clear range crosses a junction when it extends more than end_clip past it on both sides."""
    return row[0] < j - end_clip and row[1] > j + end_clip


# ---- refinement: a path worked by hand, penalty 2 ----
OPS = {"=": 7, "X": 8, "I": 1, "D": 2}


def encode(runs):
    return np.array([n << 4 | OPS[c] for n, c in runs], np.uint32)


# a1 = 5, b1 = 7 (frame).  Sums: 4= -> 4; 3X -> -2; 10= starts again at A 12 / B 14 -> 10; 1I -> 8; 20= -> 28; 2D -> 24; 5= -> 29, the
# best, ending at A 47 / B 50; 8X -> 13; 4= -> 17.  The stretch has 38 columns and 3 errors.
REFINE_RUNS = [(4, "="), (3, "X"), (10, "="), (1, "I"), (20, "="), (2, "D"), (5, "="), (8, "X"), (4, "=")]
REFINE_WANT = {0: (12, 47, 14, 50), 1: (12, 47, 249, 285)}     # a1, a2, b1, b2 for to_rc 0 and 1: B [14, 51) in the frame, flipped in 300


def refine_record(to_rc):
    """The record of REFINE_RUNS: 55 bases of A from 5, 56 of B from 7 in the frame."""
    b1, b2 = (7, 62) if not to_rc else (300 - 62 - 1, 300 - 7 - 1)
    return rec(1, 2, 5, 59, 200, b1, b2, 300, to_rc)


def random_paths(rng, n):
    """n records with random paths: (records, op_offsets, ops)."""
    out, offs, ops = [], [0], []
    for _ in range(n):
        runs, prev = [], None
        for _ in range(int(rng.integers(0, 40))):
            c = str(rng.choice(["=", "X", "I", "D"], p=[.5, .2, .15, .15]))
            if c != prev:
                runs.append((int(rng.integers(1, 60)), c))
                prev = c
        na, nb = sum(k for k, c in runs if c in "=XI"), sum(k for k, c in runs if c in "=XD")
        if na == 0 or nb == 0:
            runs, na, nb = [], 1, 1
        a1, f1, o = int(rng.integers(0, 50)), int(rng.integers(0, 50)), int(rng.integers(0, 2))
        blen = f1 + nb + 13
        b1, b2 = (f1, f1 + nb - 1) if not o else (blen - f1 - nb, blen - f1 - 1)
        out.append(rec(1, 2, a1, a1 + na - 1, a1 + na + 9, b1, b2, blen, o, 0.8 if runs else 0.0))
        ops += encode(runs).tolist()
        offs.append(len(ops))
    return recs(out), np.array(offs, np.int64), np.array(ops, np.uint32)
