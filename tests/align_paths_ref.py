"""CPU restatement of the realignment stage's paths (include/mhap_hip.h, "the realignment stage's paths"): the banded aligner's matrix
with the three choices of every cell kept, and the path read back from the end cell.

The matrix is align_banded_ref.align_banded's, computed by anti-diagonals over the whole band, without the carried begin cell, column
and error counts: here they come out of the trace-back, which is what ties the two restatements together (tests/test_align_paths_cpu.py).
Per cell (i, j), 1-based, one uint8 of an (m + 1) x (n + 1) array: bits 0-1 H's choice (0 stop, 1 diagonal, 2 E, 3 F), bit 2 "E(i,j)
extends E(i,j-1)", bit 3 "F(i,j) extends F(i-1,j)".  Row 0, column 0 and every cell outside the band keep 0: a path stops there.

align_pairs_banded_paths has the signature and the result of mhap_amd.align_pairs_banded_paths; replay checks every invariant the
contract implies.
"""
import numpy as np

from align_ref import NEG, rc_bytes

NONE = (0, -1, -1, -1, -1, 0, 0)
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
MAXLEN = (1 << 28) - 1
LETTERS = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}


def encode(codes):
    """Codes of consecutive columns -> runs len << 4 | code; a run longer than 2^28 - 1 is split."""
    runs = []
    k = 0
    while k < len(codes):
        e = k
        while e < len(codes) and codes[e] == codes[k]:
            e += 1
        length = e - k
        while length > MAXLEN:
            runs.append(MAXLEN << 4 | codes[k])
            length -= MAXLEN
        runs.append(length << 4 | codes[k])
        k = e
    return runs


def align_path(s1, s2, diag, band):
    """((score, read_begin, read_end, ref_begin, ref_end, columns, errors), runs) of the local alignment of s1 against s2 in the band."""
    m, n = len(s1), len(s2)
    if m == 0 or n == 0 or band < 0:
        return NONE, []
    a = np.frombuffer(bytes(s1), np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(s2), np.uint8).astype(np.int64)
    bits = np.zeros((m + 1, n + 1), np.uint8)

    def blank():
        return np.zeros(m + 1, np.int64), np.full(m + 1, NEG, np.int64), np.full(m + 1, NEG, np.int64)

    (H2, _, _), (H1, E1, F1) = blank(), blank()
    best = (0, 0, 0)
    for d in range(2, m + n + 1):          # 1-based cells (i, j), i + j = d
        lo, hi = max(1, d - n), min(m, d - 1)
        lo = max(lo, -((band + diag - d) // 2))
        hi = min(hi, (d - diag + band) // 2)
        H0, E0, F0 = blank()
        if lo <= hi:
            i = np.arange(lo, hi + 1)
            j = d - i
            mis = a[i - 1] != b[j - 1]
            eext, eopn = E1[i] - 1, H1[i] - 2
            ext = eext >= eopn
            E = np.where(ext, eext, eopn)
            fext, fopn = F1[i - 1] - 1, H1[i - 1] - 2
            fx = fext >= fopn
            F = np.where(fx, fext, fopn)
            D = H2[i - 1] + np.where(mis, -2, 2)
            take_d = (D > 0) & (D >= E) & (D >= F)
            take_e = ~take_d & (E > 0) & (E >= F)
            take_f = ~take_d & ~take_e & (F > 0)
            H = np.where(take_d, D, np.where(take_e, E, np.where(take_f, F, 0)))
            H0[i], E0[i], F0[i] = H, E, F
            bits[i, j] = (np.where(take_d, 1, np.where(take_e, 2, np.where(take_f, 3, 0))) | (ext.astype(np.int64) << 2)
                          | (fx.astype(np.int64) << 3)).astype(np.uint8)
            hm = int(H.max())
            if hm > 0:
                k = int(np.nonzero(H == hm)[0][-1])     # on one anti-diagonal the largest i has the smallest j
                cand = (hm, int(j[k]) - 1, int(i[k]) - 1)
                if cand[0] > best[0] or (cand[0] == best[0] and (cand[1], cand[2]) < (best[1], best[2])):
                    best = cand
        H2, H1, E1, F1 = H1, H0, E0, F0
    if best[0] <= 0:
        return NONE, []
    score, ej, ei = best
    # the trace-back: from the end cell in state H
    i, j, state, codes = ei + 1, ej + 1, "H", []
    while True:
        c = int(bits[i, j])
        if state == "H":
            if c & 3 == 0:
                break
            if c & 3 == 1:
                codes.append(OP_EQ if a[i - 1] == b[j - 1] else OP_X)
                i, j = i - 1, j - 1
            else:
                state = "E" if c & 3 == 2 else "F"
        elif state == "E":
            codes.append(OP_D)
            state = "E" if c & 4 else "H"
            j -= 1
        else:
            codes.append(OP_I)
            state = "F" if c & 8 else "H"
            i -= 1
    codes.reverse()
    errors = sum(1 for c in codes if c != OP_EQ)
    return (score, i, ei, j, ej, len(codes), errors), encode(codes)


def replay(s1, s2, fields, runs):
    """Every invariant of the path contract for one pair: s2 as the aligner sees it (reverse-complemented already when b_rc)."""
    score, rb, re_, fb, fe, cols, errs = (int(x) for x in fields)
    runs = [int(r) for r in runs]
    if score <= 0:
        assert tuple(int(x) for x in fields) == NONE and runs == []
        return
    ops = [(r >> 4, r & 15) for r in runs]
    assert ops and all(length >= 1 and code in LETTERS for length, code in ops), ops
    for (l0, c0), (_, c1) in zip(ops, ops[1:]):
        assert c0 != c1 or l0 == MAXLEN, ops
    assert ops[0][1] == OP_EQ and ops[-1][1] == OP_EQ, ops

    def total(codes):
        return sum(length for length, code in ops if code in codes)

    assert total((OP_EQ, OP_X, OP_I)) == re_ - rb + 1
    assert total((OP_EQ, OP_X, OP_D)) == fe - fb + 1
    assert total((OP_EQ, OP_X, OP_I, OP_D)) == cols
    assert total((OP_X, OP_I, OP_D)) == errs
    i, j, got, prev = rb, fb, 0, None
    for length, code in ops:
        if code in (OP_EQ, OP_X):
            x, y = s1[i:i + length], s2[j:j + length]
            assert len(x) == length and len(y) == length
            same = [p == q for p, q in zip(x, y)]
            assert all(same) if code == OP_EQ else not any(same), (i, j, length, code)
            got += (2 if code == OP_EQ else -2) * length
            i, j = i + length, j + length
        else:
            got -= length + (0 if prev == code else 1)       # a gap of L columns costs 2 + (L - 1), split or not
            if code == OP_I:
                i += length
            else:
                j += length
        prev = code
    assert (i, j) == (re_ + 1, fe + 1) and got == score, (i, j, got, fields)


def _one(args):
    s1, s2, rc, diag, band = args
    return align_path(s1, rc_bytes(s2) if rc else s2, diag, band)


def align_pairs_banded_paths(bases, pairs7, workers=8):
    """The CPU counterpart of mhap_amd.align_pairs_banded_paths: (results, op_offsets, ops); big batches over `workers` processes."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs7 = np.asarray(pairs7, dtype=np.int64).reshape(-1, 7)
    raw = bases.tobytes()
    jobs = [(raw[ao:ao + al], raw[bo:bo + bl], rc, dg, bd) for ao, al, bo, bl, rc, dg, bd in pairs7.tolist()]
    cells = float(((pairs7[:, 1] + pairs7[:, 3]).astype(np.float64) * np.minimum(pairs7[:, 1], 2 * pairs7[:, 6] + 1)).sum()) if len(jobs) else 0.0
    if workers > 1 and len(jobs) > 1 and cells > 2e7:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
            res = pool.map(_one, jobs, chunksize=1)
    else:
        res = [_one(j) for j in jobs]
    out = np.zeros((len(jobs), 7), np.int32)
    offsets = np.zeros(len(jobs) + 1, np.int64)
    ops = []
    for q, (fields, runs) in enumerate(res):
        out[q] = fields
        ops += runs
        offsets[q + 1] = len(ops)
    return out, offsets, np.array(ops, np.uint32)
