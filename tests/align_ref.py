"""CPU restatement of the mhap_align_pairs contract (include/mhap_hip.h): SSW's scoring as EstimateROC calls it (+2 / -2, a gap of
length L costs 2 + (L - 1)) with this project's end-cell, predecessor and path-boundary rules.

Cells on one anti-diagonal i + j = d are independent, so each diagonal is one numpy step.  Every cell carries what the kernel carries
along its chosen predecessor: the begin cell, the column count and the error count of its path.  align_pairs(bases, pairs) has the
signature of mhap_amd.align_pairs, so it can be handed to mhap_amd.roc.estimate_roc(aligner=...).
"""
import numpy as np

NEG = -(1 << 28)
_RC = {ord(a): ord(b) for a, b in zip("ABCDGHKMNRSTVWY", "TVGHCDMKNYSABWR")}


def rc_bytes(b):
    """Utils.rc (J/utils/Utils.java:496-507): reversed, upper-cased, IUPAC complemented, any other byte unchanged."""
    out = bytearray()
    for c in reversed(bytes(b)):
        if ord("a") <= c <= ord("z"):
            c -= 32
        out.append(_RC.get(c, c))
    return bytes(out)


def align(s1, s2):
    """(score, read_begin, read_end, ref_begin, ref_end, columns, errors) of the local alignment of s1 against s2 (bytes)."""
    m, n = len(s1), len(s2)
    if m == 0 or n == 0:
        return (0, -1, -1, -1, -1, 0, 0)
    a = np.frombuffer(bytes(s1), np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(s2), np.uint8).astype(np.int64)

    def blank():   # one anti-diagonal indexed by row i = 0..m; entries off the diagonal's cells are the boundary (H 0, E/F -inf)
        return {"H": np.zeros(m + 1, np.int64), "E": np.full(m + 1, NEG, np.int64), "F": np.full(m + 1, NEG, np.int64),
                "mH": np.zeros((4, m + 1), np.int64), "mE": np.zeros((4, m + 1), np.int64), "mF": np.zeros((4, m + 1), np.int64)}

    p2, p1 = blank(), blank()
    best = (0, 0, 0, None)   # score, j, i (0-based end cell), carried (bi, bj, cols, errs)
    one_one = np.array([0, 0, 1, 1], np.int64)[:, None]
    for d in range(2, m + n + 1):          # 1-based cells (i, j), i + j = d
        lo, hi = max(1, d - n), min(m, d - 1)
        i = np.arange(lo, hi + 1)
        j = d - i
        mis = a[i - 1] != b[j - 1]
        cur = blank()
        # E(i,j) = max(H(i,j-1) - 2, E(i,j-1) - 1), extension on ties
        eext, eopn = p1["E"][i] - 1, p1["H"][i] - 2
        ext = eext >= eopn
        E = np.where(ext, eext, eopn)
        mE = np.where(ext, p1["mE"][:, i], p1["mH"][:, i]) + one_one
        # F(i,j) = max(H(i-1,j) - 2, F(i-1,j) - 1), extension on ties
        fext, fopn = p1["F"][i - 1] - 1, p1["H"][i - 1] - 2
        fx = fext >= fopn
        F = np.where(fx, fext, fopn)
        mF = np.where(fx, p1["mF"][:, i - 1], p1["mH"][:, i - 1]) + one_one
        # diagonal; out of an H = 0 cell it begins a path at (i - 1, j - 1) 0-based
        dH = p2["H"][i - 1]
        D = dH + np.where(mis, -2, 2)
        mD = p2["mH"][:, i - 1] + np.stack([np.zeros_like(i), np.zeros_like(i), np.ones_like(i), mis.astype(np.int64)])
        fresh = dH == 0
        mD = np.where(fresh, np.stack([i - 1, j - 1, np.ones_like(i), mis.astype(np.int64)]), mD)
        take_d = (D > 0) & (D >= E) & (D >= F)
        take_e = ~take_d & (E > 0) & (E >= F)
        take_f = ~take_d & ~take_e & (F > 0)
        H = np.where(take_d, D, np.where(take_e, E, np.where(take_f, F, 0)))
        mH = np.where(take_d, mD, np.where(take_e, mE, np.where(take_f, mF, 0)))
        cur["H"][i], cur["E"][i], cur["F"][i] = H, E, F
        cur["mH"][:, i], cur["mE"][:, i], cur["mF"][:, i] = mH, mE, mF
        hm = int(H.max())
        if hm > 0:
            k = int(np.nonzero(H == hm)[0][-1])     # on one diagonal the largest i has the smallest j
            cand = (hm, int(j[k]) - 1, int(i[k]) - 1)
            if cand[0] > best[0] or (cand[0] == best[0] and (cand[1], cand[2]) < (best[1], best[2])):
                best = (cand[0], cand[1], cand[2], tuple(int(x) for x in mH[:, k]))
        p2, p1 = p1, cur
    if best[0] <= 0:
        return (0, -1, -1, -1, -1, 0, 0)
    s, ej, ei, (bi, bj, cols, errs) = best
    return (s, bi, ei, bj, ej, cols, errs)


def _one(args):
    s1, s2, rc = args
    return align(s1, rc_bytes(s2) if rc else s2)


def align_pairs(bases, pairs, device=0, handle=None, workers=8):
    """The CPU counterpart of mhap_amd.align_pairs (same arguments and result layout); big batches over `workers` processes."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 5)
    out = np.zeros((len(pairs), 7), np.int32)
    raw = bases.tobytes()
    jobs = [(raw[ao:ao + al], raw[bo:bo + bl], rc) for ao, al, bo, bl, rc in pairs.tolist()]
    cells = float((pairs[:, 1].astype(np.float64) * pairs[:, 3]).sum()) if len(pairs) else 0.0
    if workers > 1 and len(jobs) > 1 and cells > 2e7:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
            res = pool.map(_one, jobs, chunksize=1)
    else:
        res = [_one(j) for j in jobs]
    for q, r in enumerate(res):
        out[q] = r
    return out
