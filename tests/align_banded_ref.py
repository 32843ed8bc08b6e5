"""CPU restatement of the realignment stage (include/mhap_hip.h): the banded aligner's contract, the plan that turns an overlap record
into a banded pair, and the conversion of an alignment back into a record.

align_banded is align_ref.align with the band as a mask: a cell (i, j), 0-based, is computed iff |j - i - diag| <= band; every other
cell keeps the boundary values (H 0, E and F minus infinity, nothing carried).  align_pairs_banded has the signature of
mhap_amd.align_pairs_banded.
"""
import numpy as np

from align_ref import NEG, rc_bytes

NONE = (0, -1, -1, -1, -1, 0, 0)


def align_banded(s1, s2, diag, band):
    """(score, read_begin, read_end, ref_begin, ref_end, columns, errors) of the local alignment of s1 against s2 inside the band."""
    m, n = len(s1), len(s2)
    if m == 0 or n == 0 or band < 0:
        return NONE
    a = np.frombuffer(bytes(s1), np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(s2), np.uint8).astype(np.int64)

    def blank():
        return {"H": np.zeros(m + 1, np.int64), "E": np.full(m + 1, NEG, np.int64), "F": np.full(m + 1, NEG, np.int64),
                "mH": np.zeros((4, m + 1), np.int64), "mE": np.zeros((4, m + 1), np.int64), "mF": np.zeros((4, m + 1), np.int64)}

    p2, p1 = blank(), blank()
    best = (0, 0, 0, None)
    one_one = np.array([0, 0, 1, 1], np.int64)[:, None]
    for d in range(2, m + n + 1):          # 1-based cells (i, j), i + j = d; j - i is the same 0-based
        lo, hi = max(1, d - n), min(m, d - 1)
        # the band: -band <= d - 2 i - diag <= band
        lo = max(lo, -((band + diag - d) // 2))          # ceil((d - diag - band) / 2)
        hi = min(hi, (d - diag + band) // 2)
        cur = blank()
        if lo > hi:
            p2, p1 = p1, cur
            continue
        i = np.arange(lo, hi + 1)
        j = d - i
        assert (np.abs(j - i - diag) <= band).all()
        mis = a[i - 1] != b[j - 1]
        eext, eopn = p1["E"][i] - 1, p1["H"][i] - 2
        ext = eext >= eopn
        E = np.where(ext, eext, eopn)
        mE = np.where(ext, p1["mE"][:, i], p1["mH"][:, i]) + one_one
        fext, fopn = p1["F"][i - 1] - 1, p1["H"][i - 1] - 2
        fx = fext >= fopn
        F = np.where(fx, fext, fopn)
        mF = np.where(fx, p1["mF"][:, i - 1], p1["mH"][:, i - 1]) + one_one
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
        return NONE
    s, ej, ei, (bi, bj, cols, errs) = best
    return (s, bi, ei, bj, ej, cols, errs)


def _one(args):
    s1, s2, rc, diag, band = args
    return align_banded(s1, rc_bytes(s2) if rc else s2, diag, band)


def align_pairs_banded(bases, pairs7, device=0, handle=None, workers=8):
    """The CPU counterpart of mhap_amd.align_pairs_banded; big batches over `workers` processes."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs7 = np.asarray(pairs7, dtype=np.int64).reshape(-1, 7)
    out = np.zeros((len(pairs7), 7), np.int32)
    raw = bases.tobytes()
    jobs = [(raw[ao:ao + al], raw[bo:bo + bl], rc, dg, bd) for ao, al, bo, bl, rc, dg, bd in pairs7.tolist()]
    cells = float(((pairs7[:, 1] + pairs7[:, 3]).astype(np.float64) * np.minimum(pairs7[:, 1], 2 * pairs7[:, 6] + 1)).sum()) if len(jobs) else 0.0
    if workers > 1 and len(jobs) > 1 and cells > 2e7:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
            res = pool.map(_one, jobs, chunksize=1)
    else:
        res = [_one(j) for j in jobs]
    for q, r in enumerate(res):
        out[q] = r
    return out


def plan(records, ids, offsets, lengths, max_shift=0.2, band=0):
    """mhap_realign_plan: records (mhap_amd.api.RECORD_DTYPE rows) -> int64 (n, 7) banded pairs.  Raises ValueError where the
    library returns MHAP_E_INVALID."""
    where = {int(r): k for k, r in reversed(list(enumerate(np.asarray(ids).tolist())))}
    out = np.zeros((len(records), 7), np.int64)
    for q, r in enumerate(records):
        fa, fb = int(r["from_id"]), int(r["to_id"])
        if fa not in where or fb not in where:
            raise ValueError(f"record {q}: unknown read")
        ka, kb = where[fa], where[fb]
        alen, blen = int(r["alen"]), int(r["blen"])
        if int(lengths[ka]) != alen or int(lengths[kb]) != blen:
            raise ValueError(f"record {q}: wrong length")
        a1, a2, b1, b2 = int(r["a1"]), int(r["a2"]), int(r["b1"]), int(r["b2"])
        rc = int(r["to_rc"]) != 0
        if rc:
            b1, b2 = blen - b2 - 1, blen - b1 - 1
        diag = ((b1 + b2) - (a1 + a2)) // 2                       # Python's // floors toward minus infinity
        w = band if band > 0 else max(1, int(max(a2 - a1, b2 - b1) * max_shift))   # int() truncates toward zero, as Java's (int)
        out[q] = (int(offsets[ka]), alen, int(offsets[kb]), blen, 1 if rc else 0, diag, w)
    return out


def to_records(records, results):
    """mhap_realign_records' conversion: (realigned records, detail (n, 3))."""
    out = records.copy()
    out["pad"] = 0
    detail = np.zeros((len(records), 3), np.int32)
    for q, (r, a) in enumerate(zip(records, np.asarray(results).tolist())):
        score, rb, re_, fb, fe, cols, errs = a
        if score > 0 and cols > 0:
            blen, rc = int(r["blen"]), int(r["to_rc"]) != 0
            out[q]["a1"], out[q]["a2"] = rb, re_
            out[q]["b1"], out[q]["b2"] = (blen - fe - 1, blen - fb - 1) if rc else (fb, fe)
            out[q]["score"] = 1.0 - float(errs) / float(cols)
            detail[q] = (score, cols, errs)
        else:
            out[q]["a1"] = out[q]["a2"] = out[q]["b1"] = out[q]["b2"] = 0
            out[q]["score"] = 0.0
    return out, detail
