#!/usr/bin/env python
"""Cost of repeat marking next to the trimming whose pile-up it shares: synthetic records over a tiling of reads (and a repeat family
planted among them) are piled up (the adds), marked (the finish: histogram, depth, count, prefix sum, fill) and judged (the apply) by
api.RepeatSession, several times, and a TrimSession finishes on the same records in the same process.

    python tools/repeat_bench.py [--reads 100000] [--length 10000] [--depth 20] [--repeats 5] [--adds 8] > profiles/repeat_bench.txt

Times are host clocks.  An add does not wait for the device, so the adds are timed up to a stream synchronise behind the last of
them.  Either finish ends in one synchronise of its own.  The repeat finish reads the difference array up to three times (histogram,
count, and the fill for the reads that have intervals) where the trimming's reads it once, so two to three times the trimming's
finish is the expectation this tool tests; it is no threshold.  The bytes quoted are 4 per slot of the difference array per pass.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12     # bytes per second: the data sheet, and a float4 copy on the chip


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}, n = {len(ts)})"


def synthetic(n, length, depth, family=200, seed=5):
    """Reads of one length tiling a line, `depth` deep: read i overlaps reads i + 1 .. i + depth - 1 exactly; and `family` reads spread
    over the table that also overlap each other in their middle fifth, a repeat about family / depth times as deep as the rest."""
    step = max(1, length // depth)
    i = np.repeat(np.arange(n, dtype=np.int64), depth - 1)
    k = np.tile(np.arange(1, depth, dtype=np.int64), n)
    ok = (i + k < n) & (length - k * step > 0)
    i, k = i[ok], k[ok]
    recs = np.zeros(len(i), api.RECORD_DTYPE)
    recs["from_id"], recs["to_id"] = i + 1, i + k + 1
    recs["a1"], recs["a2"], recs["b1"], recs["b2"] = k * step, length - 1, 0, length - 1 - k * step
    rng = np.random.default_rng(seed)
    fam = np.sort(rng.choice(n, min(family, n), replace=False))
    x, y = np.triu_indices(len(fam), 1)
    rep = np.zeros(len(x), api.RECORD_DTYPE)
    rep["from_id"], rep["to_id"] = fam[x] + 1, fam[y] + 1
    rep["a1"] = rep["b1"] = 2 * length // 5
    rep["a2"] = rep["b2"] = 3 * length // 5 - 1
    out = np.concatenate([recs, rep])
    out["alen"] = out["blen"] = length
    out["score"], out["raw"] = 0.9, 50.0
    return np.arange(1, n + 1, dtype=np.int64), np.full(n, length, np.int32), out[rng.permutation(len(out))]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adds", type=int, default=8, help="calls the records are split over")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("repeat_bench: no GPU")
    ids, lengths, records = synthetic(a.reads, a.length, a.depth)
    print(f"{len(ids)} reads x {a.length} bp, {len(records)} synthetic records")
    parts = np.array_split(records, max(1, a.adds))
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        t_add, t_finish, t_apply, t_trim = [], [], [], []
        for rep in range(max(3, a.repeats) + 1):
            with api.RepeatSession(ids, lengths, handle=ms) as rs:
                ms.synchronize()
                t0 = time.perf_counter()
                for p in parts:
                    rs.add(p)
                ms.synchronize()
                t1 = time.perf_counter()
                counts = rs.finish()
                t2 = time.perf_counter()
                keep, _ = rs.apply(records)
                t3 = time.perf_counter()
            with api.TrimSession(ids, lengths, handle=ms) as ts:
                for p in parts:
                    ts.add(p)
                ms.synchronize()
                t4 = time.perf_counter()
                tcounts = ts.finish()
                t5 = time.perf_counter()
            if rep:          # the first pass is the warm-up: first hipMalloc of every buffer
                t_add.append(t1 - t0)
                t_finish.append(t2 - t1)
                t_apply.append(t3 - t2)
                t_trim.append(t5 - t4)
        slots = int(((lengths.astype(np.int64) + 4) & ~3).sum())
        fin, tfin = sorted(t_finish)[len(t_finish) // 2], sorted(t_trim)[len(t_trim) // 2]
        print(f"{len(parts)} adds, to the end of their kernels:      {spread(t_add)}")
        print(f"repeat finish (histogram, depth, count, scan, fill): {spread(t_finish)}")
        print(f"apply (upload, kernel, download):             {spread(t_apply)}; {int(keep.sum())} of {len(records)} records kept")
        print(f"trim finish on the same records:              {spread(t_trim)}")
        marked = counts["reads_with_interval"] / max(1, counts["reads"])     # the fill walks the reads that have intervals only
        print(f"repeat finish / trim finish = {fin / tfin:.2f} ({2 + marked:.3f} passes over the difference array against one)")
        for name, t, passes in (("repeat finish", fin, 2 + marked), ("trim finish", tfin, 1)):
            nbytes = int(4 * slots * passes)
            print(f"{name}: {nbytes / 1e6:.1f} MB in {t * 1e3:.2f} ms = {nbytes / t / 1e12:.2f} TB/s, {100 * nbytes / t / HBM_MEASURED:.0f} % of the "
                  f"{HBM_MEASURED / 1e12:.2f} TB/s a copy reaches, {100 * nbytes / t / HBM_SPEC:.0f} % of the {HBM_SPEC / 1e12:.1f} TB/s data sheet")
        print(api.repeat_counts_line([counts[k] for k in api.REPEAT_COUNTS]))
        print(api.trim_counts_line([tcounts[k] for k in api.TRIM_COUNTS]))
        print(f"{4 * slots / 1e6:.1f} MB of difference array and {32 * max(len(p) for p in parts) / 1e6:.1f} MB of records on the device")


if __name__ == "__main__":
    main()
