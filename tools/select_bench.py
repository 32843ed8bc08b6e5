#!/usr/bin/env python
"""Cost of overlap selection next to the repeat marking on the same records: the synthetic records of tools/repeat_bench.py over a
tiling of reads, and one read given many entries of its own, go through api.SelectSession — the adds (one lane per record: two entries
and their counts), the finish (prefix sum, scatter into segments, rows, radix select of the reads above best_n) and the apply — several
times, and a RepeatSession finishes on the same records in the same process.

    python tools/select_bench.py [--reads 100000] [--length 10000] [--depth 20] [--hot 100000] [--best 40] [--repeats 5] [--adds 8] > profiles/select_bench.txt

Times are host clocks.  An add does not wait for the device, so the adds are timed up to a stream synchronise behind the last of
them.  Either finish ends in one synchronise of its own.  The selection never touches a per-base array: its finish moves 8 bytes per
entry into the segments and reads 4 bytes per entry per pass of the select, where the repeat finish walks 4 bytes per base two to
three times, so a small fraction of the repeat finish is the expectation this tool tests; it is no threshold.  A run without a GPU
fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
from repeat_bench import spread, synthetic  # noqa: E402


def hot_read(n, length, entries, seed=6):
    """`entries` records between read 1 and the other reads, spans of 500 .. length on read 1 and the whole of the other read: one
    segment far above the LDS budget, with many equal keys."""
    rng = np.random.default_rng(seed)
    r = np.zeros(entries, api.RECORD_DTYPE)
    span = rng.integers(500, length + 1, entries)
    r["from_id"], r["to_id"] = 1, 2 + rng.integers(0, max(n - 1, 1), entries)
    r["a1"] = rng.integers(0, length - span + 1)
    r["a2"] = r["a1"] + span - 1
    r["b1"], r["b2"] = 0, length - 1
    r["alen"] = r["blen"] = length
    r["score"], r["raw"] = 1.0 - rng.integers(0, 3000, entries) / 10000.0, 50.0
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--hot", type=int, default=100000, help="entries given to read 1")
    ap.add_argument("--best", type=int, default=40, help="best_n")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adds", type=int, default=8, help="calls the records are split over")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("select_bench: no GPU")
    ids, lengths, records = synthetic(a.reads, a.length, a.depth)
    tiled = len(records)
    records = np.concatenate([records, hot_read(a.reads, a.length, a.hot)]) if a.hot > 0 and a.reads > 1 else records
    records = records[np.random.default_rng(7).permutation(len(records))]
    print(f"{len(ids)} reads x {a.length} bp, {tiled} synthetic records and {len(records) - tiled} more on read 1; best_n {a.best}")
    parts = np.array_split(records, max(1, a.adds))
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        t_add, t_finish, t_apply, t_repeat = [], [], [], []
        for rep in range(max(3, a.repeats) + 1):
            with api.SelectSession(ids, lengths, best_n=a.best, handle=ms) as ss:
                ms.synchronize()
                t0 = time.perf_counter()
                for p in parts:
                    ss.add(p)
                ms.synchronize()
                t1 = time.perf_counter()
                rows, counts = ss.finish()
                t2 = time.perf_counter()
                views = ss.apply(records)
                t3 = time.perf_counter()
            with api.RepeatSession(ids, lengths, handle=ms) as rs:
                for p in parts:
                    rs.add(p)
                ms.synchronize()
                t4 = time.perf_counter()
                rcounts = rs.finish()
                t5 = time.perf_counter()
            if rep:          # the first pass is the warm-up: first hipMalloc of every buffer
                t_add.append(t1 - t0)
                t_finish.append(t2 - t1)
                t_apply.append(t3 - t2)
                t_repeat.append(t5 - t4)
        fin, rfin = sorted(t_finish)[len(t_finish) // 2], sorted(t_repeat)[len(t_repeat) // 2]
        print(f"{len(parts)} adds, to the end of their kernels:            {spread(t_add)}")
        print(f"select finish (scan, scatter, rows, select, copy):  {spread(t_finish)}")
        print(f"apply (upload, kernel, download):                   {spread(t_apply)}; {int((views != 0).sum())} of {len(records)} records keep a view")
        print(f"repeat finish on the same records:                  {spread(t_repeat)}")
        print(f"select finish / repeat finish = {fin / rfin:.2f}")
        print(f"the longest segment: {int(rows[:, 0].max())} entries, {int(rows[rows[:, 0].argmax(), 1])} kept at threshold {int(rows[rows[:, 0].argmax(), 2])}")
        print(api.select_counts_line([counts[k] for k in api.SELECT_COUNTS]))
        print(api.repeat_counts_line([rcounts[k] for k in api.REPEAT_COUNTS]))
        print(f"{16 * len(records) / 1e6:.1f} MB of entries, {8 * len(records) / 1e6:.1f} MB of keys and {32 * max(len(p) for p in parts) / 1e6:.1f} MB of records on the device")


if __name__ == "__main__":
    main()
