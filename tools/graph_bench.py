#!/usr/bin/env python
"""Cost of the string graph next to the realignment it follows: the records of one C2-shaped search are realigned once, then classed
(the adds) and built and reduced (the finish) by api.GraphSession, several times; the times and the counts are printed.

    python tools/graph_bench.py [--reads 100000] [--length 10000] [--repeats 5] [--adds 8] > profiles/graph_bench.txt

Times are host clocks.  An add does not wait for the device, so the adds are timed twice: as the calls return, and up to a stream
synchronise behind the last of them; the finish ends in a synchronise of its own and includes the download of the arc table.  A run
without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import workloads as W  # noqa: E402
from mhap_amd.graph import counts_line  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=W.CONFIGS["c2"]["reads"])
    ap.add_argument("--length", type=int, default=W.CONFIGS["c2"]["length"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adds", type=int, default=8, help="calls the records are split over")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_bench: no GPU")
    fasta = W.config_reads("c2", reads=a.reads, length=a.length)
    with mhap_amd.MinHashSearch(W.params_for("c2")) as ms:
        ms.add_data(fasta)
        recs = ms.find_matches()
        t = time.perf_counter()
        out, _ = mhap_amd.realign_records(recs, fasta, handle=ms)
        t_realign = time.perf_counter() - t
        kept = out[kept_rows(out)]
        print(f"C2-shaped search: {len(fasta)} reads x {a.length} bp, {len(recs)} records, {len(kept)} realigned and kept ({t_realign * 1e3:.1f} ms)")
        parts = np.array_split(kept, max(1, a.adds))
        t_call, t_add, t_finish = [], [], []
        for rep in range(max(3, a.repeats) + 1):
            with mhap_amd.GraphSession(fasta.ids, fasta.lengths, handle=ms) as gs:
                ms.synchronize()
                t0 = time.perf_counter()
                for p in parts:
                    gs.add(p)
                t1 = time.perf_counter()
                ms.synchronize()
                t2 = time.perf_counter()
                arcs, counts = gs.finish()
                t3 = time.perf_counter()
            if rep:          # the first pass is the warm-up: first hipMalloc of every buffer
                t_call.append(t1 - t0)
                t_add.append(t2 - t0)
                t_finish.append(t3 - t2)
        print(f"{len(parts)} adds, as the calls return:      {spread(t_call)}")
        print(f"{len(parts)} adds, to the end of their kernels: {spread(t_add)}")
        print(f"finish (list, reduction, arc table down): {spread(t_finish)}")
        print(counts_line(counts))
        deg = np.bincount(arcs[:, 0], minlength=2 * len(fasta)) if len(arcs) else np.zeros(1, np.int64)
        print(f"out-degree before reduction: mean {deg.mean():.1f}, max {int(deg.max())}; {32 * len(kept) / 1e6:.1f} MB of records on the device")


if __name__ == "__main__":
    main()
