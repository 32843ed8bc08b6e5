#!/usr/bin/env python
"""Cost of cleaning the string graph (tips and simple bubbles, in rounds) next to the unitig build it repeats.

    python tools/clean_bench.py [--reads 20000,200000] [--keep 0.6] [--repeats 5]
    python tools/clean_bench.py --unitigs-only      # mhap_graph_unitigs alone: runs on a library without mhap_graph_clean too

The layout is tests/string_graph_ref.layout at scale: --reads reads of 3 000 - 9 000 positions on a line of 800 positions per read,
both strands, a record for every two reads that share at least 500 positions, its alignment short of the shared interval by 0 - 300
positions at either end, and the records thinned to --keep of them, so that transitive arcs stay, short branches dangle and unitigs
fall apart (no bases are needed).  One session per size: add, finish once, then mhap_graph_unitigs and mhap_graph_clean in turn,
each starting from the uncleaned graph.  Times are host clocks around calls that end in a synchronise, the first pass being the
warm-up.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
from mhap_amd.graph import counts_line  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}, n = {len(ts)})"


def thinned_layout(n, keep, seed):
    """(ids, lengths, records) of n reads placed on a line; the records of string_graph_ref.placed, made with numpy."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(3000, 9001, n)
    start = np.sort(rng.integers(0, max(800 * n - 9000, 1), n))
    end, strand = start + ln, rng.integers(0, 2, n)
    last = np.searchsorted(start, end - 500, side="right")           # read j > i shares >= 500 with i when start[j] <= end[i] - 500 ...
    cnt = np.maximum(last - np.arange(n) - 1, 0)
    i = np.repeat(np.arange(n), cnt)
    j = i + 1 + np.arange(len(i)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ok = np.minimum(end[i], end[j]) - start[j] >= 500                # ... and does not end inside that margin
    i, j = i[ok], j[ok]
    swap = rng.integers(0, 2, len(i)).astype(bool)
    x, y = np.where(swap, j, i), np.where(swap, i, j)
    lo = np.maximum(start[x], start[y]) + rng.integers(0, 301, len(x))
    hi = np.minimum(end[x], end[y]) - rng.integers(0, 301, len(x))
    ok = (hi - lo >= 1) & (rng.random(len(x)) < keep)
    x, y, lo, hi = x[ok], y[ok], lo[ok], hi[ok]
    recs = np.zeros(len(x), api.RECORD_DTYPE)
    recs["from_id"], recs["to_id"], recs["score"] = x + 1, y + 1, 0.9
    recs["alen"], recs["blen"], recs["to_rc"] = ln[x], ln[y], strand[x] != strand[y]
    for r, one, two in ((x, "a1", "a2"), (y, "b1", "b2")):
        fwd = strand[r] == 0
        recs[one] = np.where(fwd, lo - start[r], end[r] - hi)
        recs[two] = np.where(fwd, hi - start[r] - 1, end[r] - lo - 1)
    return np.arange(1, n + 1, dtype=np.int64), ln.astype(np.int32), recs


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def run(ms, n, keep, repeats, clean):
    ids, lengths, recs = thinned_layout(n, keep, n)
    gc, uc = np.zeros(len(api.GRAPH_COUNTS), np.int64), np.zeros(len(api.UNITIG_COUNTS), np.int64)
    cc = np.zeros(6, np.int64)
    t_unitigs, t_clean = [], []
    with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
        for part in np.array_split(recs, 8):
            gs.add(part)
        ms._chk(gs._lib.mhap_graph_finish(gs._s, api._ptr(gc)))
        for rep in range(max(3, repeats) + 1):
            tu = timed(lambda: ms._chk(gs._lib.mhap_graph_unitigs(gs._s, api._ptr(uc))))
            tc = timed(lambda: ms._chk(gs._lib.mhap_graph_clean(gs._s, None, api._ptr(cc)))) if clean else 0.0
            if rep:
                t_unitigs.append(tu)
                t_clean.append(tc)
        print(f"thinned layout: {n} reads, {len(recs)} records ({keep:.0%} kept)")
        print(counts_line(dict(zip(api.GRAPH_COUNTS, gc.tolist()))))
        print(api.unitig_counts_line(uc))
        print(f"mhap_graph_unitigs: {spread(t_unitigs)}")
        if clean:
            ms._chk(gs._lib.mhap_graph_unitigs_counts(gs._s, api._ptr(uc)))
            print(api.clean_counts_line(cc))
            print(api.unitig_counts_line(uc))
            print(f"mhap_graph_clean:   {spread(t_clean)}   ({int(cc[0])} rounds and the last build: {int(cc[0]) + 1} unitig builds)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", default="20000,200000", help="comma-separated table sizes")
    ap.add_argument("--keep", type=float, default=0.6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unitigs-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("clean_bench: no GPU")
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        for n in (int(x) for x in a.reads.split(",")):
            run(ms, n, a.keep, a.repeats, not a.unitigs_only)


if __name__ == "__main__":
    main()
