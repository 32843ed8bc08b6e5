#!/usr/bin/env python
"""Speed of the realignment stage: the banded aligner (mhap_align_pairs_banded) against the full-matrix one (mhap_align_pairs) on the
same whole-read pairs of a C2-shaped search, and the time to realign all of that search's records at the automatic band.

    python tools/realign_bench.py [--reads 100000] [--length 10000] [--pairs 2048] [--band 1250] [--repeats 5] > profiles/realign_bench.txt

Times are host clocks around calls that end in a stream synchronise (the calls return results on the host).  For the kernel comparison
the bases are compacted to the reads the chosen pairs name, so that both calls upload the same few tens of megabytes and not the whole
data set; the two aligners alternate inside every repeat, after one warm-up each.  Cell counts are computed here from the shapes.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import workloads as W  # noqa: E402


def band_cells(pairs7):
    """Cells of each pair that lie in its band and in its matrix."""
    out = np.zeros(len(pairs7), np.float64)
    for q, (_, m, _, n, _, diag, band) in enumerate(pairs7.tolist()):
        i = np.arange(m, dtype=np.int64)
        out[q] = np.maximum(0, np.minimum(n - 1, i + diag + band) - np.maximum(0, i + diag - band) + 1).sum()
    return out


def compact(fasta, pairs7):
    """The bases of the reads the pairs name, back to back, and the pairs with their offsets moved there."""
    offs = np.unique(np.concatenate([pairs7[:, 0], pairs7[:, 2]]))
    lens = {int(o): int(l) for o, l in zip(np.concatenate([pairs7[:, 0], pairs7[:, 2]]).tolist(), np.concatenate([pairs7[:, 1], pairs7[:, 3]]).tolist())}
    new, chunks, at = {}, [], 0
    for o in offs.tolist():
        new[o] = at
        chunks.append(fasta.bases[o:o + lens[o]])
        at += lens[o]
    p = pairs7.copy()
    p[:, 0] = [new[o] for o in pairs7[:, 0].tolist()]
    p[:, 2] = [new[o] for o in pairs7[:, 2].tolist()]
    return np.concatenate(chunks), p


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.1f} ms (min {ts[0] * 1e3:.1f}, max {ts[-1] * 1e3:.1f}, n = {len(ts)})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=W.CONFIGS["c2"]["reads"])
    ap.add_argument("--length", type=int, default=W.CONFIGS["c2"]["length"])
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--band", type=int, default=1250)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("realign_bench: no GPU")
    fasta = W.config_reads("c2", reads=a.reads, length=a.length)
    with mhap_amd.MinHashSearch(W.params_for("c2")) as ms:
        ms.add_data(fasta)
        t_search, recs = timed(ms.find_matches)
        t_search, recs = timed(ms.find_matches)          # (the second search is the warm one)
        recs = recs[np.lexsort((recs["to_rc"], recs["to_id"], recs["from_id"]))].copy()
        print(f"C2-shaped search: {len(fasta)} reads x {a.length} bp, {len(recs)} records, warm search {t_search * 1e3:.1f} ms")

        # 1. the two kernels on the same whole-read pairs
        sel = recs[np.linspace(0, len(recs) - 1, min(a.pairs, len(recs))).astype(np.int64)]
        bases, pairs7 = compact(fasta, mhap_amd.realign_plan(sel, fasta, band=a.band))
        pairs5 = np.ascontiguousarray(pairs7[:, :5])
        full_cells = float((pairs7[:, 1].astype(np.float64) * pairs7[:, 3]).sum())
        bcells = float(band_cells(pairs7).sum())
        full = mhap_amd.align_pairs(bases, pairs5, handle=ms)             # warm-up, and the results to compare
        banded = mhap_amd.align_pairs_banded(bases, pairs7, handle=ms)
        tf, tb = [], []
        for _ in range(a.repeats):
            tf.append(timed(lambda: mhap_amd.align_pairs(bases, pairs5, handle=ms))[0])
            tb.append(timed(lambda: mhap_amd.align_pairs_banded(bases, pairs7, handle=ms))[0])
        mf, mb = sorted(tf)[len(tf) // 2], sorted(tb)[len(tb) // 2]
        print(f"{len(pairs7)} whole-read pairs, {len(bases) / 1e6:.1f} MB of bases uploaded per call")
        print(f"  full matrix  (mhap_align_pairs):        {spread(tf)}; {full_cells:.3e} cells, {full_cells / mf / 1e9:.1f} G cell updates/s")
        print(f"  band = {a.band:<5d} (mhap_align_pairs_banded): {spread(tb)}; {bcells:.3e} cells ({bcells / full_cells:.1%} of the matrix), "
              f"{bcells / mb / 1e9:.1f} G cell updates/s")
        print(f"  banded / full time: {mb / mf:.3f}; pairs whose banded score equals the full-matrix score: "
              f"{int((banded[:, 0] == full[:, 0]).sum())} of {len(pairs7)}")

        # 2. all records at the automatic band, next to the search they follow
        one = [timed(lambda: mhap_amd.realign_records(recs[:1], fasta, handle=ms))[0] for _ in range(3)]
        out, detail = mhap_amd.realign_records(recs, fasta, handle=ms)    # warm-up
        ta = [timed(lambda: mhap_amd.realign_records(recs, fasta, handle=ms))[0] for _ in range(max(2, a.repeats // 2))]
        auto = mhap_amd.realign_plan(recs, fasta)
        acells = float(band_cells(auto).sum())
        ma = sorted(ta)[len(ta) // 2]
        print(f"realign all {len(recs)} records at the automatic band (mean band {auto[:, 6].mean():.0f}): {spread(ta)}; {acells:.3e} cells")
        print(f"  of which the upload of the {len(fasta.bases) / 1e9:.2f} GB of bases and one record: {spread(one)}")
        print(f"  {int((detail[:, 0] > 0).sum())} records aligned, {int((detail[:, 0] == 0).sum())} without an alignment; "
              f"mean aligned identity {float(out['score'][detail[:, 0] > 0].mean()):.4f}; warm search before it: {t_search * 1e3:.1f} ms")
        # 3. the same records with their paths (mhap_realign_records_paths), alternating with the call without them
        mhap_amd.realign_records_paths(recs, fasta, handle=ms)            # warm-up: the trace buffers' first hipMalloc
        tn, tp = [], []
        for _ in range(max(3, a.repeats)):
            tn.append(timed(lambda: mhap_amd.realign_records(recs, fasta, handle=ms))[0])
            t, (_, dp, op_offsets, ops) = timed(lambda: mhap_amd.realign_records_paths(recs, fasta, handle=ms))
            tp.append(t)
        mn, mp = sorted(tn)[len(tn) // 2], sorted(tp)[len(tp) // 2]
        res = mhap_amd.align_pairs_banded(fasta.bases, auto, handle=ms)
        ok = res[:, 0] > 0
        rows, cols2 = (res[ok, 2] - res[ok, 1] + 1).astype(np.int64), (res[ok, 4] - res[ok, 3] + 1).astype(np.int64)
        diags = np.minimum((res[ok, 5] - rows) + (res[ok, 5] - cols2) + 1, 2 * auto[ok, 6] + 1)
        trace = diags * ((rows + 7) // 8) * 4
        print(f"realign all {len(recs)} records without paths: {spread(tn)}")
        print(f"realign all {len(recs)} records with paths:    {spread(tp)}; with / without: {mp / mn:.3f}; {len(ops)} runs, "
              f"{len(ops) / max(1, int(ok.sum())):.0f} per aligned record")
        print(f"  trace: {trace.sum() / 1e9:.2f} GB over {int(ok.sum())} records, mean {trace.mean() / 1e6:.2f} MB, max {trace.max() / 1e6:.2f} MB "
              f"(mean {diags.mean():.0f} diagonals x {rows.mean():.0f} rows at 4 bits a cell); budget "
              f"{os.environ.get('MHAP_REALIGN_TRACE_BYTES', 'default (2 GiB)')}")
        if not mb < mf:
            print("realign_bench: the banded kernel is NOT faster than the full-matrix kernel", file=sys.stderr)
            sys.exit(3)


if __name__ == "__main__":
    main()
