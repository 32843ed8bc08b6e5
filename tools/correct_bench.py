#!/usr/bin/env python
"""Cost of read correction next to the realignment it follows: the records of one C2-shaped search are realigned with paths alone, and
realigned with paths and then voted and called (api.CorrectSession), alternating; both times and the vote-table bytes are printed.

    python tools/correct_bench.py [--reads 100000] [--length 10000] [--repeats 5] [--min-coverage 4] > profiles/correct_bench.txt

Times are host clocks around calls that end in a stream synchronise.  The session's begin (the upload of the bases and the zeroing of
the table) is timed on its own; the vote is the add of all records' views, the call is finish with the download of the corrected bytes.
A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import workloads as W  # noqa: E402
from mhap_amd.correct import select_paths  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-coverage", type=int, default=4)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("correct_bench: no GPU")
    fasta = W.config_reads("c2", reads=a.reads, length=a.length)
    with mhap_amd.MinHashSearch(W.params_for("c2")) as ms:
        ms.add_data(fasta)
        recs = ms.find_matches()
        recs = recs[np.lexsort((recs["to_rc"], recs["to_id"], recs["from_id"]))].copy()
        print(f"C2-shaped search: {len(fasta)} reads x {a.length} bp, {len(fasta.bases)} bases, {len(recs)} records")

        def with_paths():
            out, _, off, ops = mhap_amd.realign_records_paths(recs, fasta, handle=ms)
            rows = kept_rows(out)
            return (out[rows],) + select_paths(off, ops, rows)

        def corrected():
            kept, off, ops = with_paths()
            t_begin, cs = timed(lambda: mhap_amd.CorrectSession(fasta, handle=ms))
            with cs:
                t_vote, _ = timed(lambda: cs.add(kept, off, ops))
                t_call, (seqs, stats, skipped) = timed(lambda: cs.finish(a.min_coverage))
                table = cs.table_bytes()
            return t_begin, t_vote, t_call, stats, skipped, table, len(kept), len(ops)

        with_paths()          # warm-up: the trace buffers' first hipMalloc
        corrected()
        tp, tc, parts = [], [], []
        for _ in range(max(3, a.repeats)):
            tp.append(timed(with_paths)[0])
            t, r = timed(corrected)
            tc.append(t)
            parts.append(r[:3])
        _, _, _, stats, skipped, table, n_kept, n_ops = r
        mp, mc = sorted(tp)[len(tp) // 2], sorted(tc)[len(tc) // 2]
        tot = stats.astype(np.int64).sum(axis=0).tolist()
        print(f"realign {len(recs)} records with paths:                    {spread(tp)}")
        print(f"realign with paths, then vote and call ({n_kept} records): {spread(tc)}; with / without: {mc / mp:.3f}")
        for name, k in (("begin (bases up, table zeroed)", 0), ("vote (add)", 1), ("call (finish + copy)", 2)):
            print(f"  of which {name}: {spread([p[k] for p in parts])}")
        print(f"  vote table: {table} bytes ({table / 1e9:.2f} GB, 48 per base); {n_ops} runs re-uploaded ({4 * n_ops / 1e6:.1f} MB); "
              f"{2 * n_kept} views, skipped_views = {skipped}")
        print(f"  {tot[0]} bases in, {tot[1]} out; {tot[2]} substitutions, {tot[3]} deletions, {tot[4]} insertions, {tot[5]} positions of low coverage")


if __name__ == "__main__":
    main()
