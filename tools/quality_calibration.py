#!/usr/bin/env python
"""Calibration of the base qualities ("base qualities" of include/mhap_hip.h) against a truth genome.

    python tools/quality_calibration.py [--genome 20000] [--coverage 25] [--seed 7] [--min-cov 4]

The workload is tests/consensus_ref.py's quality_workload: reads of 600 - 999 bases at 12 % error drawn from a random genome, one
banded pair per two reads whose true placements share at least 200 bases.  The pairs are aligned with paths on the GPU, every record
votes (api.CorrectSession), and the quality pass runs twice: with per_vote = 10 and cap = 93, which makes the quality byte the net
vote m itself, and with the defaults.  Every corrected byte is marked right or wrong against the read's truth with
difflib.SequenceMatcher(autojunk=False) matching blocks.  Printed: per net vote the bytes, the wrong bytes, the empirical Phred
-10 log10(wrong / bytes) and the quality the defaults state; the same per stated quality; and the measured slope in tenths of a
Phred unit per net vote: least squares through the origin (the rule has no intercept) of the empirical Phred on m, weighted by
bytes, over the net votes below the cap's (m < 20) that have at least 10 wrong bytes, so that the Phred is resolved.  The truth
genome is the yardstick.  A run without a GPU fails: there is no fallback."""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mhap_amd  # noqa: E402
import consensus_ref as cref  # noqa: E402
import quality_ref as qref  # noqa: E402


def phred(wrong, n):
    return -10.0 * math.log10(wrong / n) if wrong else float("inf")


def table(title, keys, wrong, stated=None):
    print(title)
    print("| value | bytes | wrong | empirical Phred |" + (" stated by the defaults |" if stated else ""))
    print("|---|---|---|---|" + ("---|" if stated else ""))
    for k in sorted(set(keys.tolist())):
        sel = keys == k
        n, w = int(sel.sum()), int(wrong[sel].sum())
        e = f"{phred(w, n):.1f}" if w else f"> {phred(1, n):.1f}"
        print(f"| {k} | {n} | {w} | {e} |" + (f" {stated(k)} |" if stated else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--genome", type=int, default=20000)
    ap.add_argument("--coverage", type=float, default=25.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--min-cov", type=int, default=4)
    a = ap.parse_args()
    n_reads = int(round(a.coverage * a.genome / 800.0))                      # reads of 600 - 999 bases
    t0 = time.time()
    reads, truths, bases, pairs, meta = cref.quality_workload(a.seed, genome_len=a.genome, n_reads=n_reads)
    print(f"{a.genome} bases, {n_reads} reads ({len(bases)} bases), {len(pairs)} pairs; drawn in {time.time() - t0:.1f} s", flush=True)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    lengths = np.array([len(r) for r in reads], np.int32)
    fasta = mhap_amd.FastaData(bases, np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64), lengths, np.arange(1, len(reads) + 1))
    with mhap_amd.CorrectSession(fasta) as cs:
        cs.add(recs, offsets, ops)
        seqs, stats, skipped = cs.finish(a.min_cov)
        votes, _ = cs.quality(10, 93)                                         # the net vote itself (93 and more as 93)
        quals, hist = cs.quality()
    print(f"corrected: {int(stats[:, 1].sum())} bytes, {int(stats[:, 2].sum())} substitutions, {int(stats[:, 3].sum())} deletions, "
          f"{int(stats[:, 4].sum())} insertions, {int(stats[:, 5].sum())} low positions, skipped_views = {skipped}", flush=True)
    print(mhap_amd.api.quality_counts_line(hist), flush=True)
    t0, wrong = time.time(), []
    for r, (s, t) in enumerate(zip(seqs, truths)):
        wrong.append(qref.wrong_bytes(s, t))
        if r % 100 == 99:
            print(f"marked {r + 1} reads in {time.time() - t0:.0f} s", flush=True)
    wrong = np.concatenate(wrong)
    m, q = np.concatenate(votes).astype(np.int64), np.concatenate(quals).astype(np.int64)
    print(f"{len(wrong)} bytes, {int(wrong.sum())} wrong ({phred(int(wrong.sum()), len(wrong)):.1f})")
    p = mhap_amd.api.QualityParams()
    table("per net vote m:", m, wrong, stated=lambda k: min(p.cap, p.per_vote * k // 10))
    table("per stated quality (the defaults):", q, wrong)
    med, lo, hi = qref.ranking(quals, [wrong])
    print(f"median quality {med}: below it {lo[0]} wrong of {lo[1]}, at or above {hi[0]} wrong of {hi[1]}")
    num = den = 0.0
    used = []
    for k in range(1, 20):
        sel = m == k
        n, w = int(sel.sum()), int(wrong[sel].sum())
        if w >= 10:
            num += n * k * phred(w, n)
            den += n * k * k
            used.append(k)
    if den:
        slope = 10.0 * num / den
        print(f"measured slope over m in {used}: {slope:.1f} tenths of a Phred unit per net vote; to the nearest 5: {int(5 * round(slope / 5))}")
    else:
        print("no net vote below 20 has 10 wrong bytes: no slope")


if __name__ == "__main__":
    main()
