"""The table behind the default (q_lo, q_hi) of the quality-weighted votes (EXPERIMENTS.md, "Quality-weighted votes"): wrong corrected
bytes on the CPU restatement, unweighted and under every candidate pair, per seed of tests/weighted_vote_ref.py's weighted workload.
No GPU: paths from tests/align_paths_ref.py, min_cov 4, wrong bytes as tests/quality_ref.py counts them.

    python tools/weight_thresholds.py [--seeds 101 102 103 104 105]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import align_paths_ref as apr  # noqa: E402
import consensus_ref as cref  # noqa: E402
import quality_ref as qref  # noqa: E402
import weighted_vote_ref as wref  # noqa: E402


def wrong_counts(seed, pairs_of_thresholds, min_cov=4):
    """(wrong bytes unweighted, [wrong bytes per (q_lo, q_hi)], raw wrong bytes) on one seed, the same reads and paths for all."""
    reads, quals, truths, bases, pairs, meta = wref.weighted_workload(seed)
    results, offsets, ops = apr.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    ids = range(1, len(reads) + 1)
    ref = cref.Consensus(reads, ids)
    ref.add(recs, offsets, ops)
    plain = sum(int(qref.wrong_bytes(ref.call_read(r, min_cov)[0], truths[r]).sum()) for r in range(len(reads)))
    raw = sum(int(qref.wrong_bytes(reads[r], truths[r]).sum()) for r in range(len(reads)))
    out = []
    for q_lo, q_hi in pairs_of_thresholds:
        w = wref.WeightedConsensus(reads, quals, ids, q_lo, q_hi)
        w.add(recs, offsets, ops)
        out.append(sum(int(qref.wrong_bytes(w.call_read(r, min_cov)[0], truths[r]).sum()) for r in range(len(reads))))
    return plain, out, raw


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--seeds", type=int, nargs="+", default=[101, 102, 103, 104, 105])
    a = ap.parse_args(argv)
    print("seed raw unweighted " + " ".join(f"({lo},{hi})" for lo, hi in wref.CANDIDATES))
    total_plain, totals = 0, [0] * len(wref.CANDIDATES)
    for seed in a.seeds:
        plain, out, raw = wrong_counts(seed, wref.CANDIDATES)
        print(seed, raw, plain, *out, flush=True)
        total_plain += plain
        totals = [x + y for x, y in zip(totals, out)]
    print("sum", "-", total_plain, *totals)
    best = min(range(len(totals)), key=lambda k: (totals[k], k))
    print(f"fewest wrong bytes: {wref.CANDIDATES[best]}, {totals[best]} against {total_plain} unweighted "
          f"({100.0 * (total_plain - totals[best]) / total_plain:.1f} % fewer)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
