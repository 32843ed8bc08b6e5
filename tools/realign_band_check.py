#!/usr/bin/env python
"""Band adequacy of the realignment stage's automatic band, on the CPU restatements (tests/align_banded_ref.py, tests/align_ref.py):
the share of truly overlapping records whose banded score at the automatic band equals the full-matrix score.

    python tools/realign_band_check.py --search records.npy     # on a GPU: the self search of the end-to-end test's reads, saved
    python tools/realign_band_check.py --records records.npy    # anywhere: the comparison, over a process pool

The reads are those of tests/test_realign_gpu.py (120 x 2 000 bp, 15 % error, coverage 30, its seed); "truly overlapping" is that test's
rule (the two reads share at least 200 genome bases by the generator's truth)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mhap_amd  # noqa: E402

N_READS, READ_LEN, SEED = 120, 2000, 0x5EA1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--search")
    ap.add_argument("--records")
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    fasta = mhap_amd.synth_reads(N_READS, READ_LEN, seed=SEED, coverage=30.0, error_rate=0.15)
    if a.search:
        with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
            ms.add_data(fasta)
            recs = ms.find_matches()
        np.save(a.search, recs[np.lexsort((recs["to_rc"], recs["to_id"], recs["from_id"]))])
        print(f"{len(recs)} records saved to {a.search}")
        return
    import align_banded_ref as bref
    import align_ref
    recs = np.load(a.records)
    truth, G = mhap_amd.synth_truth(N_READS, READ_LEN, seed=SEED, coverage=30.0, error_rate=0.15)
    row = {int(i): k for k, i in enumerate(fasta.ids.tolist())}

    def shared(x, y):
        s1, e1 = int(truth["start"][x]), int(truth["start"][x] + truth["span"][x])
        s2, e2 = int(truth["start"][y]), int(truth["start"][y] + truth["span"][y])
        return sum(max(0, min(e1, e2 + k) - max(s1, s2 + k)) for k in (-G, 0, G))

    true = np.array([shared(row[int(r["from_id"])], row[int(r["to_id"])]) >= 200 for r in recs])
    recs = recs[true]
    pairs = bref.plan(recs, fasta.ids, fasta.offsets, fasta.lengths, 0.2, 0)
    banded = bref.align_pairs_banded(fasta.bases, pairs, workers=a.workers)
    full = align_ref.align_pairs(fasta.bases, pairs[:, :5], workers=a.workers)
    same = banded[:, 0] == full[:, 0]
    print(f"{len(recs)} truly overlapping records (of {len(true)}); automatic band: mean {pairs[:, 6].mean():.0f}, min {pairs[:, 6].min()}, "
          f"max {pairs[:, 6].max()}")
    print(f"banded score == full-matrix score: {int(same.sum())} of {len(recs)} ({same.mean():.1%}); "
          f"all seven fields equal: {int((banded == full).all(axis=1).sum())}")
    if not same.all():
        loss = (full[~same, 0] - banded[~same, 0]) / full[~same, 0]
        print(f"where they differ the band loses {loss.mean():.1%} of the score on average (worst {loss.max():.1%})")


if __name__ == "__main__":
    main()
