#!/usr/bin/env python
"""Wall time of the unitig consensus, stage by stage, next to the correction session on the same records.

    python tools/consensus_bench.py [--sets 20000:170,400000:3400] [--repeats 3]

Each set is genome:reads: reads of 2 500 - 3 500 bases at 10 % error drawn from a circular genome of that many bases
(synth_reads_from_genome), searched with the default parameters, realigned with paths, and laid out with max_hang 300, min_ovlp
1 000, fuzz 300 (the scaled flags of the driver tests; the first set is the input of the end-to-end test).  The consensus session
gets the kept records and runs --repeats times; its four stage times are mhap_consensus_times' (host clocks, each stage ending
behind a wait for the stream).  The correction session gets the same records with their runs: add is its vote, finish its call.
After each, the quality pass (ConsensusSession.quality, CorrectSession.quality: the kernel, the download of one byte per output
byte and of the histogram) is timed on its own, to be read next to `call` and `finish`.
--weigh makes both sessions weighted ones ("quality-weighted votes" in include/mhap_hip.h) over one Phred value drawn per base from
5, 14 and 30, with the default thresholds: the same records, the weighted vote, call and quality kernels.
The first repeat is the warm-up.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402


def run(G, n, seed, repeats, weigh=False):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, G).astype(np.uint8)
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, n).astype(np.int32), seed=9, error_rate=0.10)
    wkw = dict(qualities=np.random.default_rng(seed + 1).choice([5, 14, 30], len(fa.bases)).astype(np.uint8)) if weigh else {}
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
        ms.add_data(fa)
        out, _, op_off, ops = api.realign_records_paths(ms.find_matches(), fa, handle=ms)
        keep = kept_rows(out, 0.0)
        kept = out[keep]
        k_off = np.concatenate([[0], np.cumsum((op_off[1:] - op_off[:-1])[keep])]).astype(np.int64)
        k_ops = np.concatenate([ops[op_off[q]:op_off[q + 1]] for q in keep]) if len(keep) else np.zeros(0, np.uint32)
        for rep in range(repeats):
            with api.GraphSession(fa.ids, fa.lengths, handle=ms, max_hang=300, min_ovlp=1000, fuzz=300) as gs:
                gs.add(kept)
                gs.finish()
                u = gs.unitigs()
                with api.ConsensusSession(gs, fa, **wkw) as cs:
                    cs.add(kept)
                    t0 = time.time()
                    counts = cs.run()
                    wall = time.time() - t0
                    t = cs.times()
                    t0 = time.time()
                    cs.quality()
                    t_cq = time.time() - t0
            with api.CorrectSession(fa, handle=ms, **wkw) as cr:
                t0 = time.time()
                cr.add(kept, k_off, k_ops)
                t_add = time.time() - t0
                t0 = time.time()
                cr.finish()
                t_fin = time.time() - t0
                t0 = time.time()
                cr.quality()
                t_rq = time.time() - t0
            print(f"{'weighted, ' if weigh else ''}{G} bases, {len(fa)} reads ({int(fa.lengths.sum())} bases), {len(kept)} records, {u['counts']['unitigs']} unitigs of {u['counts']['total_bases']} bases, "
                  f"repeat {rep}: consensus run {wall * 1e3:.1f} ms = placement {t['placement'] * 1e3:.1f} + alignment {t['alignment'] * 1e3:.1f} + vote "
                  f"{t['vote'] * 1e3:.1f} + call {t['call'] * 1e3:.1f}; correction of the same records: add {t_add * 1e3:.1f} ms, finish {t_fin * 1e3:.1f} ms; "
                  f"quality pass: consensus {t_cq * 1e3:.1f} ms, correction {t_rq * 1e3:.1f} ms", flush=True)
        print(api.consensus_counts_line([counts[k] for k in api.CONSENSUS_COUNTS]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sets", default="20000:170,400000:3400", help="genome bases:reads, comma-separated")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--weigh", action="store_true", help="weighted sessions over drawn base qualities")
    a = ap.parse_args()
    for k, item in enumerate(a.sets.split(",")):
        G, n = (int(x) for x in item.split(":"))
        run(G, n, 41 + 2 * k, a.repeats, a.weigh)


if __name__ == "__main__":
    main()
