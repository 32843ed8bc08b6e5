#!/usr/bin/env python
"""Cost of read trimming next to the realignment it follows: the records of one C2-shaped search are realigned once, then piled up
(the adds), turned into clear ranges (the finish) and rewritten (the apply) by api.TrimSession, several times; the times, the counts
and the finish's bytes per second against the HBM figures of an MI355X are printed.

    python tools/trim_bench.py [--reads 100000] [--length 10000] [--repeats 5] [--adds 8] > profiles/trim_bench.txt

Times are host clocks.  An add does not wait for the device, so the adds are timed twice: as the calls return, and up to a stream
synchronise behind the last of them.  The finish ends in a synchronise of its own; it is one memset of 56 bytes, the run kernel and a
download of 64 bytes, so its time is the run kernel's plus a launch and a wait, and the rate printed is a lower bound of the kernel's.
The bytes are what the kernel must read and write: 4 per slot of the difference array, 12 per read in, 17 per read out.  The apply
uploads 32 bytes per record, downloads 32 and copies 64 on the host: it is timed whole.  A run without a GPU fails: there is no
fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api, workloads as W  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12     # bytes per second: the data sheet, and a float4 copy on the chip


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
        sys.exit("trim_bench: no GPU")
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
        t_call, t_add, t_finish, t_apply = [], [], [], []
        for rep in range(max(3, a.repeats) + 1):
            with mhap_amd.TrimSession(fasta.ids, fasta.lengths, handle=ms) as ts:
                ms.synchronize()
                t0 = time.perf_counter()
                for p in parts:
                    ts.add(p)
                t1 = time.perf_counter()
                ms.synchronize()
                t2 = time.perf_counter()
                counts = ts.finish()
                t3 = time.perf_counter()
                _, keep = ts.apply(kept)
                t4 = time.perf_counter()
            if rep:          # the first pass is the warm-up: first hipMalloc of every buffer
                t_call.append(t1 - t0)
                t_add.append(t2 - t0)
                t_finish.append(t3 - t2)
                t_apply.append(t4 - t3)
        slots = int(((fasta.lengths.astype(np.int64) + 4) & ~3).sum())
        nbytes = 4 * slots + 29 * len(fasta)
        fin = sorted(t_finish)[len(t_finish) // 2]
        print(f"{len(parts)} adds, as the calls return:      {spread(t_call)}")
        print(f"{len(parts)} adds, to the end of their kernels: {spread(t_add)}")
        print(f"finish (run kernel, counts down):        {spread(t_finish)}")
        print(f"apply (upload, kernel, download, copy):  {spread(t_apply)}; {int(keep.sum())} of {len(kept)} records kept")
        print(f"finish: {nbytes / 1e6:.1f} MB in {fin * 1e3:.2f} ms = {nbytes / fin / 1e12:.2f} TB/s, {100 * nbytes / fin / HBM_MEASURED:.0f} % of the "
              f"{HBM_MEASURED / 1e12:.2f} TB/s a copy reaches, {100 * nbytes / fin / HBM_SPEC:.0f} % of the {HBM_SPEC / 1e12:.1f} TB/s data sheet")
        print(api.trim_counts_line([counts[k] for k in api.TRIM_COUNTS]))
        print(f"{4 * slots / 1e6:.1f} MB of difference array and {32 * max(len(p) for p in parts) / 1e6:.1f} MB of records on the device")


if __name__ == "__main__":
    main()
