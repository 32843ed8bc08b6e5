#!/usr/bin/env python
"""Wall time of the streamed ingest of a FASTQ file next to its FASTA twin: mhap_fasta_scan_open plus mhap_index_add_scan.

    python tools/fastq_ingest_bench.py [--reads 25600] [--length 10000] [--repeats 3] [--dir /tmp]

Synthetic reads (synth_reads, 15 % error) are written once as FASTA (workloads.write_fasta) and once as single-line FASTQ with one
quality drawn per base; each file is scanned and added to a fresh index --repeats times (host clocks around calls that end in a
synchronise; the first repeat is the warm-up, the files are in the page cache from their writing on).  The FASTQ scan also reads the
quality lines, in its sequential record pass; the qualities are not uploaded.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api, workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=25600)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default="/tmp")
    a = ap.parse_args()
    fa = mhap_amd.synth_reads(a.reads, a.length, seed=7)
    twin, fastq = os.path.join(a.dir, "ingest_twin.fasta"), os.path.join(a.dir, "ingest_reads.fastq")
    workloads.write_fasta(fa, twin)
    rng = np.random.default_rng(3)
    with open(fastq, "wb") as fh:
        for i in range(len(fa)):
            o, n = int(fa.offsets[i]), int(fa.lengths[i])
            fh.write(b"@r" + str(int(fa.ids[i])).encode() + b"\n" + fa.bases[o:o + n].tobytes() + b"\n+\n")
            fh.write((rng.integers(0, 41, n).astype(np.uint8) + 33).tobytes() + b"\n")
    print(f"{len(fa)} reads, {int(fa.lengths.sum())} bases; {os.path.getsize(twin)} bytes of FASTA, {os.path.getsize(fastq)} of FASTQ", flush=True)
    for rep in range(a.repeats):
        for name, path in (("FASTA", twin), ("FASTQ", fastq)):
            with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
                t0 = time.time()
                with api.FastaScan(path) as scan:
                    t1 = time.time()
                    ms.add_scan(scan)
                    ms.synchronize()
                    t2 = time.time()
                    t_q = 0.0
                    if scan.has_qualities:
                        scan.qualities()
                        t_q = time.time() - t2
                print(f"repeat {rep}, {name}: scan_open {1e3 * (t1 - t0):.1f} ms, add_scan {1e3 * (t2 - t1):.1f} ms, together {1e3 * (t2 - t0):.1f} ms"
                      + (f"; copying the qualities out {1e3 * t_q:.1f} ms" if t_q else ""), flush=True)
    os.remove(twin)
    os.remove(fastq)


if __name__ == "__main__":
    main()
