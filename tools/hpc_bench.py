#!/usr/bin/env python
"""Cost of the homopolymer compression: the reads of BASELINE configs[1] (1 Gbase) are compressed several times by hpc.compress, the
records of one search of the compressed reads are expanded, and `mhap-hip --hpc` is run beside the plain search of the same file; the
times, the counts and the two passes' bytes per second against the HBM figures of an MI355X are printed.

    python tools/hpc_bench.py [--reads 100000] [--length 10000] [--repeats 5] [--no-cli] > profiles/hpc_bench.txt

The compression's times are the library's own (mhap_hpc_times): the upload of the raw reads, the two passes with the scan between
them, and the kernel that sums the run counts up, each between HIP events on the handle's stream, and the whole call on the host's clock, which adds the
planning on the host, the allocations and the one wait in the middle.  The bytes are what the two passes must move: each reads every
raw base once (2 B per raw base), the second writes a byte and an int32 per compressed base (5 B); the tile table and the scan add
40 B per tile of 4 096 bases and are left out.  The run counts are made in the second pass and summed by a kernel of one lane per
tile, reported by itself.  The expansion uploads 24 bytes per record and downloads 32: it is timed whole, on the host's clock.  The driver runs are
wall clocks of the whole process, file reading and start-up included.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api, hpc, workloads as W  # noqa: E402

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12     # bytes per second: the data sheet, and a float4 copy on the chip
LOAD_X4 = 10 * 256 * 2.4e9                   # streaming 16-byte loads: about 10 B per cycle and CU, 256 CUs at 2.4 GHz
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mhap_amd", "lib", "mhap-hip")


def spread(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.2f} ms (min {ms[0]:.2f}, max {ms[-1]:.2f}, n = {len(ms)})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=W.CONFIGS["c2"]["reads"])
    ap.add_argument("--length", type=int, default=W.CONFIGS["c2"]["length"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true", help="leave out the two runs of the driver")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hpc_bench: no GPU")
    fasta = W.config_reads("c2", reads=a.reads, length=a.length)
    times = {k: [] for k in ("upload", "passes", "counts", "call")}
    with mhap_amd.MinHashSearch(W.params_for("c2")) as ms:
        for rep in range(max(3, a.repeats) + 1):
            with hpc.compress(fasta, handle=ms) as hp:
                if rep:      # the first pass is the warm-up: first hipMalloc of every buffer
                    for k, v in hp.times().items():
                        times[k].append(v)
                counts = hp.counts
        raw, comp = counts["raw_bases"], counts["compressed_bases"]
        print(f"{len(fasta)} reads x {a.length} bp: " + api.hpc_counts_line([counts[k] for k in api.HPC_COUNTS]))
        for k, what in (("upload", "upload of the raw reads and tables"), ("passes", "count, scan, reads' rows, write"), ("counts", "run counts summed over the tiles"),
                        ("call", "whole call, host clock")):
            print(f"{what + ':':40s}{spread(times[k])}")
        nbytes = 2 * raw + 5 * comp
        t = sorted(times["passes"])[len(times["passes"]) // 2] * 1e-3
        print(f"two passes: {nbytes / 1e6:.1f} MB in {t * 1e3:.2f} ms = {nbytes / t / 1e12:.2f} TB/s: {100 * nbytes / t / LOAD_X4:.0f} % of the {LOAD_X4 / 1e12:.1f} TB/s of "
              f"streaming 16-byte loads, {100 * nbytes / t / HBM_MEASURED:.0f} % of the {HBM_MEASURED / 1e12:.2f} TB/s a copy reaches, "
              f"{100 * nbytes / t / HBM_SPEC:.0f} % of the {HBM_SPEC / 1e12:.1f} TB/s data sheet")
        with hpc.compress(fasta, handle=ms) as hp:
            t0 = time.perf_counter()
            ms.add_data(hp.fasta)
            recs = ms.find_matches()
            t_search = time.perf_counter() - t0
            t_expand = []
            for rep in range(max(3, a.repeats) + 1):
                t0 = time.perf_counter()
                out = hp.expand(recs)
                if rep:
                    t_expand.append((time.perf_counter() - t0) * 1e3)
            print(f"search of the compressed reads: {len(recs)} records in {t_search * 1e3:.1f} ms (sketch, index, search; host clock)")
            print(f"{'expansion of ' + str(len(out)) + ' records:':40s}{spread(t_expand)}")
    if a.no_cli:
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fasta")
        W.write_fasta(fasta, path)
        p = W.params_for("c2")
        flags = ["--num-hashes", str(p.num_hashes), "--ordered-sketch-size", str(p.ordered_sketch_size)]
        for name, extra in (("plain", []), ("--hpc", ["--hpc"])):
            t0 = time.perf_counter()
            r = subprocess.run([CLI, "-s", path] + flags + extra, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            dt = time.perf_counter() - t0
            if r.returncode != 0:
                sys.exit(f"hpc_bench: mhap-hip {name} failed ({r.returncode})")
            print(f"mhap-hip -s reads.fasta {name:6s}: {dt:.2f} s wall, {r.stdout.count(10)} overlaps printed")


if __name__ == "__main__":
    main()
