#!/usr/bin/env python
"""Cost of sequence assessment next to the counting it is built on: a random genome, reads cut from it with 1 % substitutions and
written as a FASTA file, the genome with 50 planted substitutions as the assembly, and at k = 16 (a) the set build from the open
count of the reads, (b) the evaluation of the reads file and of the assembly, one sequence, against the set, through the streamed
ingest, and (c) the comparison of two sets, each next to the time mhap_kmer_count_add_scan takes to count the same file in the same
process.

    python tools/kmer_qv_bench.py [--reads 100000] [--length 10000] [--genome 5000000] [--repeats 3] > profiles/kmer_qv_bench.txt

Times are host clocks around calls that end in a stream synchronise, so they hold the ingest's packing and uploads as well as the
kernels; MHAP_HOST_PROF=1 prints the ingest's own group times.  The evaluation does one bitmap lookup per window where the counting
makes two passes of one global atomic per window, so at most the counting's time is the expectation this tool tests; it is no
threshold.  A run without a GPU fails: there is no fallback."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402

K = 16


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}, n = {len(ts)})"


def median(ts):
    return sorted(ts)[len(ts) // 2]


def write_inputs(d, n, length, genome_len, seed=9, error=0.01, edits=50):
    """reads.fasta: n reads of `length` bases cut from a random genome, 1 % of their bases substituted, each read on its own;
    genome.fasta: the genome as one sequence with `edits` substitutions planted (the assembly that is assessed)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, genome_len)]
    hdr = 10                                               # ">r0000000\n", then the bases, then "\n": records of one size
    recs = np.empty((n, hdr + length + 1), np.uint8)
    starts = rng.integers(0, genome_len - length, n)
    for i in range(n):
        recs[i, :hdr] = np.frombuffer(b">r%07d\n" % i, np.uint8)
        recs[i, hdr:hdr + length] = genome[starts[i]:starts[i] + length]
    recs[:, -1] = ord("\n")
    ne = int(n * length * error)
    recs[rng.integers(0, n, ne), hdr + rng.integers(0, length, ne)] = acgt[rng.integers(0, 4, ne)]
    with open(os.path.join(d, "reads.fasta"), "wb") as f:
        f.write(recs)
    asm = genome.copy()
    at = rng.choice(genome_len, edits, replace=False)
    asm[at] = acgt[(np.searchsorted(acgt, asm[at]) + 1 + rng.integers(0, 3, edits)) % 4]
    with open(os.path.join(d, "genome.fasta"), "wb") as f:
        f.write(b">genome\n" + asm.tobytes() + b"\n")
    return os.path.join(d, "reads.fasta"), os.path.join(d, "genome.fasta")


def count(ms, scan):
    ms.synchronize()
    t0 = time.perf_counter()
    ms.kmer_count_begin(K, True)
    ms.kmer_count_add_scan(scan)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--genome", type=int, default=5000000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("kmer_qv_bench: no GPU")
    reps = max(3, a.repeats)
    with tempfile.TemporaryDirectory() as d, mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        t0 = time.perf_counter()
        reads_path, genome_path = write_inputs(d, a.reads, a.length, a.genome)
        print(f"{a.reads} reads x {a.length} bp of a {a.genome} bp genome, k = {K} (inputs written in {time.perf_counter() - t0:.1f} s)")
        with api.FastaScan(reads_path) as reads, api.FastaScan(genome_path) as genome:
            t_count_reads, t_count_genome, t_set, t_valley, t_eval_reads, t_eval_genome, t_compare = [], [], [], [], [], [], []
            solid = own = None
            for rep in range(reps + 1):
                for valley in (False, True):       # the set at a given threshold, and with the histogram finish and the valley in front
                    tc = count(ms, reads)
                    t1 = time.perf_counter()
                    s = ms.kmer_count_finish_set(0 if valley else 2)
                    t2 = time.perf_counter()
                    if rep:                        # the first pass is the warm-up: first hipMalloc of every buffer, the file's pages
                        t_count_reads.append(tc)
                        (t_valley if valley else t_set).append(t2 - t1)
                    if solid is not None:
                        solid.close()
                    solid = s
                tc = count(ms, genome)
                if own is not None:
                    own.close()
                own = ms.kmer_count_finish_set(1)
                t3 = time.perf_counter()
                er = ms.kmer_set_eval(solid, reads)
                t4 = time.perf_counter()
                eg = ms.kmer_set_eval(solid, genome)
                t5 = time.perf_counter()
                cmp3 = ms.kmer_set_compare(solid, own)
                t6 = time.perf_counter()
                if rep:
                    t_count_genome.append(tc)
                    t_eval_reads.append(t4 - t3)
                    t_eval_genome.append(t5 - t4)
                    t_compare.append(t6 - t5)
            wr, wg = int(er.totals[1]), int(eg.totals[1])
            print(f"count the reads file (begin, add_scan):        {spread(t_count_reads)}; {solid.total} windows")
            print(f"set build at a given min_count:                {spread(t_set)}")
            print(f"set build at the valley (histogram finish too): {spread(t_valley)}; min_count {solid.min_count}, {solid.members} of {solid.distinct} distinct")
            print(f"evaluate the reads file:                       {spread(t_eval_reads)}; {wr} windows, {wr / median(t_eval_reads) / 1e9:.2f} G windows/s; "
                  f"{median(t_eval_reads) / median(t_count_reads):.2f} of counting it")
            print(f"count the genome file:                         {spread(t_count_genome)}")
            print(f"evaluate the genome file (one sequence):       {spread(t_eval_genome)}; {wg} windows, {wg / median(t_eval_genome) / 1e9:.2f} G windows/s; "
                  f"{median(t_eval_genome) / median(t_count_genome):.2f} of counting it")
            nbytes = 2 * (4 ** K // 8)
            print(f"compare two sets:                              {spread(t_compare)}; {nbytes / 1e6:.0f} MB read, {nbytes / median(t_compare) / 1e12:.2f} TB/s")
            print(er.summary(solid, None))
            print(eg.summary(solid, own, cmp3[2]))
            solid.close()
            own.close()


if __name__ == "__main__":
    main()
