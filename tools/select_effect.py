#!/usr/bin/env python
"""What overlap selection does to read correction where a repeat family piles false overlaps up: a drawn circular genome with copies
of one repeat, reads at a few percent error (api.synth_reads_from_genome, the truth from api.synth_truth), the driver's overlaps,
and `mhap-hip --realign --correct` without and with `--best-overlaps`.  Every corrected read is compared with the stretch of the genome
it was drawn from (edit distance, banded), and the sums are given apart for the reads that touch a copy of the repeat and for those
that do not, next to the uncorrected reads' and to the driver's own timing lines.

    python tools/select_effect.py [--genome 90000] [--repeat 3000] [--copies 6] [--depth 25] [--error 0.05] [--best 40] [--min-span 500]

No ratio is expected of it; whatever comes out is the record (EXPERIMENTS.md, "Overlap selection").  A run without a GPU fails."""
import argparse
import multiprocessing
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def edit_distance(a, b, band):
    """Levenshtein distance of two byte strings inside a band round the main diagonal (exact when the distance is below the band)."""
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n, m = len(a), len(b)
    big = n + m + 1
    prev = np.arange(m + 1, dtype=np.int64)
    j = np.arange(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        lo, hi = max(1, i - band), min(m, i + band)
        cur = np.full(m + 1, big, np.int64)
        if lo == 1:
            cur[0] = i
        t = np.minimum(prev[lo - 1:hi] + (b[lo - 1:hi] != a[i - 1]), prev[lo:hi + 1] + 1)      # diagonal and up
        if lo == 1:
            t = np.concatenate([[i], t])
            cur[0:hi + 1] = np.minimum.accumulate(t - j[0:hi + 1]) + j[0:hi + 1]                   # and everything to the left
        else:
            cur[lo:hi + 1] = np.minimum.accumulate(t - j[lo:hi + 1]) + j[lo:hi + 1]
        prev = cur
    return int(prev[m])


def read_fasta(path):
    seqs = []
    with open(path, "rb") as fh:
        for line in fh:
            if not line.startswith(b">"):
                seqs.append(line.strip())
    return seqs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--genome", type=int, default=90000)
    ap.add_argument("--repeat", type=int, default=3000)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--depth", type=int, default=25)
    ap.add_argument("--error", type=float, default=0.05)
    ap.add_argument("--best", type=int, default=40)
    ap.add_argument("--min-span", type=int, default=500)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--workers", type=int, default=8, help="processes that compute the edit distances")
    a = ap.parse_args()
    pool = multiprocessing.Pool(a.workers)     # started before this process opens the GPU: the workers only compare byte strings
    import torch
    if not torch.cuda.is_available():
        sys.exit("select_effect: no GPU")
    rng = np.random.default_rng(a.seed)
    G = a.genome
    codes = rng.integers(0, 4, G).astype(np.uint8)
    starts = [G // a.copies * c + G // (3 * a.copies) for c in range(a.copies)]
    for c in starts[1:]:
        codes[c:c + a.repeat] = codes[starts[0]:starts[0] + a.repeat]
    lengths = rng.integers(4000, 6001, a.depth * G // 5000).astype(np.int32)
    fa = mhap_amd.synth_reads_from_genome(codes, lengths, seed=9, error_rate=a.error)
    truth, _ = api.synth_truth(len(lengths), lengths=lengths, genome_len=G, seed=9, error_rate=a.error)
    genome = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
    true_seq, touches = [], []
    for t in truth:
        s, n = int(t["start"]), int(t["span"])
        seq = (genome + genome)[s:s + n]
        true_seq.append(seq.translate(COMP)[::-1] if t["strand"] else seq)
        touches.append(any((c - s) % G < n or (s - c) % G < a.repeat for c in starts))
    touches = np.array(touches)
    print(f"{G}-base circular genome, {a.copies} copies of a {a.repeat}-base repeat, {len(lengths)} reads of 4000 - 6000 bases at {a.error:g} error "
          f"({a.depth} x); {int(touches.sum())} reads touch a copy, {int((~touches).sum())} do not")
    band = 400

    def sums(seqs):
        d = np.array(pool.starmap(edit_distance, [(s, t, band) for s, t in zip(seqs, true_seq)], chunksize=8), np.int64)
        return int(d[touches].sum()), int(d[~touches].sum())

    raw = [fa.sequence(i).encode() for i in range(len(fa))]
    print("uncorrected reads: edit distance to the truth, reads on a copy / others = %d / %d" % sums(raw))
    with tempfile.TemporaryDirectory() as tmp:
        fasta = os.path.join(tmp, "reads.fasta")
        with open(fasta, "w") as fh:
            for i in range(len(fa)):
                fh.write(f">read{i}\n{fa.sequence(i)}\n")
        for name, flags in (("all overlaps", []), (f"--best-overlaps {a.best} --best-min-span {a.min_span}",
                                                   ["--best-overlaps", str(a.best), "--best-min-span", str(a.min_span)])):
            out = os.path.join(tmp, "corrected.fasta")
            run = subprocess.run([CLI, "-s", fasta, "--realign", "--correct", out] + flags, capture_output=True, timeout=1200)
            if run.returncode != 0:
                sys.exit(run.stderr.decode()[-2000:])
            print("%s: edit distance to the truth, reads on a copy / others = %d / %d" % ((name,) + sums(read_fasta(out))))
            for line in run.stderr.decode().split("\n"):
                if line.startswith(("Time (s) to realign", "Time (s) to vote", "Time (s) to select", "Best overlaps:", "Corrected ")):
                    print("    " + line)
    pool.close()


if __name__ == "__main__":
    main()
