"""The variant filter's figures for EXPERIMENTS.md ("Variant filter"), on the planted diploid of tests/variant_cases.py; prints one JSON
line per row.
  python tools/variant_probe.py accuracy    # share of cross- and same-haplotype overlaps set aside at 0, 1 and 12 % read error
  python tools/variant_probe.py repeat      # a two-copy repeat, 1 % diverged, in a haploid genome: cross-copy overlaps through both filters
  python tools/variant_probe.py cost DIR    # mhap-hip --realign with and without --variant-filter on the planted reads and on c1's: stderr seconds
Truth comes from the layout: two reads of different haplotypes (copies) are a cross overlap.  The records are written from the layout
and realigned by the GPU aligner, as the truth gate of tests/test_variant_gpu.py does."""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import api, workloads  # noqa: E402
from mhap_amd.correct import select_paths  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402
import consensus_ref as cr  # noqa: E402
import variant_cases as vc  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")


def fasta_of(reads, ids):
    lengths = np.array([len(r) for r in reads], np.int32)
    return mhap_amd.FastaData(np.frombuffer(b"".join(reads), np.uint8), (np.cumsum(lengths, dtype=np.int64) - lengths).astype(np.int64), lengths, np.array(ids, np.int64))


def judged(ms, d, found, params):
    """(records kept by the realignment, their rows in `found`, keep, counts) of one session."""
    fa = fasta_of(d["reads"], d["ids"])
    out, _, op_offsets, ops = api.realign_records_paths(found, fa, handle=ms)
    rows = kept_rows(out)
    off, runs = select_paths(op_offsets, ops, rows)
    with api.VariantSession(fa, handle=ms, **params) as vs:
        vs.add(out[rows], off, runs)
        counts = vs.finish()
        keep, _ = vs.apply(out[rows], off, runs)
    return out[rows], rows, keep, counts


def accuracy(ms):
    for copies in (1, 3):
        for error in (0.0, 0.01, 0.12):
            d = vc.planted_diploid(error=error, copies=copies)
            found = vc.layout_records(d)
            hap = np.array([p[0] for p in d["place"]])
            for name, params in (("defaults", api.VARIANT_DEFAULTS), ("min_diff 4", dict(api.VARIANT_DEFAULTS, min_diff=4)),
                                 ("min_depth 4, min_minor 2", dict(api.VARIANT_DEFAULTS, min_depth=4, min_minor=2))):
                recs, rows, keep, counts = judged(ms, d, found, params)
                cross = hap[recs["from_id"] - 1] != hap[recs["to_id"] - 1]
                print(json.dumps(dict(reads=len(d["reads"]), error=error, params=name, realigned=len(recs), of=len(found), sites=counts["sites"], deep=counts["deep_positions"],
                                      bases=counts["bases"], cross=int(cross.sum()), cross_set_aside=int((cross & (keep == 0)).sum()), same=int((~cross).sum()),
                                      same_set_aside=int((~cross & (keep == 0)).sum()))), flush=True)


def repeat(ms):
    """A haploid genome of 20 kb whose stretch [3 000, 6 000) stands a second time at [12 000, 15 000), 1 % diverged; the true overlaps
    from the layout and, for every two reads that share 1 kb of the stretch from different copies, the false one."""
    first, second, length = 3000, 12000, 3000
    for copies, error in ((1, 0.0), (3, 0.0), (3, 0.01), (3, 0.12)):
        d = vc.planted_diploid(every=0, repeat=(first, second, length, 100), error=error, copies=copies)
        true = vc.layout_records(d)
        false = []
        place, reads = d["place"], d["reads"]
        for x in range(len(reads)):
            for y in range(len(reads)):
                (_, sa, ea, ta), (_, sb, eb, tb) = place[x], place[y]
                lo, hi = max(sa - first, sb - second, 0), min(ea - first, eb - second, length)   # the shared stretch in the copies' own coordinates
                if hi - lo < 1000:
                    continue

                def own(s, e, strand, n, g0):
                    b, f = (e - (g0 + hi), e - 1 - (g0 + lo)) if strand else (g0 + lo - s, g0 + hi - 1 - s)
                    return min(int(b * n / (e - s)), n - 1), min(int(f * n / (e - s)), n - 1)
                a1, a2 = own(sa, ea, ta, len(reads[x]), first)
                b1, b2 = own(sb, eb, tb, len(reads[y]), second)
                rec = np.zeros(1, cr.RECORD_DTYPE)
                rec[0] = (x + 1, y + 1, 0.9, 100.0, a1, a2, len(reads[x]), b1, b2, len(reads[y]), int(ta != tb), 0)
                false.append(rec)
        found = np.concatenate([true] + false)
        is_false = np.arange(len(found)) >= len(true)
        for name, params in (("defaults", api.VARIANT_DEFAULTS), ("min_depth 4, min_minor 2", dict(api.VARIANT_DEFAULTS, min_depth=4, min_minor=2))):
            recs, rows, keep, counts = judged(ms, d, found, params)
            fa = fasta_of(d["reads"], d["ids"])
            with api.RepeatSession(fa.ids, fa.lengths, handle=ms, **api.REPEAT_DEFAULTS) as rs:   # the repeat filter on the survivors
                rs.add(recs[keep != 0])
                rs.finish()
                rkeep, _ = rs.apply(recs[keep != 0])
            f = is_false[rows]
            fk = f[keep != 0]
            print(json.dumps(dict(reads=len(reads), error=error, params=name, true=int((~f).sum()), true_set_aside=int((~f & (keep == 0)).sum()), false=int(f.sum()),
                                  false_set_aside_by_variants=int((f & (keep == 0)).sum()), false_left_after_repeat_filter=int((fk & (rkeep != 0)).sum()),
                                  true_set_aside_by_repeat_filter=int((~fk & (rkeep == 0)).sum()), sites=counts["sites"])), flush=True)


def seconds(stderr, prefix):
    m = [re.search(r": ([0-9.e+-]+)", l) for l in stderr.split("\n") if l.startswith(prefix)]
    return float(m[0].group(1)) if m and m[0] else None


def cost(directory):
    os.makedirs(directory, exist_ok=True)
    d = vc.planted_diploid(copies=3)
    planted = os.path.join(directory, "planted.fasta")
    with open(planted, "w") as fh:
        for i, r in enumerate(d["reads"]):
            fh.write(f">read{i}\n{r.decode()}\n")
    c1 = os.path.join(directory, "c1.fasta")
    workloads.write_fasta(workloads.config_reads("c1"), c1)
    for name, fasta in (("planted diploid, 90 reads", planted), ("c1", c1)):
        for flags in ([], ["--variant-filter"]):
            for _ in range(2):   # the second run is the one to read: the first pays for the file cache and the code objects
                r = subprocess.run([CLI, "-s", fasta, "--realign"] + flags, capture_output=True, text=True, timeout=900, cwd=directory)
            assert r.returncode == 0, r.stderr[-2000:]
            line = [l for l in r.stderr.split("\n") if l.startswith(("Variant sites", "Time (s) to mark"))]
            print(json.dumps(dict(input=name, flags=flags, total=seconds(r.stderr, "Total time (s)"), realign=seconds(r.stderr, "Time (s) to realign"),
                                  variant=seconds(r.stderr, "Time (s) to mark variant sites and judge"), lines=line)), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "accuracy"
    if what == "cost":
        cost(sys.argv[2])
    else:
        with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
            (accuracy if what == "accuracy" else repeat)(ms)
