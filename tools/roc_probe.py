"""EstimateROC (mhap_amd.roc) with the GPU alignment check, measured on c2 and c5slice; prints one JSON line.
  python tools/roc_probe.py [--workdir DIR] [--configs c2,c5slice]
Steps per configuration, each a child process under its own `timeout` (the probe stops at the first that fails):
  prep     the configuration's reads and their truth (mhap_synth_truth -> truth.m4), the overlaps from MinHashSearch (c5slice: with the -f
           filter counted from the reads on the GPU), written as MHAP text
  sampled  estimate_roc, 10 000 trials, DP on: phase wall times, pairs aligned, cells, sensitivity / specificity / PPV
  full     the same in full mode (trials = 0); its alignment batch is saved for the next step
  nodp     full mode with DP off: what DP rescues and rejects
  align    the full-mode batch through align_pairs once, under `rocprofv3 --kernel-trace --stats`: device time and cell updates / s"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _paths(a):
    d = os.path.join(a.workdir, a.config)
    os.makedirs(d, exist_ok=True)
    return {k: os.path.join(d, f) for k, f in (("fasta", "reads.fasta"), ("ovl", "ovl.txt"), ("m4", "truth.m4"), ("batch", "full_batch.npz"))}


def step_prep(a):
    import mhap_amd
    from mhap_amd import workloads as W
    c = W.CONFIGS[a.config]
    p = _paths(a)
    t = time.time()
    fa = W.config_reads(a.config)
    truth, G = mhap_amd.synth_truth(c["reads"], c["length"], seed=c["seed"])
    wrapped = W.write_truth_m4(p["m4"], truth, G)
    W.write_fasta(fa, p["fasta"], prefix="")
    out = {"reads": len(fa), "genome": G, "wrapped_reads": wrapped, "gen_s": round(time.time() - t, 1)}
    flt = None
    if c["filter"]:
        flt = mhap_amd.FrequencyCounts.from_counts(mhap_amd.count_kmers(fa), filter_cutoff=1e-5, repeat_weight=0.9)
    t = time.time()
    with mhap_amd.MinHashSearch(W.params_for(a.config, device=0), kmer_filter=flt) as ms:
        ms.add_data(fa)
        recs = ms.find_matches()
    out["search_s"] = round(time.time() - t, 1)
    lines = mhap_amd.records_to_lines(recs)
    with open(p["ovl"], "w") as fh:
        fh.write("".join(x + "\n" for x in lines))
    out["records"] = len(lines)
    return out


def _roc(a, trials, dp, save=None):
    import mhap_amd
    from mhap_amd import roc
    p = _paths(a)
    batch = {}

    def aligner(bases, pairs):
        if save:
            np.savez(save, bases=bases, pairs=pairs)
        t = time.perf_counter()
        r = mhap_amd.align_pairs(bases, pairs)
        batch["align_call_s"] = round(time.perf_counter() - t, 3)
        return r

    r = roc.estimate_roc(p["m4"], p["ovl"], p["fasta"], min_ovl=2000, trials=trials, dp=dp, aligner=aligner)
    out = {k: v for k, v in r.as_dict().items() if k not in ("phases", "lines")}
    out["phases_s"] = {k: round(v, 3) for k, v in r.phases.items()}
    out["lines"] = r.lines
    out.update(batch)
    return out


def step_sampled(a):
    return _roc(a, 10000, True)


def step_full(a):
    return _roc(a, 0, True, save=_paths(a)["batch"])


def step_nodp(a):
    return _roc(a, 0, False)


def step_align(a):
    import mhap_amd
    z = np.load(_paths(a)["batch"])
    pairs = z["pairs"]
    t = time.perf_counter()
    mhap_amd.align_pairs(z["bases"], pairs)
    dt = time.perf_counter() - t
    cells = float((pairs[:, 1].astype(np.float64) * pairs[:, 3]).sum())
    return {"pairs": int(len(pairs)), "cells": cells, "wall_s": round(dt, 3)}


def child(step, a, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", step,
                                                                "--workdir", a.workdir, "--config", a.config]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, {"step": step, "config": a.config, "exit": r.returncode, "stderr": r.stderr[-1500:]}
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    return json.loads(lines[-1]) if lines else None, None


def kernel_stats(d):
    out = {"calls": 0, "ms": 0.0}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "align_pairs_kernel" in row.get("Name", ""):
                    out["calls"] += int(row.get("Calls", 0))
                    out["ms"] += float(row.get("TotalDurationNs", 0)) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--workdir")
    ap.add_argument("--config", default="c2")
    ap.add_argument("--configs", default="c2,c5slice")
    a = ap.parse_args()
    steps = {"prep": step_prep, "sampled": step_sampled, "full": step_full, "nodp": step_nodp, "align": step_align}
    if a.step:
        print(json.dumps(steps[a.step](a)))
        return 0
    a.workdir = a.workdir or tempfile.mkdtemp(prefix="roc_probe_")
    os.makedirs(a.workdir, exist_ok=True)
    res = {"tool": "roc_probe", "min_ovl": 2000}
    for cfg in a.configs.split(","):
        a.config = cfg
        r = res[cfg] = {}
        for step, limit in (("prep", 1200), ("sampled", 1200), ("full", 1800), ("nodp", 1200)):
            got, err = child(step, a, limit)
            r[step] = got
            if err:
                res["error"] = err
                print(json.dumps(res))
                return 1
        prof = os.path.join(a.workdir, cfg, "rocprof")
        os.makedirs(prof, exist_ok=True)
        got, err = child("align", a, 1200, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "kt", "--"])
        if err:
            res["error"] = err
            print(json.dumps(res))
            return 1
        ks = kernel_stats(prof)
        got["device_ms"] = round(ks["ms"], 3)
        got["kernel_calls"] = ks["calls"]
        got["cell_updates_per_s"] = got["cells"] / (ks["ms"] / 1e3) if ks["ms"] > 0 else None
        r["align_profiled"] = got
        full, nodp = r["full"], r["nodp"]
        r["dp_effect"] = {"pairs_checked": full["dp_pairs"], "rescued": full["tp"] - nodp["tp"], "rejected": full["fp"]}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
