"""The GPU k-mer counter (mhap_kmer_count_*) measured at size, on the GPU box; prints one JSON line.
  python tools/kmer_count_probe.py [--workdir DIR] [--reads 625000] [--histogram]
Steps, each a child process under its own `timeout` (the probe stops at the first that fails):
  c5rank   c5rank-shaped reads (625 000 x 12 kb, mhap_synth_reads_repeats) counted through the API (add_reads): wall time
           (--histogram: finished with the k-mer count histogram, then GetHistogramStats' loop, mhap_histogram_stats, timed on it)
  profile  the same step under `rocprofv3 --kernel-trace --stats`: device time of the counter's kernels per Gbase
           (--histogram: once with the histogram on, then once with it off)
  c2       C2 written as a FASTA file: mhap-hip-kmers file -> filter, then `mhap-hip -s file -f filter` end to end
  cpu      the numpy counter (workloads.count_kmers) on a 4 000-read sample: the CPU figure"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "mhap_amd", "lib")


def step_c5rank(a):
    os.environ.setdefault("MHAP_HOST_PROF", "1")   # ([kmer] lines on stderr: windows, flushes)
    import mhap_amd
    from mhap_amd import workloads as W
    t = time.time()
    fa = W.config_reads("c5rank", reads=a.reads)
    gen = time.time() - t
    bases = int(fa.lengths.astype("int64").sum())
    t = time.perf_counter()
    kc = mhap_amd.count_kmers(fa, k=16, canonical=True, min_fraction=2.5e-6, histogram=a.histogram)
    dt = time.perf_counter() - t
    out = {"reads": len(fa), "gbase": round(bases / 1e9, 3), "gen_s": round(gen, 1), "count_s": round(dt, 3),
           "gbase_per_s": round(bases / 1e9 / dt, 2), "total": kc.total, "distinct": kc.distinct, "lines": len(kc)}
    if a.histogram and a.stats:
        from mhap_amd import histogram_stats as H
        hc, hn = kc.histogram
        keep = hc <= 0x7FFFFFFF                        # (GetHistogramStats reads counts as int)
        t = time.perf_counter()
        mean, stdev, cut = H.histogram_stats(hc[keep].astype("int32"), hn[keep].astype("int64"), 0.99)
        out["stats"] = {"rows": int(keep.sum()), "kmers": int(hn[keep].sum()), "s": round(time.perf_counter() - t, 2),
                        "line": H.format_line(mean, stdev, cut)}
    return out


def step_c2(a):
    from mhap_amd import workloads as W
    fasta = os.path.join(a.workdir, "c2.fasta")
    t = time.time()
    W.write_fasta(W.config_reads("c2"), fasta)
    wr = time.time() - t
    out = {"fasta_gb": round(os.path.getsize(fasta) / 1e9, 3), "write_fasta_s": round(wr, 1)}
    kfile = os.path.join(a.workdir, "c2_kmers.txt")
    t = time.perf_counter()
    r = subprocess.run([os.path.join(LIB, "mhap-hip-kmers"), "-o", kfile, fasta], capture_output=True, text=True)
    out["kmers_cli_s"] = round(time.perf_counter() - t, 3)
    out["kmers_cli_rc"] = r.returncode
    out["kmers_cli_stderr"] = r.stderr.strip()[-400:]
    if r.returncode != 0:
        return out
    flags = ["--num-hashes", "512", "--ordered-sketch-size", "1536", "--filter-threshold", "1e-5"]
    for name, extra in (("mhap_hip_s", []), ("mhap_hip_s_f", ["-f", kfile])):
        t = time.perf_counter()
        r = subprocess.run([os.path.join(LIB, "mhap-hip"), "-s", fasta] + extra + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        out[name + "_s"] = round(time.perf_counter() - t, 3)
        out[name + "_rc"] = r.returncode
        out[name + "_records"] = r.stdout.count("\n")
        if r.returncode != 0:
            out[name + "_stderr"] = r.stderr[-400:]
            break
    return out


def step_cpu(a):
    from mhap_amd import workloads as W
    fa = W.config_reads("c5rank", reads=4000)
    t = time.perf_counter()
    u, cnt, total = W.count_kmers(fa, 16, True, max_reads=4000)
    dt = time.perf_counter() - t
    return {"reads": 4000, "windows": total, "s": round(dt, 3), "mbase_per_s": round(int(fa.lengths.sum()) / 1e6 / dt, 2)}


def child(step, a, limit, prefix=(), extra=()):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", step,
                                                                "--workdir", a.workdir, "--reads", str(a.reads)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, {"step": step, "exit": r.returncode, "stderr": r.stderr[-1500:]}
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    return json.loads(lines[-1]) if lines else None, None


def kernel_stats(d):
    out = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "kmer_" in name:
                    key = name.split("(")[0].replace("void ", "").replace("mhap::", "")
                    e = out.setdefault(key, {"calls": 0, "ms": 0.0})
                    e["calls"] += int(row.get("Calls", 0))
                    e["ms"] += float(row.get("TotalDurationNs", 0)) / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--workdir")
    ap.add_argument("--reads", type=int, default=625000)
    ap.add_argument("--profile-dir", help="where rocprofv3 writes its CSV files (default: WORKDIR/rocprof)")
    ap.add_argument("--histogram", action="store_true", help="finish with the k-mer count histogram; profile it on and off")
    ap.add_argument("--stats", action="store_true", help=argparse.SUPPRESS)   # (the c5rank child: time the stats loop too)
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"c5rank": step_c5rank, "c2": step_c2, "cpu": step_cpu}[a.step](a)))
        return 0
    a.workdir = a.workdir or tempfile.mkdtemp(prefix="kmer_probe_")
    os.makedirs(a.workdir, exist_ok=True)
    a.profile_dir = a.profile_dir or os.path.join(a.workdir, "rocprof")
    res = {"tool": "kmer_count_probe"}
    got, err = child("c5rank", a, 900, extra=["--histogram", "--stats"] if a.histogram else [])
    res["c5rank"] = got
    if err:
        res["error"] = err
        print(json.dumps(res))
        return 1
    for name, extra in ((("profile_histogram", ["--histogram"]), ("profile", [])) if a.histogram else (("profile", []),)):
        pdir = os.path.join(a.profile_dir, name)
        os.makedirs(pdir, exist_ok=True)
        got, err = child("c5rank", a, 900, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "kt", "--"], extra)
        if err:
            res["error"] = err
            print(json.dumps(res))
            return 1
        ks = kernel_stats(pdir)
        dev_ms = sum(v["ms"] for v in ks.values())
        res[name] = {"kernels": {k: {"calls": v["calls"], "ms": round(v["ms"], 2)} for k, v in ks.items()}, "device_ms": round(dev_ms, 2),
                     "device_ms_per_gbase": round(dev_ms / got["gbase"], 2) if got and got.get("gbase") else None}
    if a.histogram:   # (the c2 and cpu steps do not change with the histogram)
        print(json.dumps(res))
        return 0
    got, err = child("c2", a, 900)
    res["c2"] = got
    if err:
        res["error"] = err
        print(json.dumps(res))
        return 1
    got, err = child("cpu", a, 600)
    res["cpu_numpy"] = got
    if err:
        res["error"] = err
    print(json.dumps(res))
    return 0 if not err else 1


if __name__ == "__main__":
    sys.exit(main())
