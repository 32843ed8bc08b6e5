"""KmerStatSimulator (mhap_amd.kmer_sim) in Java-exact and device mode at L = 5 000, k = 16, overlap 1 000 and the PacBio mix 0.1188 / 0.0183 /
0.0129 (BASELINE's); prints one JSON line and writes it to --out (default profiles/ksim_probe.json).
  python tools/ksim_probe.py [--trials 10000] [--workdir DIR] [--out FILE]
Steps, each a child process under its own `timeout` (the probe stops at the first that fails):
  gen      the host replay alone (mhap_ksim_next): trials/s; the trials are saved for the next step
  gpu      the saved trials' pairs through pair_kmer_stats alone, after a warm-up call: wall time per pair and per window
  e2e      simulate_pairs end to end (generation overlapped with the GPU) and the shared-pair identity distribution; the one-time
           setup (torch's runtime, the library handle, a warm-up run) is timed apart as setup_s
  device   --rng device, 10^6 trials (generator kernel + the same stats kernel), timed the same way; formatting timed apart
  kernels  the gpu step's batch and a 20 000-trial device run once more under `rocprofv3 --kernel-trace --stats`: device time per
           pair and per window of the stats kernel, and of the generator kernel
The bound beside the device time is computed from shapes: the LDS bytes the two bitonic sorts of a pair move (16 B per slot and pass,
read and written) over the LDS bandwidth of all CUs (128 B/clk/CU at 2.4 GHz, 256 CUs; MI355X_MICROARCH)."""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, K, OVERLAP, RATES = 5000, 16, 1000, (0.1188, 0.0183, 0.0129)


def _batch(a):
    return os.path.join(a.workdir, "trials.npy")


def _pairs(m):
    t = np.arange(m, dtype=np.int64) * 3 * L
    rows = np.zeros((2 * m, 4), dtype=np.int64)
    rows[0::2, 0] = t; rows[0::2, 2] = t + L
    rows[1::2, 0] = t; rows[1::2, 2] = t + 2 * L
    rows[:, 1] = L; rows[:, 3] = L
    return rows


def step_gen(a):
    from mhap_amd import kmer_sim as KS
    err, pi, pd, ps = KS._rates(*RATES)
    g = KS._JavaTrials(0, L, 2 * L - OVERLAP, err, pi, pd, ps, False, False, None)
    t = time.perf_counter()
    reads, _, done, e = g.next(a.trials)
    dt = time.perf_counter() - t
    g.close()
    assert e is None and done == a.trials
    np.save(_batch(a), reads)
    return {"trials": a.trials, "gen_s": round(dt, 3), "gen_trials_per_s": round(a.trials / dt, 1)}


def step_gpu(a):
    import mhap_amd
    reads = np.load(_batch(a))
    rows = _pairs(len(reads))
    b = reads.reshape(-1)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1, device=0)) as ms:
        mhap_amd.pair_kmer_stats(b[:3 * L * 64], rows[:128], K, handle=ms)   # warm-up (allocation, code object)
        t = time.perf_counter()
        mhap_amd.pair_kmer_stats(b, rows, K, handle=ms)
        dt = time.perf_counter() - t
    n = len(rows)
    return {"pairs": n, "gpu_s": round(dt, 3), "us_per_pair": round(dt / n * 1e6, 2), "ns_per_window": round(dt / (2 * n * (L - K + 1)) * 1e9, 3)}


def _warm_session():
    """torch's HIP runtime, the library handle and a KsimDevice, warmed by a small run: the one-time setup a process pays once."""
    import torch  # noqa: F401
    from mhap_amd import api, kmer_sim as KS
    t = time.perf_counter()
    ses = api.KsimDevice(0)
    KS.simulate_pairs(16, K, float(L), OVERLAP, *RATES, session=ses)
    KS.simulate_pairs(16, K, float(L), OVERLAP, *RATES, rng="device", session=ses)
    return ses, time.perf_counter() - t


def step_e2e(a):
    from mhap_amd import kmer_sim as KS
    ses, setup = _warm_session()
    t = time.perf_counter()
    cols = KS.simulate_pairs(a.trials, K, float(L), OVERLAP, *RATES, session=ses)
    dt = time.perf_counter() - t
    ses.close()
    t = time.perf_counter()
    text = KS.format_lines(cols)
    fmt = time.perf_counter() - t
    ident = cols[:, 3]
    q = np.quantile(ident, [0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99]).tolist()
    return {"trials": a.trials, "setup_s": round(setup, 3), "e2e_s": round(dt, 3), "trials_per_s": round(a.trials / dt, 1),
            "format_s": round(fmt, 3), "stdout_bytes": len(text),
            "shared_identity_quantiles": {p: round(v, 4) for p, v in zip(("1", "10", "25", "50", "75", "90", "99"), q)},
            "shared_identity_mean": round(float(ident.mean()), 4), "shared_identity_ge_0_78": round(float((ident >= 0.78).mean()), 4),
            "shared_minhash_jaccard_mean": round(float(cols[:, 2].mean()), 4), "random_minhash_jaccard_mean": round(float(cols[:, 6].mean()), 5),
            "random_identity_max": round(float(np.nanmax([KS.jaccard_to_identity(v, K) for v in cols[:, 6]])), 4)}


def step_device(a):
    from mhap_amd import kmer_sim as KS
    ses, setup = _warm_session()
    t = time.perf_counter()
    cols = KS.simulate_pairs(a.device_trials, K, float(L), OVERLAP, *RATES, rng="device", session=ses)
    dt = time.perf_counter() - t
    ses.close()
    t = time.perf_counter()
    text = KS.format_lines(cols)
    fmt = time.perf_counter() - t
    return {"trials": a.device_trials, "setup_s": round(setup, 3), "wall_s": round(dt, 3), "trials_per_s": round(a.device_trials / dt, 1),
            "format_s": round(fmt, 3), "stdout_bytes": len(text),
            "shared_mer_count_mean": round(float(cols[:, 0].mean()), 3), "shared_minhash_jaccard_mean": round(float(cols[:, 2].mean()), 5),
            "shared_identity_ge_0_78": float((cols[:, 3] >= 0.78).mean()), "random_identity_max": round(float(np.nanmax(
                [KS.jaccard_to_identity(v, K) for v in np.unique(cols[:, 6])])), 4)}


def step_kernels(a):
    from mhap_amd import kmer_sim as KS
    out = step_gpu(a)
    KS.simulate_pairs(a.profile_device_trials, K, float(L), OVERLAP, *RATES, rng="device")
    out["device_trials"] = a.profile_device_trials
    return out


def child(step, a, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", step, "--workdir",
                                                                a.workdir, "--trials", str(a.trials), "--device-trials", str(a.device_trials),
                                                                "--profile-device-trials", str(a.profile_device_trials)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        return None, {"step": step, "exit": r.returncode, "stderr": r.stderr[-1500:]}
    lines = [x for x in r.stdout.split("\n") if x.startswith("{")]
    return json.loads(lines[-1]) if lines else None, None


def kernel_stats(d, name):
    out = {"calls": 0, "ms": 0.0}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if name in row.get("Name", ""):
                    out["calls"] += int(row.get("Calls", 0))
                    out["ms"] += float(row.get("TotalDurationNs", 0)) / 1e6
    return out


def lds_bound_s(pairs):
    """Two bitonic sorts of P = 16 384 slots per pair (packed keys, both reads' windows): 16 B of LDS traffic per slot and pass."""
    P = 1 << math.ceil(math.log2(2 * (L - K + 1)))
    passes = int(math.log2(P) * (math.log2(P) + 1) / 2)
    bytes_per_pair = 2 * passes * P * 16
    return pairs * bytes_per_pair / (128 * 2.4e9 * 256), bytes_per_pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--workdir")
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--device-trials", type=int, default=1000000)
    ap.add_argument("--profile-device-trials", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksim_probe.json"))
    a = ap.parse_args()
    steps = {"gen": step_gen, "gpu": step_gpu, "e2e": step_e2e, "device": step_device, "kernels": step_kernels}
    if a.step:
        print(json.dumps(steps[a.step](a)))
        return 0
    a.workdir = a.workdir or tempfile.mkdtemp(prefix="ksim_probe_")
    os.makedirs(a.workdir, exist_ok=True)
    res = {"tool": "ksim_probe", "L": L, "k": K, "overlap": OVERLAP, "rates": RATES}
    for step, limit in (("gen", 900), ("gpu", 900), ("e2e", 1200), ("device", 1500)):
        got, err = child(step, a, limit)
        res[step] = got
        if err:
            res["error"] = err
            print(json.dumps(res))
            return 1
    prof = os.path.join(a.workdir, "rocprof")
    os.makedirs(prof, exist_ok=True)
    got, err = child("kernels", a, 900, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "kt", "--"])
    if err:
        res["error"] = err
    else:
        ks = kernel_stats(prof, "pair_kmer_stats_kernel")
        kg = kernel_stats(prof, "ksim_gen_kernel")
        n = got["pairs"] + 128 + 2 * a.profile_device_trials           # the gpu step's pairs, its warm-up and the device run's pairs
        bound, bpp = lds_bound_s(n)
        res["kernels"] = {"stats_calls": ks["calls"], "stats_device_ms": round(ks["ms"], 3), "pairs": n,
                          "us_per_pair": round(ks["ms"] * 1e3 / n, 2), "ns_per_window": round(ks["ms"] * 1e6 / (n * 2 * (L - K + 1)), 3),
                          "lds_bytes_per_pair": bpp, "lds_bound_ms": round(bound * 1e3, 3),
                          "fraction_of_lds_bound": round(bound * 1e3 / ks["ms"], 3) if ks["ms"] > 0 else None,
                          "gen_calls": kg["calls"], "gen_device_ms": round(kg["ms"], 3), "gen_trials": a.profile_device_trials,
                          "gen_ns_per_source_base": round(kg["ms"] * 1e6 / (a.profile_device_trials * 2 * 2 * L), 4) if kg["ms"] else None}
    e, g, gp, dv = res["e2e"], res["gen"], res["gpu"], res["device"]
    res["summary"] = {"java_trials_per_s_e2e": e["trials_per_s"], "host_gen_s": g["gen_s"], "gpu_s": gp["gpu_s"],
                      "java_e2e_over_host_gen": round(e["e2e_s"] / g["gen_s"], 2), "device_trials_per_s": dv["trials_per_s"],
                      "device_over_java_trials_per_s": round(dv["trials_per_s"] / e["trials_per_s"], 1)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")
    return 0 if "error" not in res else 1


if __name__ == "__main__":
    sys.exit(main())
