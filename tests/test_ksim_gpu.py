"""KmerStatSimulator on the GPU: mhap_pair_kmer_stats against the transcription's compareKmers / BottomSketch on crafted pairs (both
scratch paths, packed and hashed keys, the narrowed key hash), and the CLI's stdout byte for byte against the transcription."""
import ctypes as C
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import api, kmer_sim as K  # noqa: E402
import ksim_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

PACBIO = (0.1188, 0.0183, 0.0129)
LDS = 160 * 1024    # LDS per workgroup on gfx950 (the kernel takes min(device limit, 160 KiB); the tests check the path it reports)


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, p=0.1):
    return "".join(rng.choice("ACGT") if rng.random() < p else c for c in s)


def _run(pairs_str, k, skip=()):
    bases, rows, off = [], [], 0
    for a, b in pairs_str:
        bases += [a, b]
        rows.append((off, len(a), off + len(a), len(b)))
        off += len(a) + len(b)
    buf = np.frombuffer("".join(bases).encode("latin-1"), dtype=np.uint8)
    return mhap_amd.pair_kmer_stats(buf, np.array(rows, dtype=np.int64), k, skip=skip), np.array(rows, dtype=np.int64)


def _paths(rows, k, hashed):
    out = np.zeros(len(rows), dtype=np.int32)
    assert api.load_library().mhap_pair_kmer_stats_paths(api._ptr(rows), C.c_int64(len(rows)), C.c_int32(k), C.c_int64(LDS),
                                                        C.c_int32(hashed), api._ptr(out)) == 0
    return out


def _lds_cap_len(k, hashed):
    """The longest equal-length pair that still takes the LDS path."""
    lo, hi = k, 1 << 16
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _paths(np.array([[0, mid, 0, mid]], dtype=np.int64), k, hashed)[0] == 1:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _crafted(k, rng):
    pairs = []
    for n in (max(k - 1, 0), k, k + 1, 3 * k + 5, 300):
        a = _rand(rng, n)
        pairs.append((a, _mutate(rng, a, 0.05)))
    a = _rand(rng, 500)
    pairs.append((a, _rand(rng, 500)))                                       # unrelated
    pairs.append(("A" * 400, "A" * 350))                                     # homopolymers: one k-mer, equal hashes everywhere
    pairs.append(("ACG" * 150, "CGA" * 140 + "T" * 20))                      # tandem repeats
    pairs.append((_rand(rng, 420, "ACGTNRYKMSW"), _rand(rng, 400, "ACGTN")))  # IUPAC bytes
    b = _rand(rng, 380)
    pairs.append((b, b[::-1]))
    pairs.append((b, "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[c] for c in reversed(b))))   # reverse complement: equal sketches
    pairs.append(("", "ACGT" * 10))
    return pairs


@pytest.mark.parametrize("k", [1, 12, 16, 31, 32, 33, 64])
def test_pair_stats_crafted(k):
    rng = random.Random(k)
    pairs = _crafted(k, rng)
    got, _ = _run(pairs, k)
    for (a, b), g in zip(pairs, got):
        assert tuple(g) == R.pair_stats(a, b, k), (k, len(a), len(b))


@pytest.mark.parametrize("k,hashed", [(16, False), (12, True), (40, True)])
def test_pair_stats_around_lds_cap_and_beyond(k, hashed):
    cap = _lds_cap_len(k, hashed)
    rng = random.Random(cap)
    alphabet = "ACGTN" if hashed else "ACGT"
    pairs = []
    for n in (cap, cap + 1, 3 * cap):
        a = _rand(rng, n, alphabet)
        pairs.append((a, _mutate(rng, a, 0.08)))
    got, rows = _run(pairs, k)
    assert list(_paths(rows, k, hashed)) == [1, 2, 2]
    buf = np.frombuffer("".join(x + y for x, y in pairs).encode("latin-1"), dtype=np.uint8)
    _, taken = mhap_amd.pair_kmer_stats(buf, rows, k, paths=True)
    assert list(taken) == [1, 2, 2]      # the paths the device took (a smaller LDS limit than 160 KiB would fail here, not pass quietly)
    for (a, b), g in zip(pairs, got):
        assert tuple(g) == R.pair_stats(a, b, k), (k, len(a))


def test_pair_stats_skip_mers():
    rng = random.Random(5)
    k = 12
    a = _rand(rng, 600)
    b = a[100:] + _rand(rng, 100)
    only_a = a[:k]                      # in the first read only
    both = [a[200 + 13 * i:200 + 13 * i + k] for i in range(20)]   # in both reads
    skip = [only_a] + both + ["ACGT", "A" * 40]                     # other lengths never match
    iupac_a = a[:300] + "N" + a[300:]
    pairs = [(a, b), (b, a), (iupac_a, b)]
    got, _ = _run(pairs, k, skip=skip)
    for (x, y), g in zip(pairs, got):
        assert tuple(g) == R.pair_stats(x, y, k, skip=skip)
    plain, _ = _run(pairs[:1], k)
    assert got[0][0] == plain[0][0] - len(set(both)) and got[0][1] == plain[0][1]


def test_pair_stats_narrowed_key_hash():
    rng = random.Random(9)
    pairs = _crafted(16, rng) + [(_rand(rng, 2000), _rand(rng, 2000))]
    a = _rand(rng, 3000)
    pairs.append((a, _mutate(rng, a)))
    env = dict(os.environ, MHAP_KSIM_HASH_BITS="3")
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); import mhap_amd; d = json.load(sys.stdin);"
            "r = mhap_amd.pair_kmer_stats(np.frombuffer(d['b'].encode(), np.uint8), np.array(d['p'], np.int64), 16);"
            "print(json.dumps(r.tolist()))" % ROOT)
    import json
    bases, rows, off = [], [], 0
    for x, y in pairs:
        bases += [x, y]
        rows.append([off, len(x), off + len(x), len(y)])
        off += len(x) + len(y)
    r = subprocess.run([sys.executable, "-c", code], input=json.dumps({"b": "".join(bases), "p": rows}), capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    for (x, y), g in zip(pairs, got):
        assert tuple(g) == R.pair_stats(x, y, 16)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "mhap_amd.kmer_sim", *map(str, args)], cwd=ROOT, capture_output=True, text=True, timeout=900)


def test_cli_usage1_stdout_equals_transcription():
    r = _cli(30, 16, 400, 100, *PACBIO)
    assert r.returncode == 0, r.stderr
    want, _ = R.run(30, 400, *PACBIO, k=16, overlap=100)
    assert r.stdout == want
    # (the GPU runtime may add lines of its own to stderr)
    assert [x for x in r.stderr.splitlines() if x.startswith(("Started", "Loaded", "Done"))] == ["Started...", "Loaded reference", "Done 0/30"]


def _fasta(tmp_path, recs):
    p = tmp_path / "ref.fa"
    p.write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(recs)))
    return str(p)


def test_cli_reference_skip_and_one_sided(tmp_path):
    rng = random.Random(2)
    recs = [_rand(rng, n) for n in (1700, 900, 4000, 500)]
    raw = [recs[0][:10] + "N" + recs[0][10:]] + recs[1:]
    path = _fasta(tmp_path, raw)
    skip_p = tmp_path / "skip.txt"
    skip = {recs[2][i:i + 16]: 3 for i in range(0, 2000, 7)}
    skip_p.write_text("".join(f"{m}\t{c}\n" for m, c in skip.items()))
    r = _cli(30, 16, 400, 150, *PACBIO, "true", path, str(skip_p))
    assert r.returncode == 0, r.stderr
    want, _ = R.run(30, 400, *PACBIO, k=16, overlap=150, one_sided=True, reference=recs, skip=skip)
    assert r.stdout == want
    r = _cli(30, 12, 400, 100, 0.05, 0.05, 0.05, "false", path)
    assert r.returncode == 0, r.stderr
    assert r.stdout == R.run(30, 400, 0.05, 0.05, 0.05, k=12, overlap=100, reference=recs)[0]


def test_api_chunking_does_not_change_columns():
    a = K.simulate_pairs(23, 16, 300, 100, *PACBIO, chunk=5)
    b = K.simulate_pairs(23, 16, 300, 100, *PACBIO)
    assert np.array_equal(a, b, equal_nan=True) and a.shape == (23, 7)
    f = R.KmerStatSimulator(0)
    f.totalTrials, f.requestedLength, f.kmer, f.overlap = 23, 300.0, 16, 100
    f.simulate(*PACBIO)
    assert a[:, 0].tolist() == f.sharedMerCounts and a[:, 6].tolist() == f.randomMinHash


# ---- --rng device ---------------------------------------------------------------------------------------------------------
def _genome(seed, n):
    rng = random.Random(seed)
    return _rand(rng, n)


def test_device_chunking_does_not_change_output():
    recs = [_genome(1, 9000), _genome(2, 2500)]
    args = (37, 16, 500, 150, 0.1, 0.03, 0.02)
    kw = dict(reference=recs, rng="device", seed=5, return_reads=True)
    base = K.simulate_pairs(*args, **kw)
    for chunk in (1, 7):
        got = K.simulate_pairs(*args, chunk=chunk, **kw)
        for a, b in zip(base, got):
            assert np.array_equal(a, b, equal_nan=True), chunk
    reads_all, ids_all = K.simulate_reads(19, 300, 0.1, 0.03, 0.02, rng="device", seed=5)
    reads_7, ids_7 = K.simulate_reads(19, 300, 0.1, 0.03, 0.02, rng="device", seed=5, chunk=7)
    assert np.array_equal(reads_all, reads_7) and np.array_equal(ids_all, ids_7)


def test_device_error_zero_reads_are_genome_windows():
    recs = [_genome(3, 5000), _genome(4, 1500), _genome(5, 800)]
    L = 300
    cols, reads, meta, ev = K.simulate_pairs(50, 16, L, 100, 0.0, 0.0, 0.0, reference=recs, rng="device", seed=9, return_reads=True)
    for t in range(50):
        sid, fpos, spos, rsid, rpos = (int(x) for x in meta[t])
        g, rg = recs[sid], recs[rsid]
        assert len(g) >= 4 * L and len(rg) >= 2 * L
        assert reads[t, 0].tobytes().decode() == "".join(g[(fpos + L + i) % len(g)] for i in range(L))   # the last L of the 2L window
        assert reads[t, 1].tobytes().decode() == "".join(g[(spos + i) % len(g)] for i in range(L))
        assert reads[t, 2].tobytes().decode() == "".join(rg[(rpos + i) % len(rg)] for i in range(L))
        assert spos == (fpos + 2 * L - 100) % len(g)
        assert not (rsid == sid and min(fpos + L, rpos + L) - max(fpos, rpos) + 1 > 0)
    assert (ev[:, :, :3] == 0).all() and (ev[:, :, 3] == 2 * L).all()
    reads2, ids = K.simulate_reads(5, L, 0.0, 0.0, 0.0, reference=recs, rng="device", seed=9)
    for t in range(5):
        g = recs[ids[t, 0]]
        fpos = ids[t, 1] - L
        assert reads2[t].tobytes().decode() == "".join(g[(fpos + L + i) % len(g)] for i in range(L))


@pytest.mark.parametrize("ref", [False, True])
def test_device_statistics_recomputed_on_cpu(ref):
    recs = [_genome(6, 4000), "ACGTRYACGT" * 150] if ref else None
    k, L = 12, 250
    cols, reads, meta, ev = K.simulate_pairs(25, k, L, 80, 0.08, 0.02, 0.03, reference=recs, rng="device", seed=2, return_reads=True)
    kk = min(K.BOTTOM_K, L - k + 1)
    for t in range(25):
        a, b, c = (reads[t, r].tobytes().decode() for r in range(3))
        for (x, y), (cs, cj, cm) in (((a, b), (0, 1, 2)), ((a, c), (4, 5, 6))):
            sh, tot, inter = R.pair_stats(x, y, k)
            assert cols[t, cs] == sh and cols[t, cj] == sh / tot and cols[t, cm] == inter / kk
        assert cols[t, 3] == K.jaccard_to_identity(cols[t, 2], k)


def test_device_realised_error_rates():
    ins, dele, sub = 0.06, 0.04, 0.05
    err = ins + dele + sub
    _, _, _, ev = K.simulate_pairs(400, 16, 1000, 200, ins, dele, sub, rng="device", seed=11, return_reads=True)
    ev = ev[:, :2].reshape(-1, 4).sum(axis=0).astype(np.float64)    # the first reads and the shared partners (the random ones: no walk)
    V = ev[3]
    for got, rate in zip(ev[:3], (ins, dele, sub)):
        p = rate                                    # per visit: P(error) * P(type | error) = the configured rate
        se = math.sqrt(p * (1 - p) / V)
        assert abs(got / V - p) <= 4 * se, (got / V, p)
    assert abs((ev[0] + ev[1] + ev[2]) / V - err) <= 4 * math.sqrt(err * (1 - err) / V)


@pytest.mark.parametrize("setting", ["pacbio_noref", "low_error_ref"])
def test_device_means_match_java_mode(setting):
    if setting == "pacbio_noref":
        args, recs = (2000, 16, 800, 300, *PACBIO), None
    else:
        args, recs = (2000, 12, 500, 250, 0.03, 0.01, 0.02), [_genome(8, 60000), _genome(9, 3000)]
    j = K.simulate_pairs(*args, reference=recs, rng="java", seed=0)
    d = K.simulate_pairs(*args, reference=recs, rng="device", seed=0)
    n = len(j)
    for c in (0, 2):     # mean shared k-mer count, mean shared MinHash Jaccard
        se = math.sqrt(j[:, c].var(ddof=1) / n + d[:, c].var(ddof=1) / n)
        assert abs(j[:, c].mean() - d[:, c].mean()) <= 4 * se, (setting, c, j[:, c].mean(), d[:, c].mean(), se)


def test_device_cli_both_usages(tmp_path):
    r = _cli("--rng", "device", 12, 16, 400, 100, *PACBIO)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 12 + 6 and all(len(x.split("\t")) == 7 for x in lines[:12])
    assert lines[12].startswith("Shared mer counts stats: ") and lines[17].startswith("Random MinHash jaccard stats: ")
    path = _fasta(tmp_path, [_genome(10, 3000)])
    r = _cli("--rng", "device", "--seed", 4, 6, 130, *PACBIO, path)
    assert r.returncode == 0, r.stderr
    reads, ids = K.simulate_reads(6, 130, *PACBIO, reference=path, rng="device", seed=4)
    want = "".join(f">s{i} {ids[i, 0]} {ids[i, 1]}\n{K.convert_to_fasta(reads[i].tobytes().decode())}\n" for i in range(6))
    assert r.stdout == want and r.stdout.splitlines()[1] == reads[0].tobytes().decode()[:60]


def test_device_too_short_raises():
    with pytest.raises(K.KsimError, match="shorter than"):
        K.simulate_pairs(20, 12, 200, 50, 0.0, 0.6, 0.0, rng="device")
