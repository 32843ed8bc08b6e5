"""Exact k-mer counting on the GPU and the `-f` repeat filter file made from it (mhap_kmer_count_*, mhap_amd.count_kmers,
mhap-hip-kmers): the window arithmetic on the host, the file byte for byte against workloads.write_filter_file, the streamed ingest
path against a plain Counter, the filter in use against the oracle, the CLI, and the error paths."""
import collections
import ctypes as C
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import mhap_amd
from mhap_amd import FastaData, MhapParams, MinHashSearch, api
from mhap_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMERS_CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip-kmers")
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
_RC = str.maketrans("ACGT", "TGCA")


def _value(s):
    v = 0
    for c in s:
        v = (v << 2) | "ACGT".index(c)
    return v


def _py_windows(seq, k, canonical):
    """The counter's windows restated: a window counts when its k bytes are all A/C/G/T (upper case)."""
    vals, valid = [], []
    for i in range(len(seq) - k + 1):
        w = seq[i:i + k]
        if all(c in "ACGT" for c in w):
            v = _value(w)
            if canonical:
                v = min(v, _value(w.translate(_RC)[::-1]))
            vals.append(v)
            valid.append(1)
        else:
            vals.append(0)
            valid.append(0)
    return vals, valid


def _selftest(seq, k, canonical):
    lib = mhap_amd.load_library()
    s = seq.encode("latin-1")
    n = max(len(s) - k + 1, 0)
    out = np.zeros(max(n, 1), np.uint64)
    ok = np.zeros(max(n, 1), np.uint8)
    rc = lib.mhap_selftest_kmer_windows(s, C.c_int32(len(s)), C.c_int32(k), C.c_int32(1 if canonical else 0), api._ptr(out), api._ptr(ok))
    return rc, out[:n].tolist(), ok[:n].tolist()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", list(range(1, 17)))
def test_kernel_window_arithmetic_matches_python(k):
    rnd = random.Random(1000 + k)
    seqs = ["".join(rnd.choice("ACGT") for _ in range(300)),
            "".join(rnd.choice("ACGTNRYKMSWBDHVacgtn") for _ in range(300)),
            "".join(rnd.choice("ACGT") for _ in range(40)) + "N" * (k + 2) + "".join(rnd.choice("ACGT") for _ in range(40)),
            "A" * 50 + "T" * 50, "".join(rnd.choice("ACGT") for _ in range(k - 1)), ""]
    if k % 2 == 0:                                                   # palindromes: value == value of the reverse complement
        half = "".join(rnd.choice("ACGT") for _ in range(k // 2))
        seqs.append(half + half.translate(_RC)[::-1])
    for seq in seqs:
        for canonical in (True, False):
            rc, got, ok = _selftest(seq, k, canonical)
            assert rc == 0
            want, wok = _py_windows(seq, k, canonical)
            assert ok == wok, (seq, k)
            assert got == want, (seq, k, canonical)
    if k % 2 == 0:
        _, got, ok = _selftest(seqs[-1], k, True)
        assert ok == [1] and got == [_value(seqs[-1])]


def test_unsupported_k_is_rejected_on_the_host():
    for k in (0, 17, -3):
        rc, _, _ = _selftest("ACGTACGTACGTACGTACGT", k, True)
        assert rc == -1, k
    for k in ("0", "17"):
        r = subprocess.run([KMERS_CLI, "-o", "/dev/null", "-k", k, "x.fasta"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "from 1 to 16" in r.stderr, r.stderr
    r = subprocess.run([KMERS_CLI, "-o", "/dev/null", "--min-fraction", "abc", "x.fasta"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--min-fraction" in r.stderr
    r = subprocess.run([KMERS_CLI, "x.fasta"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-o" in r.stderr


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

def _mixed_reads():
    """Synthetic reads (2-bit packed by the counter) plus reads with N runs, IUPAC codes and lower-case bytes (raw), short reads."""
    fa = mhap_amd.synth_reads(24, 1500, seed=77, error_rate=0.1, repeats=(200, 1500, 0.02))
    rnd = random.Random(5)
    extra = ["".join(rnd.choice("ACGT") for _ in range(400)) + "N" * 30 + "".join(rnd.choice("ACGT") for _ in range(300)),
             "".join(rnd.choice("ACGTRYKM") for _ in range(500)), "ACGTACGTAC", "A" * 700, "ACGT" * 5]
    seqs = [fa.sequence(i) for i in range(len(fa))] + extra
    mixed = FastaData.from_strings(seqs)
    low = "".join(rnd.choice("ACGTacgt") for _ in range(600)).encode()   # (from_strings upper-cases: lower-case bytes set by hand)
    bases = np.concatenate([mixed.bases, np.frombuffer(low, np.uint8)])
    return FastaData(bases, np.append(mixed.offsets, len(mixed.bases)), np.append(mixed.lengths, len(low)),
                     np.arange(1, len(mixed) + 2, dtype=np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [9, 12, 15, 16])
def test_filter_file_is_byte_identical_to_the_numpy_counter(tmp_path, k):
    fa = _mixed_reads()
    thirds = np.array_split(np.arange(len(fa)), 3)
    for canonical in (True, False):
        for mf in (0.0, 2.5e-6):
            with MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=0)) as ms:
                ms.kmer_count_begin(k, canonical)
                for part in thirds:                                          # several add_reads calls
                    ms.kmer_count_add(fa.subset(part))
                kc = ms.kmer_count_finish(mf)
            got, want = tmp_path / "got.txt", tmp_path / "want.txt"
            kc.write(got)
            W.write_filter_file(fa, str(want), k=k, min_fraction=mf, canonical=canonical, max_reads=None)
            assert got.read_bytes() == want.read_bytes(), (k, canonical, mf)
            u, cnt, total = W.count_kmers(fa, k, canonical, max_reads=None)
            assert kc.total == total and kc.distinct == len(u) and kc.k == k
            if mf == 0.0:
                assert len(kc) == len(u) and sorted(kc.kmers.tolist()) == u.tolist()


def _awkward_fasta(path):
    rnd = random.Random(11)
    recs, seqs = [], []
    for i in range(600):                                                     # 1.1 Mbase: past the ingest's 1-Mbase first group
        kind = i % 6
        L = rnd.randint(1000, 3500)
        s = "".join(rnd.choice("ACGT") for _ in range(L))
        if kind == 1:
            a = rnd.randint(0, L - 50)
            s = s[:a] + "N" * rnd.randint(1, 40) + s[a + 40:]
        elif kind == 2:
            s = "".join(c if rnd.random() > 0.02 else rnd.choice("RYKMSWBDHVN") for c in s)
        elif kind == 3:
            s = s.lower()
        elif kind == 4:
            s = s[:rnd.randint(0, 15)]                                       # shorter than k (or empty)
        seqs.append(s)
        body = "\n".join(s[j:j + 70] for j in range(0, len(s), 70))          # multi-line records
        recs.append(f">read{i} some description\n{body}\n")
    with gzip.open(path, "wt") as fh:
        fh.write("".join(recs))
    return seqs


_CHILD = r"""
import sys
import mhap_amd
kc = mhap_amd.count_kmers(sys.argv[1], k=int(sys.argv[3]), canonical=sys.argv[4] == "1", min_fraction=0.0)
kc.write(sys.argv[2])
print(kc.total, kc.distinct, len(kc))
"""


@pytest.mark.gpu
def test_scan_path_on_an_awkward_fasta_matches_a_counter(tmp_path):
    path = tmp_path / "reads.fasta.gz"
    seqs = _awkward_fasta(str(path))
    k = 16
    for canonical in (True, False):
        cnt = collections.Counter()
        for s in seqs:
            s = s.upper()
            r = s.translate(_RC)[::-1]
            run, L = 0, len(s)
            for i, c in enumerate(s):                                        # i = the window's last base
                run = run + 1 if c in "ACGT" else 0
                if run >= k:
                    w = s[i - k + 1:i + 1]
                    cnt[min(w, r[L - 1 - i:L - 1 - i + k]) if canonical else w] += 1
        total = sum(cnt.values())
        out = tmp_path / f"k{int(canonical)}.txt"
        # small ingest groups and a small staging budget: many groups and more than one flush of the staged windows
        env = dict(os.environ, MHAP_INGEST_GROUP_BASES="6000", MHAP_KMER_STAGE_WINDOWS="15000", MHAP_HOST_PROF="1",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", _CHILD, str(path), str(out), str(k), "1" if canonical else "0"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stderr.count("[ingest] group") >= 10, r.stderr[-3000:]
        assert r.stderr.count("[kmer] flush") >= 2, r.stderr[-3000:]
        want = [f"{len(cnt)} {len(cnt)}"] + [f"{km}\t{c / total:.10e}" for km, c in sorted(cnt.items(), key=lambda kv: (-kv[1], kv[0]))]
        assert out.read_text().split("\n")[:-1] == want
        assert r.stdout.split() == [str(total), str(len(cnt)), str(len(cnt))]


@pytest.mark.gpu
def test_the_filter_in_use_matches_the_oracle(tmp_path):
    fa = mhap_amd.synth_reads(150, 3000, seed=404, error_rate=0.05, repeats=(300, 1500, 0.01))
    kc = mhap_amd.count_kmers(fa, k=16, canonical=True, min_fraction=1e-5)
    assert len(kc) > 100 and kc.distinct > len(kc)
    path = tmp_path / "kmers.txt"
    kc.write(path)
    mem = mhap_amd.FrequencyCounts.from_counts(kc, filter_cutoff=1e-5, repeat_weight=0.9)
    fil = mhap_amd.FrequencyCounts.from_file(str(path), filter_cutoff=1e-5, repeat_weight=0.9)
    for a in ("hashes", "fractions", "whitelist"):
        assert getattr(mem, a).tobytes() == getattr(fil, a).tobytes(), a
    assert mem.size_bloom == fil.size_bloom == kc.distinct
    assert (mem.offset, mem.range, mem.no_tf, mem.filter_cutoff) == (fil.offset, fil.range, fil.no_tf, fil.filter_cutoff)
    p = MhapParams(num_hashes=128, ordered_sketch_size=512, device=0)

    def records(flt):
        with MinHashSearch(p, kmer_filter=flt) as ms:
            ms.add_data(fa)
            return sorted(mhap_amd.records_to_lines(ms.find_matches()))
    got_mem, got_file, plain = records(mem), records(fil), records(None)
    oflt = O.Filter(fil.hashes, fil.fractions, 1e-5, 0.9, 3.0, False)
    want = O.record_lines(O.run_self(fa, H=128, S=512, nthreads=8, flt=oflt)["records"])
    assert got_mem == got_file == want and len(want) > 50
    assert plain != want                                                 # the filter changes the records


@pytest.mark.gpu
def test_cli_writes_the_api_file_and_mhap_hip_uses_it(tmp_path):
    fa = mhap_amd.synth_reads(120, 3000, seed=31, error_rate=0.05, repeats=(300, 1500, 0.01))
    fasta = tmp_path / "r.fasta"
    W.write_fasta(fa, str(fasta))
    out = tmp_path / "kmers.txt"
    r = subprocess.run([KMERS_CLI, "-o", str(out), "--min-fraction", "1e-5", str(fasta)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert len([l for l in r.stderr.split("\n") if l]) == 1 and "Counted" in r.stderr
    api_file = tmp_path / "api.txt"
    mhap_amd.count_kmers(str(fasta), min_fraction=1e-5).write(api_file)
    assert out.read_bytes() == api_file.read_bytes()
    gzdir = tmp_path / "gz"
    gzdir.mkdir()
    with open(fasta, "rb") as src, gzip.open(gzdir / "r.fasta.gz", "wb") as dst:
        dst.write(src.read())
    r2 = subprocess.run([KMERS_CLI, "-o", str(tmp_path / "nrc.txt"), "--no-rc", "-k", "12", "--min-fraction", "0", str(gzdir)],
                        capture_output=True, text=True, timeout=300)   # (a directory: every file in it)
    assert r2.returncode == 0, r2.stderr
    W.write_filter_file(fa, str(tmp_path / "nrc_want.txt"), k=12, min_fraction=0.0, canonical=False, max_reads=None)
    assert (tmp_path / "nrc.txt").read_bytes() == (tmp_path / "nrc_want.txt").read_bytes()
    flags = ["--num-hashes", "128", "--ordered-sketch-size", "512", "--filter-threshold", "1e-5"]
    m = subprocess.run([CLI, "-s", str(fasta), "-f", str(out)] + flags, capture_output=True, text=True, timeout=300)
    assert m.returncode == 0, m.stderr[-2000:]
    lines = sorted(l for l in m.stdout.split("\n") if l)
    flt = mhap_amd.FrequencyCounts.from_file(str(out), filter_cutoff=1e-5, repeat_weight=0.9)
    oflt = O.Filter(flt.hashes, flt.fractions, 1e-5, 0.9, 3.0, False)
    want = O.record_lines(O.run_self(FastaData.from_file(str(fasta)), H=128, S=512, nthreads=8, flt=oflt)["records"])
    assert lines == want and len(lines) > 50
    bad = subprocess.run([KMERS_CLI, "-o", str(tmp_path / "x.txt"), str(tmp_path / "missing.fasta")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "missing.fasta" in bad.stderr


@pytest.mark.gpu
def test_error_paths(tmp_path):
    fa = mhap_amd.synth_reads(8, 500, seed=3)
    with MinHashSearch(MhapParams(num_hashes=16, ordered_sketch_size=64, device=0)) as ms:
        with pytest.raises(mhap_amd.MhapError, match="no k-mer count is open"):
            ms.kmer_count_add(fa)                                        # add before begin
        with pytest.raises(mhap_amd.MhapError, match="no k-mer count is open"):
            ms.kmer_count_finish()
        for k in (0, 17):
            with pytest.raises(mhap_amd.MhapError, match="from 1 to 16"):
                ms.kmer_count_begin(k)
        ms.kmer_count_begin(16)
        with pytest.raises(mhap_amd.MhapError, match="already open"):
            ms.kmer_count_begin(16)
        ms.kmer_count_add(fa)
        kc = ms.kmer_count_finish(0.0)
        assert kc.total == 8 * (500 - 15)
        with pytest.raises(mhap_amd.MhapError, match="no k-mer count is open"):
            ms.kmer_count_finish()                                       # finish twice
        ms.kmer_count_begin(12)
        ms.kmer_count_add(fa)
        ms.add_data(fa)                                                  # an index call in between closes the count
        with pytest.raises(mhap_amd.MhapError, match="index changed"):
            ms.kmer_count_add(fa)
        with pytest.raises(mhap_amd.MhapError, match="no k-mer count is open"):
            ms.kmer_count_finish()
        ms.kmer_count_begin(12)                                          # and a new one works
        ms.kmer_count_add(fa)
        assert ms.kmer_count_finish(0.0).total == 8 * (500 - 11)
    with pytest.raises(mhap_amd.MhapError):
        mhap_amd.count_kmers(str(tmp_path / "missing.fasta"))
    for k in (0, 17):
        with pytest.raises(mhap_amd.MhapError, match="from 1 to 16"):
            mhap_amd.count_kmers(fa, k=k)
    empty = mhap_amd.count_kmers(FastaData.from_strings([]))
    empty.write(tmp_path / "e.txt")
    assert (tmp_path / "e.txt").read_text() == "0 0\n" and empty.total == 0
    with pytest.raises(mhap_amd.MhapError):
        empty.write(tmp_path / "no_such_dir" / "x.txt")
