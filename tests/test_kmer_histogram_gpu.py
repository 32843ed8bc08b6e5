"""The k-mer count histogram of the GPU counter (kmer_count_kernel<2>, mhap_kmer_count_finish_flags(MHAP_KMER_HISTOGRAM),
KmerCounts.histogram, mhap-hip-kmers --histogram) against np.unique over the counts of a CPU counter: every bucket layout of
kmer_low_bits, a flush before every group, single counts past the dense LDS range (2^16, 2^24), thousands of counts past it (the tail
list at and near its bound), raw reads and the scan path; with the histogram on, the lines and the `-f` file are those of the same
count without it; and the CLI's histogram file read by GetHistogramStats."""
import collections
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import histogram_stats_ref as R
import mhap_amd
from mhap_amd import FastaData, MhapError
from mhap_amd import workloads as W
from test_kmer_count import KMERS_CLI, ROOT, _awkward_fasta, _mixed_reads
from test_kmer_count_edges_gpu import _count, _de_bruijn, _fasta, _handle, _periodic_counter, _rand, _ref_counter

DENSE = 4096   # kmer_kernels.hip KC_HIST_DENSE: counts 1..DENSE binned in LDS, larger ones in the tail list


def _unique(counts):
    u, n = np.unique(np.asarray(list(counts), dtype=np.int64), return_counts=True)
    return u.tolist(), n.tolist()


def _check_hist(kc, counts, what):
    assert kc.histogram is not None, what
    hc, hn = kc.histogram
    assert hc.dtype == np.uint32 and hn.dtype == np.uint64, what
    assert (hc.tolist(), hn.tolist()) == _unique(counts), what
    assert sum(hn.tolist()) == kc.distinct, what
    assert sum(int(c) * int(n) for c, n in zip(hc.tolist(), hn.tolist())) == kc.total, what


def _finish_both(parts, k, canonical, mf, tmp_path):
    """The same count finished with and without the histogram: the lines and the `-f` file must not change."""
    with _handle() as ms:
        off = _count(ms, parts, k, canonical, mf)
        ms.kmer_count_begin(k, canonical)
        for fa in parts:
            ms.kmer_count_add(fa)
        on = ms.kmer_count_finish(mf, histogram=True)
    assert off.histogram is None
    with pytest.raises(MhapError):
        off.write_histogram(tmp_path / "none.txt")
    off.write(tmp_path / "off.txt")
    on.write(tmp_path / "on.txt")
    assert (tmp_path / "off.txt").read_bytes() == (tmp_path / "on.txt").read_bytes()
    assert on.kmers.tobytes() == off.kmers.tobytes() and on.counts.tobytes() == off.counts.tobytes()
    assert (on.total, on.distinct) == (off.total, off.distinct)
    return on


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 11, 12, 16])
def test_every_bucket_layout_matches_numpy(tmp_path, k):
    fa = _mixed_reads()                           # packed and raw reads (N runs, IUPAC codes, lower-case bytes), several add calls
    parts = [fa.subset(p) for p in np.array_split(np.arange(len(fa)), 3)]
    for canonical in (True, False):
        u, cnt, total = W.count_kmers(fa, k, canonical, max_reads=None)
        kc = _finish_both(parts, k, canonical, 2.5e-6, tmp_path)
        assert kc.total == total
        _check_hist(kc, cnt, (k, canonical))
        if k == 1:
            assert int(kc.histogram[0][-1]) > DENSE   # (counts past the dense range: the tail list at small k)


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [1, 4, 5, 11, 12, 16])
def test_a_flush_before_every_group_gives_the_same_histogram(tmp_path, monkeypatch, k):
    rnd = random.Random(700 + k)
    calls = [[_rand(rnd, rnd.randint(k, 500)) for _ in range(8)] + [_rand(rnd, 300, "ACGTN")] for _ in range(5)]
    if k <= 5:
        calls[2].append(_de_bruijn(k) * 3)
    parts = [_fasta(s) for s in calls]
    for canonical in (True, False):
        cnt = collections.Counter()
        for s in calls:
            _ref_counter(s, k, canonical, cnt)
        with _handle() as ms:
            ms.kmer_count_begin(k, canonical)
            for fa in parts:
                ms.kmer_count_add(fa)
            plain = ms.kmer_count_finish(0.0, histogram=True)
        monkeypatch.setenv("MHAP_KMER_STAGE_WINDOWS", "1")   # (read at begin: every group after the first flushes the staged ones)
        with _handle() as ms:
            ms.kmer_count_begin(k, canonical)
            for fa in parts:
                ms.kmer_count_add(fa)
            flushed = ms.kmer_count_finish(0.0, histogram=True)
        monkeypatch.delenv("MHAP_KMER_STAGE_WINDOWS")
        _check_hist(plain, cnt.values(), (k, canonical, "no flush"))
        _check_hist(flushed, cnt.values(), (k, canonical, "flushes"))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_single_counts_past_2_16_and_2_24(tmp_path):
    k = 16
    nA, LA = 4096, 4296
    polyA = _fasta(["A" * LA] * nA)
    small = _fasta(["C" * 2100] * 40)
    for canonical in (True, False):
        big = _finish_both([polyA], k, canonical, 1.0, tmp_path)
        assert big.histogram[0].tolist() == [nA * (LA - k + 1)] and big.histogram[1].tolist() == [1]
        assert nA * (LA - k + 1) > 1 << 24
        mid = _finish_both([small], k, canonical, 0.0, tmp_path)
        assert mid.histogram[0].tolist() == [40 * (2100 - k + 1)] and 40 * (2100 - k + 1) > 1 << 16
        rnd = random.Random(9)
        randoms = [_rand(rnd, 800) for _ in range(100)]
        mixed = _periodic_counter("A", LA, 8, k, canonical) + _periodic_counter("C", 2100, 40, k, canonical) + _ref_counter(randoms, k, canonical)
        kc = _finish_both([polyA.subset(np.arange(8)), small, _fasta(randoms)], k, canonical, 0.0, tmp_path)
        _check_hist(kc, mixed.values(), ("mixed", canonical))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_thousands_of_counts_past_the_dense_range(tmp_path):
    rnd = random.Random(2024)
    seg = _rand(rnd, 10000)
    copies = 5000
    noise = [_rand(rnd, 3000) for _ in range(200)]
    for canonical in (True, False):
        want = collections.Counter({km: c * copies for km, c in _ref_counter([seg], 16, canonical).items()})
        _ref_counter(noise, 16, canonical, want)
        kc = _finish_both([_fasta([seg] * copies), _fasta(noise)], 16, canonical, 2.5e-6, tmp_path)
        _check_hist(kc, want.values(), ("segment", canonical))
        tail = sum(n for c, n in zip(*kc.histogram) if c > DENSE)
        assert tail > 9000 and tail <= kc.total // (DENSE + 1)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_tail_list_exactly_at_its_bound(tmp_path):
    # every 6-mer exactly DENSE + 1 times: the tail holds total / (DENSE + 1) entries, its bound
    k, copies = 6, DENSE + 1
    seq = _de_bruijn(k)
    kc = _finish_both([_fasta([seq] * copies)], k, False, 0.0, tmp_path)
    assert kc.total == 4 ** k * copies
    assert kc.histogram[0].tolist() == [copies] and kc.histogram[1].tolist() == [4 ** k] == [kc.total // (DENSE + 1)]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_scan_path_on_an_awkward_fasta(tmp_path):
    path = tmp_path / "reads.fasta.gz"
    seqs = [s.upper() for s in _awkward_fasta(str(path))]   # (the ingest upper-cases a scanned file)
    for k in (7, 16):
        for canonical in (True, False):
            cnt = _ref_counter(seqs, k, canonical)
            kc = mhap_amd.count_kmers(str(path), k=k, canonical=canonical, min_fraction=0.0, histogram=True)
            _check_hist(kc, cnt.values(), (k, canonical))
            kc.write_histogram(tmp_path / "h.txt")
            u, n = _unique(cnt.values())
            assert (tmp_path / "h.txt").read_text() == "".join(f"{c}\t{m}\n" for c, m in zip(u, n))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cli_histogram_and_get_histogram_stats(tmp_path):
    fa = mhap_amd.synth_reads(150, 3000, seed=77, error_rate=0.05, repeats=(300, 1500, 0.01))
    fasta = tmp_path / "r.fasta"
    W.write_fasta(fa, str(fasta))
    f_h, f_plain, h = tmp_path / "f.txt", tmp_path / "f_plain.txt", tmp_path / "h.txt"
    r = subprocess.run([KMERS_CLI, "-o", str(f_h), "--min-fraction", "1e-5", "--histogram", str(h), str(fasta)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert len([l for l in r.stderr.split("\n") if l]) == 1 and "Counted" in r.stderr
    r = subprocess.run([KMERS_CLI, "-o", str(f_plain), "--min-fraction", "1e-5", str(fasta)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f_h.read_bytes() == f_plain.read_bytes()
    kc = mhap_amd.count_kmers(str(fasta), min_fraction=1e-5, histogram=True)
    kc.write_histogram(tmp_path / "api.txt")
    assert h.read_bytes() == (tmp_path / "api.txt").read_bytes()
    u, cnt, total = W.count_kmers(FastaData.from_file(str(fasta)), 16, True, max_reads=None)
    _check_hist(kc, cnt, "cli")
    hc, hn = _unique(cnt)
    want = R.to_string(*R.process(dict(zip(hc, hn)), 0.99))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    s = subprocess.run([sys.executable, "-m", "mhap_amd.histogram_stats", str(h), "0.99"], capture_output=True, text=True, env=env, timeout=300)
    assert (s.returncode, s.stdout, s.stderr) == (0, want + "\n", "")
    bad = subprocess.run([KMERS_CLI, "-o", str(tmp_path / "x.txt"), "--histogram", str(tmp_path / "no" / "h.txt"), str(fasta)],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1 and "cannot write" in bad.stderr and "h.txt" in bad.stderr
