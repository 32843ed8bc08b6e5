"""The GPU k-mer counter (kmer_kernels.hip, mhap_kmer_count_*) at its edges, each file byte for byte against a plain string counter:
every k from 1 to 16 (the three bucket layouts of kmer_low_bits: one counter per bucket at k <= 4, 256 buckets at k = 5..11, 2^15
counters per bucket at k >= 12), a flush before every group (the kept room's 2^L clip), more reads than the hist kernels' 32 768
waves and more than the 2^21 reads of one add_reads group, one bucket holding nearly every window (counts past 2^16 and 2^24), the
line threshold at a count's exact fraction, the streamed scan path at small k, the filter in use at k != 16 and the CLI."""
import collections
import itertools
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import mhap_amd
from mhap_amd import FastaData, MhapParams, MinHashSearch
from mhap_amd import workloads as W
from test_kmer_count import KMERS_CLI, ROOT, _CHILD, _awkward_fasta, _mixed_reads

_RC = str.maketrans("ACGT", "TGCA")
_ACGT = np.frombuffer(b"ACGT", np.uint8)
KC_THREADS, MHAP_WAVE, HIST_GRID_CAP = 256, 64, 8192
MAX_WAVES = HIST_GRID_CAP * KC_THREADS // MHAP_WAVE        # kmer_hist_kernel: 32 768 waves at most; further reads are strided
GROUP_READS = 1 << 21                                      # mhap_kmer_count_add_reads: at most 2^21 reads per group
_FLUSH = re.compile(r"\[kmer\] flush (\d+): (\d+) groups, (\d+) windows, (\d+) kept entries of room")


# ---- the reference: a plain string counter --------------------------------------------------------------------------------------

def _revcomp(s):
    return s.translate(_RC)[::-1]


def _ref_counter(seqs, k, canonical, cnt=None):
    """Every window of k bytes that are all A/C/G/T (upper case), keyed by its string (canonical: min(s, revcomp(s)))."""
    cnt = collections.Counter() if cnt is None else cnt
    for seq in seqs:
        for m in re.finditer(r"[ACGT]{%d,}" % k, seq):
            run = m.group()
            n = len(run) - k + 1
            if canonical:
                rc = _revcomp(run)
                L = len(run)
                cnt.update(min(run[i:i + k], rc[L - k - i:L - i]) for i in range(n))
            else:
                cnt.update(run[i:i + k] for i in range(n))
    return cnt


def _periodic_counter(unit, length, nreads, k, canonical, cnt=None):
    """Closed form for nreads reads of `length` bases repeating `unit` from its first base: window i starts at phase i mod p."""
    cnt = collections.Counter() if cnt is None else cnt
    p, nw = len(unit), length - k + 1
    text = unit * ((k + p) // p + 1)
    for j in range(min(p, nw)):
        w = text[j:j + k]
        cnt[min(w, _revcomp(w)) if canonical else w] += nreads * ((nw - j + p - 1) // p)
    return cnt


def _expected(cnt, mf):
    """The `-f` file: "<distinct> <lines>", then the k-mers with c / T >= mf by count descending, k-mer ascending, "%.10e" fractions."""
    T = sum(cnt.values())
    keep = sorted(((c, km) for km, c in cnt.items() if c / T >= mf), key=lambda t: (-t[0], t[1])) if T else []
    return "".join([f"{len(cnt)} {len(keep)}\n"] + [f"{km}\t{c / T:.10e}\n" for c, km in keep]).encode()


def _check(kc, cnt, mf, path, what):
    kc.write(path)
    got, want = path.read_bytes(), _expected(cnt, mf)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        i = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        pytest.fail(f"{what}: files differ at line {i}: got {g[i:i + 3]} want {w[i:i + 3]} ({len(g)} vs {len(w)} lines)")
    assert (kc.total, kc.distinct, len(kc)) == (sum(cnt.values()), len(cnt), want.count(b"\n") - 1), what


def _fasta(seqs):
    """FastaData of the strings as they are (no upper-casing: lower-case bytes stay and do not count)."""
    raw = [s.encode("latin-1") for s in seqs]
    lengths = np.array([len(b) for b in raw], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]) if raw else np.zeros(0, np.int64)
    bases = np.frombuffer(b"".join(raw), np.uint8) if raw else np.zeros(0, np.uint8)
    return FastaData(bases, offsets, lengths, np.arange(1, len(raw) + 1, dtype=np.int64))


def _seqs(fa):
    return [fa.sequence(i) for i in range(len(fa))]


def _rand(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def _count(ms, parts, k, canonical, mf):
    ms.kmer_count_begin(k, canonical)
    for fa in parts:
        ms.kmer_count_add(fa)
    return ms.kmer_count_finish(mf)


def _handle():
    return MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=0))


def _de_bruijn(k):
    """A linear de Bruijn sequence of order k over ACGT: every one of the 4^k k-mers occurs exactly once in its 4^k + k - 1 bases."""
    a, seq = [0] * (4 * k + 1), []

    def db(t, p):
        if t > k:
            if k % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    s = "".join("ACGT"[c] for c in seq)
    return s + s[:k - 1]


def _lane_reads(k, rnd):
    """Reads whose windows divide across the 64 lanes of a wave in different ways (nw = 1, 63, 64, 65, 129: packed, and raw with a
    trailing N), N runs that start or end exactly where a lane's chunk of windows starts, and (even k) palindromes."""
    out = []
    for nw in (1, 63, 64, 65, 129):
        out.append(_rand(rnd, nw + k - 1))
        out.append(_rand(rnd, nw + k - 2) + "N")
    nw, chunk = 64 * 7, 7
    for lane in (1, 5, 31, 63):
        s0 = lane * chunk                                          # first window (and first base) of the lane's share
        for a, b in ((s0, s0 + 3), (s0 - 3, s0), (s0 + k - 1, s0 + k), (s0 - 1, s0 + k - 1)):
            s = list(_rand(rnd, nw + k - 1))
            s[max(a, 0):b] = "N" * (b - max(a, 0))
            out.append("".join(s))
    if k % 2 == 0:
        half = _rand(rnd, k // 2)
        pal = half + _revcomp(half)
        out += [pal, pal * 5, _rand(rnd, 70) + pal + _rand(rnd, 3) + pal]
    return out


# ---- 1. every k, every layout ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_every_k_matches_a_string_counter(tmp_path):
    base = _seqs(_mixed_reads())
    assert sum(1 for s in base if not re.fullmatch(r"[ACGT]*", s)) >= 3   # raw reads with the packed ones in one group
    with _handle() as ms:
        for k in range(1, 17):
            seqs = base + _lane_reads(k, random.Random(70 + k))
            fa = _fasta(seqs)
            halves = [fa.subset(np.arange(0, len(fa) // 2)), fa.subset(np.arange(len(fa) // 2, len(fa)))]
            for canonical in (True, False):
                cnt = _ref_counter(seqs, k, canonical)
                for mf in (0.0, 1e-4):
                    kc = _count(ms, halves, k, canonical, mf)
                    _check(kc, cnt, mf, tmp_path / "got.txt", (k, canonical, mf))
                if not canonical:                                    # the numpy counter agrees too (it shares the 2-bit values)
                    u, c, total = W.count_kmers(fa, k, False, max_reads=None)
                    assert total == sum(cnt.values()) and len(u) == len(cnt)


# ---- 2. a flush before every group ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 11, 12, 16])
def test_a_flush_before_every_group(tmp_path, monkeypatch, capfd, k):
    monkeypatch.setenv("MHAP_KMER_STAGE_WINDOWS", "1")             # read at begin: every group after the first flushes the staged ones
    monkeypatch.setenv("MHAP_HOST_PROF", "1")
    rnd = random.Random(300 + k)
    calls = []
    for c in range(5):
        seqs = [_rand(rnd, rnd.randint(k, 400)) for _ in range(6)] + [_rand(rnd, 200, "ACGTN")]
        if k <= 5:
            seqs.append(_de_bruijn(k))                             # all 4^k k-mers in every call
        calls.append(seqs)
    if k <= 5:
        assert len(_de_bruijn(k)) == 4 ** k + k - 1 and len(_ref_counter([_de_bruijn(k)], k, False)) == 4 ** k
    with _handle() as ms:
        for canonical in (True, False):
            cnt = collections.Counter()
            for seqs in calls:
                _ref_counter(seqs, k, canonical, cnt)
            capfd.readouterr()
            kc = _count(ms, [_fasta(s) for s in calls], k, canonical, 0.0)
            err = capfd.readouterr().err
            _check(kc, cnt, 0.0, tmp_path / "got.txt", (k, canonical))
            flushes = [tuple(map(int, m)) for m in _FLUSH.findall(err)]
            assert [f[0] for f in flushes] == list(range(len(calls) - 1)), err
            for i, (_, groups, windows, room) in enumerate(flushes):
                assert groups == 1 and windows == sum(_ref_counter(calls[i], k, canonical).values()), (i, err)
                if not canonical and k <= 5:
                    # every bucket holds all 2^L of its values from the first call on, so min(kept_n + flush_n, 2^L) sums to 4^k;
                    # without the clip the room would be 4^k + the call's windows
                    assert room == 4 ** k, (i, room, err)


# ---- 3. the hist kernels' read stride and add_reads' group split ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_more_reads_than_waves(tmp_path):
    rnd = np.random.default_rng(41)
    n = 40_000
    assert n > MAX_WAVES                                           # waves 0 .. n - MAX_WAVES - 1 walk two reads
    lengths = rnd.integers(1, 61, n).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)])
    bases = _ACGT[rnd.integers(0, 4, int(lengths.sum()))]
    bases[rnd.integers(0, len(bases), 2000)] = ord("N")
    fa = FastaData(bases, offsets, lengths, np.arange(1, n + 1, dtype=np.int64))
    text = bases.tobytes().decode("latin-1")
    seqs = [text[o:o + L] for o, L in zip(offsets.tolist(), lengths.tolist())]
    with _handle() as ms:
        for k in (4, 9, 16):
            for canonical in (True, False):
                cnt = _ref_counter(seqs, k, canonical)
                kc = _count(ms, [fa], k, canonical, 0.0)
                _check(kc, cnt, 0.0, tmp_path / "got.txt", (k, canonical))
                assert kc.total > 0


def _matrix_counts(codes, k, canonical):
    """Vectorised counter over an (n, L) matrix of 2-bit codes (equal-length reads of A/C/G/T only): counts indexed by value."""
    n, L = codes.shape
    nw = L - k + 1
    v = np.zeros((n, nw), np.uint32)
    r = np.zeros((n, nw), np.uint32)
    for j in range(k):
        c = codes[:, j:j + nw].astype(np.uint32)
        v = (v << np.uint32(2)) | c
        r |= (np.uint32(3) - c) << np.uint32(2 * j)
    if canonical:
        v = np.minimum(v, r)
    return np.bincount(v.ravel(), minlength=1 << (2 * k))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_more_reads_than_one_add_reads_group(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("MHAP_KMER_STAGE_WINDOWS", "1")             # the second group flushes the first: the flush line shows the split
    monkeypatch.setenv("MHAP_HOST_PROF", "1")
    n, L, k = GROUP_READS + 5, 24, 8
    assert GROUP_READS // MAX_WAVES == 64                          # in the first group every wave walks 64 reads
    codes = np.random.default_rng(2021).integers(0, 4, (n, L)).astype(np.uint8)
    fa = FastaData(_ACGT[codes].ravel(), np.arange(n, dtype=np.int64) * L, np.full(n, L, np.int32), np.arange(1, n + 1, dtype=np.int64))
    names = ["".join(t) for t in itertools.product("ACGT", repeat=k)]
    with _handle() as ms:
        for canonical in (True, False):
            counts = _matrix_counts(codes, k, canonical)
            cnt = collections.Counter({names[i]: int(counts[i]) for i in np.nonzero(counts)[0].tolist()})
            capfd.readouterr()
            kc = _count(ms, [fa], k, canonical, 0.0)
            err = capfd.readouterr().err
            _check(kc, cnt, 0.0, tmp_path / "got.txt", canonical)
            assert kc.total == n * (L - k + 1)
            # one flush, of the first group alone; its room is clipped: every bucket of 2^L = 256 values holds far more windows
            flush_n = _matrix_counts(codes[:GROUP_READS], k, canonical).reshape(-1, 1 << 8).sum(axis=1)
            room = int(np.minimum(flush_n, 1 << 8).sum())
            assert int(flush_n.sum()) > room
            assert _FLUSH.findall(err) == [("0", "1", str(GROUP_READS * (L - k + 1)), str(room))], err


# ---- 4. one heavy bucket ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [2, 7, 16])
def test_homopolymers_and_tandem_repeats(tmp_path, k):
    rnd = random.Random(500 + k)
    nA, LA = 4096, 4296
    assert nA * (LA - 16 + 1) > 1 << 24                            # more than 2^24 windows of one k-mer at every k here
    polyA = _fasta(["A" * LA] * nA)
    rep = [("ACGT", 3000, 200), ("AC", 3001, 200)]
    rep_fa = [_fasta([u * (L // len(u)) + u[:L % len(u)]] * m) for u, L, m in rep]
    randoms = [_rand(rnd, 1000) for _ in range(300)]
    with _handle() as ms:
        for canonical in (True, False):
            cnt = _periodic_counter("A", LA, nA, k, canonical)
            assert len(cnt) == 1
            kc = _count(ms, [polyA], k, canonical, 1.0)
            _check(kc, cnt, 1.0, tmp_path / "a.txt", ("polyA", k, canonical))
            assert (tmp_path / "a.txt").read_text() == f"1 1\n{'A' * k}\t1.0000000000e+00\n"
            assert int(kc.counts[0]) == nA * (LA - k + 1) > 1 << 24

            both = collections.Counter()
            for (u, L, m), fa in zip(rep, rep_fa):
                cnt = _periodic_counter(u, L, m, k, canonical)
                assert 2 <= len(cnt) <= 4 and min(cnt.values()) > 1 << 16, cnt
                _check(_count(ms, [fa], k, canonical, 0.0), cnt, 0.0, tmp_path / "r.txt", (u, k, canonical))
                both += cnt

            mixed = both + _ref_counter(randoms, k, canonical) + _periodic_counter("A", LA, 8, k, canonical)
            parts = [rep_fa[0], _fasta(randoms[:150]), polyA.subset(np.arange(8)), rep_fa[1], _fasta(randoms[150:])]
            for mf in (0.0, 1e-3):                                   # a few heavy buckets, the others sparse
                _check(_count(ms, parts, k, canonical, mf), mixed, mf, tmp_path / "m.txt", ("mixed", k, canonical, mf))


# ---- 5. the line threshold at a count's exact fraction --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_line_threshold_edges(tmp_path):
    seqs = _seqs(_mixed_reads())
    fa = _fasta(seqs)
    k, found = None, None
    for k in (6, 5, 7, 8, 4):
        cnt = _ref_counter(seqs, k, True)
        T = sum(cnt.values())
        # a present count c whose fraction, times T, rounds up past c: a plain ceil(mf * T) would drop the count-c lines
        found = next((c for c in sorted(set(cnt.values())) if math.ceil((c / T) * T) == c + 1), None)
        if found:
            break
    assert found, "no count on a rounding edge in the corpus"
    c, f = found, found / T
    with _handle() as ms:
        for mf, written in ((f, True), (math.nextafter(f, math.inf), False), (math.nextafter(f, -math.inf), True)):
            kc = _count(ms, [fa], k, True, mf)
            _check(kc, cnt, mf, tmp_path / "t.txt", (k, c, T, mf))
            assert (c in kc.counts.tolist()) == written, (k, c, T, mf)
            assert (len(kc) > 0 and int(kc.counts.min()) == c) == written
        for mf in (0.0, -0.0, -1.0, -math.inf, 5e-324):
            kc = _count(ms, [fa], k, True, mf)
            _check(kc, cnt, mf, tmp_path / "t.txt", (k, mf))
            assert len(kc) == len(cnt)
        kc = _count(ms, [fa], k, True, math.inf)
        _check(kc, cnt, math.inf, tmp_path / "t.txt", (k, "inf"))
        assert (tmp_path / "t.txt").read_text() == f"{len(cnt)} 0\n"
        one = _fasta(["A" * 40, "T" * 25])                         # canonical: one k-mer
        kc = _count(ms, [one], k, True, 1.0)
        _check(kc, _ref_counter(["A" * 40, "T" * 25], k, True), 1.0, tmp_path / "t.txt", (k, "one"))
        assert (tmp_path / "t.txt").read_text() == f"1 1\n{'A' * k}\t1.0000000000e+00\n"
        ms.kmer_count_begin(k, True)
        ms.kmer_count_add(fa)
        with pytest.raises(mhap_amd.MhapError, match="NaN"):
            ms.kmer_count_finish(float("nan"))


# ---- 6. the streamed scan path at small k ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [4, 7, 11])
def test_scan_path_at_small_k(tmp_path, k):
    path = tmp_path / "reads.fasta.gz"
    seqs = [s.upper() for s in _awkward_fasta(str(path))]
    for canonical in (True, False):
        cnt = _ref_counter(seqs, k, canonical)
        out = tmp_path / f"k{int(canonical)}.txt"
        env = dict(os.environ, MHAP_INGEST_GROUP_BASES="6000", MHAP_KMER_STAGE_WINDOWS="15000", MHAP_HOST_PROF="1",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", _CHILD, str(path), str(out), str(k), "1" if canonical else "0"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stderr.count("[ingest] group") >= 10, r.stderr[-3000:]
        assert r.stderr.count("[kmer] flush") >= 2, r.stderr[-3000:]
        assert out.read_bytes() == _expected(cnt, 0.0), (k, canonical)
        T = sum(cnt.values())
        assert r.stdout.split() == [str(T), str(len(cnt)), str(len(cnt))]


# ---- 7. the filter in use at k != 16 --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [12, 14])
def test_the_filter_in_use_at_other_k(tmp_path, k):
    fa = mhap_amd.synth_reads(150, 3000, seed=404, error_rate=0.05, repeats=(300, 1500, 0.01))
    kc = mhap_amd.count_kmers(fa, k=k, canonical=True, min_fraction=1e-5)
    _check(kc, _ref_counter(_seqs(fa), k, True), 1e-5, tmp_path / "kmers.txt", k)
    assert len(kc) > 100 and kc.distinct > len(kc)
    mem = mhap_amd.FrequencyCounts.from_counts(kc, filter_cutoff=1e-5, repeat_weight=0.9)
    fil = mhap_amd.FrequencyCounts.from_file(str(tmp_path / "kmers.txt"), filter_cutoff=1e-5, repeat_weight=0.9)
    for a in ("hashes", "fractions", "whitelist"):
        assert getattr(mem, a).tobytes() == getattr(fil, a).tobytes(), a
    assert mem.size_bloom == fil.size_bloom == kc.distinct
    p = MhapParams(kmer_size=k, num_hashes=128, ordered_sketch_size=512, device=0)

    def records(flt):
        with MinHashSearch(p, kmer_filter=flt) as ms:
            ms.add_data(fa)
            return sorted(mhap_amd.records_to_lines(ms.find_matches()))
    got, plain = records(mem), records(None)
    oflt = O.Filter(fil.hashes, fil.fractions, 1e-5, 0.9, 3.0, False)
    want = O.record_lines(O.run_self(fa, k=k, H=128, S=512, nthreads=8, flt=oflt)["records"])
    assert got == want and len(want) > 50
    assert plain != want                                             # the filter changes the records


# ---- 8. the CLI -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_cli_at_k7_without_reverse_complements(tmp_path):
    seqs = _seqs(_mixed_reads())
    fasta = tmp_path / "r.fasta"
    fasta.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs)))
    out = tmp_path / "cli.txt"
    r = subprocess.run([KMERS_CLI, "-o", str(out), "-k", "7", "--no-rc", "--min-fraction", "0", str(fasta)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    api_file = tmp_path / "api.txt"
    kc = mhap_amd.count_kmers(str(fasta), k=7, canonical=False, min_fraction=0.0)
    _check(kc, _ref_counter([s.upper() for s in seqs], 7, False), 0.0, api_file, "api")
    assert out.read_bytes() == api_file.read_bytes()
