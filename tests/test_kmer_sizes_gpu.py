"""Sketching and search at k-mer sizes over the whole accepted range, 1 to 255, against the oracle.

Away from (k, k2) = (16, 12) hash_kmers_kernel<0, 0> hashes every strand from chars in LDS (HASH_TILE window starts plus a halo of
max(k, k2) - 1 chars), every strand is MHAP_RD_MAT with separate strides for the key and the 32-bit hash arrays, and the weight, MinHash and
ordered kernels read those arrays instead of recomputing hashes from 2-bit codes.  The cases here cover every tail length and block count of
the 128-bit hash, k2 > k as well as k > k2, lengths at the zero-window and tile edges, and the search at sixteen (k, k2).  Every case
compares with the oracle itself; the [minhash] witness line (MHAP_HOST_PROF) shows which kernels a case ran."""
import functools
import random

import numpy as np
import pytest

import mhap_amd
import oracle_lib as O
from mhap_amd import FastaData, MhapParams
from test_gpu_parity import _assert_sketch_parity, _rand_seq, _self_lines
from test_kernel_variants_gpu import MINHASH_SWITCHES, _assert_path, _env, _minhash_witness

pytestmark = pytest.mark.gpu

TILE_EDGES = (1023, 1024, 1025, 2047, 2048, 2049)      # windows: one below, at and one above one and two HASH_TILEs
IUPAC = "ACGT" * 12 + "RYKMBDHVSWN"                     # mostly bases, a fifth ambiguity codes: a raw-byte read that still repeats short k-mers

# k: every tail length (k mod 8) of the 128-bit hash with 0, 1, 2, 3, 4, 7, 8, 15, 16 and 31 whole blocks; k2 goes round a cycle offset
# against it, so that k2 > k in ten cases and k > k2 in sixteen.
_KS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 17, 18, 19, 20, 22, 23, 31, 32, 33, 63, 64, 65, 127, 128, 254, 255)
_K2_CYCLE = (1, 2, 3, 4, 5, 6, 7, 9, 31, 32, 33, 64, 255)
RANGE_PAIRS = [(k, _K2_CYCLE[(i + 8) % len(_K2_CYCLE)]) for i, k in enumerate(_KS)]
MIXED_PAIRS = [(16, 13), (16, 11), (15, 12), (17, 12), (16, 255), (255, 12)]   # half on the conditions of the k = 16 / k2 = 12 fast path
assert sum(k2 > k for k, k2 in RANGE_PAIRS) >= 8 and sum(k > k2 for k, k2 in RANGE_PAIRS) >= 8
assert {k % 8 for k in _KS} == set(range(8))


def _corpus(k, k2):
    """At most 26 reads built from k and k2: lengths one below, at and one above min(k, k2) and max(k, k2) (a read with MinHash windows and no
    ordered ones, or the reverse; length 0 left out), 1 023 ... 2 049 windows of k and of k2, a raw-byte read over ACGTN and one with IUPAC
    codes at tile-edge lengths, a homopolymer, a tandem repeat, and four random reads."""
    rnd = random.Random(1000 * k + k2)
    lo, hi = min(k, k2), max(k, k2)
    lens = []
    for n in [lo - 1, lo, lo + 1, hi - 1, hi, hi + 1] + [w + kk - 1 for kk in (k, k2) for w in TILE_EDGES]:
        if n >= 1 and n not in lens:
            lens.append(n)
    seqs = [_rand_seq(rnd, n) for n in lens]
    seqs += [_rand_seq(rnd, 1025 + k - 1, "ACGTN"), _rand_seq(rnd, 2047 + k2 - 1, IUPAC)]
    seqs += ["A" * 1500, "ACGTTGCA" * 200]
    seqs += [_rand_seq(rnd, n) for n in (300, 811, 1500, 2500)]
    assert len(seqs) <= 40
    return FastaData.from_strings(seqs)


def _strand_classes(fa, k):
    """From the oracle's k-mer hashes: per strand 'none' (no window), 'w1' (every k-mer once) or 'weighted' (some k-mer repeats)."""
    out = []
    for i in range(len(fa)):
        seq = fa.sequence(i)
        for s in (seq, O.rc(seq)):
            h = O.kmer_hashes64(s, k)
            out.append("none" if len(s) < k else "w1" if len(np.unique(h)) == len(h) else "weighted")
    return out


def _parity_with_witness(fa, p, monkeypatch, capfd, env, flt=None, oflt=None):
    """_assert_sketch_parity under the MinHash switches of `env`, and the [minhash] witness lines of its launches."""
    _env(monkeypatch, MINHASH_SWITCHES, env)
    monkeypatch.setenv("MHAP_HOST_PROF", "1")
    capfd.readouterr()
    try:
        _assert_sketch_parity(fa, p, flt, oflt)
        return _minhash_witness(capfd)
    finally:
        _env(monkeypatch, MINHASH_SWITCHES + ("MHAP_HOST_PROF",), {})


def _assert_witness_counts(wit, fa, k):
    """The launches' weighted strands are exactly the strands in which the oracle finds a repeated k-mer, and every strand whose k-mers are
    all different is on the weight-1 list."""
    cls = _strand_classes(fa, k)
    assert sum(d["strands"] for d in wit) == 2 * len(fa), wit
    assert sum(d["weighted_n"] for d in wit) == cls.count("weighted"), (wit, cls.count("weighted"))
    assert sum(d["unweighted"] for d in wit) >= cls.count("w1"), (wit, cls.count("w1"))
    return cls


@pytest.mark.parametrize("k,k2", RANGE_PAIRS + MIXED_PAIRS)
def test_sketch_parity_over_the_kmer_size_range(k, k2, monkeypatch, capfd):
    """Status, MinHash row, ordered size and ordered rows of both strands of every read of _corpus(k, k2) equal the oracle's
    (MinHashSketch.java, BottomOverlapSketch.java) at H = 64, S = 300; one launch, whose witness shows the default kernels: with k >= 14 the
    random reads are weight-1 strands on the w1 path, with k <= 6 every read of 300 bases or more is a weighted strand."""
    fa = _corpus(k, k2)
    p = MhapParams(kmer_size=k, ordered_kmer_size=k2, num_hashes=64, ordered_sketch_size=300, min_olap_length=0)
    wit = _parity_with_witness(fa, p, monkeypatch, capfd, {})
    assert len(wit) == 1, wit
    _assert_path(wit, "default")
    cls = _assert_witness_counts(wit, fa, k)
    if k >= 14:
        assert cls.count("w1") >= 8 and wit[0]["path"] == "w1" and wit[0]["unweighted"] >= cls.count("w1"), wit
    if k <= 6:
        long_reads = [i for i in range(len(fa)) if fa.lengths[i] >= 300]
        assert all(cls[2 * i] == cls[2 * i + 1] == "weighted" for i in long_reads)            # (the corpus: no such read is weight-1)
        assert wit[0]["weighted_n"] >= 2 * len(long_reads) and wit[0]["weighted"] != "none", wit
        assert wit[0]["unweighted"] <= 2 * (len(fa) - len(long_reads)), wit


VARIANTS = {"batches": {"MHAP_BATCH_BASES": 3000}, "two_cus": {"MHAP_NUM_CUS": 2}, "classic": {"MHAP_MINHASH": "classic"},
            "perchain": {"MHAP_MINHASH": "perchain"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("k,k2", [(3, 255), (255, 3), (16, 13)])
def test_launch_groups_small_grids_and_minhash_variants_at_other_kmer_sizes(k, k2, variant, monkeypatch, capfd):
    """Three pairs again in launch groups of 3 000 bases (the scratch arrays are sized by plan_launch_groups' maxima, and the key and the
    32-bit totals differ), on two CUs (every persistent workgroup takes several strands), and through the classic and the per-chain MinHash
    kernels, which read the materialised hashes like the default ones: the sketches equal the oracle's, the witness shows the variant."""
    fa = _corpus(k, k2)
    p = MhapParams(kmer_size=k, ordered_kmer_size=k2, num_hashes=64, ordered_sketch_size=300, min_olap_length=0)
    wit = _parity_with_witness(fa, p, monkeypatch, capfd, VARIANTS[variant])
    _assert_path(wit, variant if variant in ("classic", "perchain") else "default")
    _assert_witness_counts(wit, fa, k)
    if variant == "batches":
        assert len(wit) >= 12, wit                   # (every read of a tile-edge length is a group of its own)
    else:
        assert len(wit) == 1, wit
    if variant == "two_cus":
        assert wit[0]["nblocks"] <= 16 and wit[0]["strands"] > wit[0]["nblocks"], wit


# ---- search ---------------------------------------------------------------------------------------------------------------------
SEARCH_CASES = [(1, 1, 64, 300), (2, 3, 64, 300), (4, 5, 64, 300), (8, 6, 64, 300), (10, 12, 128, 512), (11, 12, 128, 512), (16, 14, 128, 512),
                (19, 12, 128, 512), (12, 19, 128, 512), (22, 23, 128, 512), (32, 33, 128, 512), (63, 31, 128, 512), (64, 65, 128, 512),
                (127, 128, 128, 512), (254, 100, 128, 512), (255, 255, 128, 512)]
# 1 % error leaves the oracle 26 and 31 records at (254, 100) and (255, 255) (a window of 255 bases is error-free one time in thirteen);
# these two cases read the same genome at 0.5 %, where it has 414 and 391.
LOW_ERROR = {(254, 100), (255, 255)}


@functools.lru_cache(maxsize=None)
def _search_reads(error_rate):
    """120 reads of 2 000 bases from a 20 kb random genome, about half of them reverse-complemented, errors of all three kinds."""
    return mhap_amd.synth_reads(120, 2000, seed=255, coverage=12.0, error_rate=error_rate)


@pytest.mark.parametrize("k,k2,H,S,candidates", [c + ("index",) for c in SEARCH_CASES] + [(8, 6, 64, 300, "bruteforce"), (255, 255, 128, 512, "bruteforce")])
def test_search_records_over_the_kmer_size_range(k, k2, H, S, candidates, monkeypatch):
    """A self search at min_olap_length 100, threshold 0.78: the sorted records, the candidates compared and the strands indexed equal the
    oracle's.  The search side sees k2 through the metadata rows' ordered_seqlen and the identity table.  At (1, 1) every pair is a
    candidate and none reaches the threshold; every other case has at least 50 records."""
    fa = _search_reads(0.005 if (k, k2) in LOW_ERROR else 0.01)
    want = O.run_self(fa, k=k, H=H, k2=k2, S=S, min_olap_length=100, threshold=0.78, nthreads=8)
    want_lines = O.record_lines(want["records"])
    if (k, k2) == (1, 1):
        assert want_lines == [] and want["compared"] == 120 * 119
    else:
        assert len(want_lines) >= 50, len(want_lines)
    print(f"oracle: {len(want_lines)} records, {want['compared']} compared")
    monkeypatch.delenv("MHAP_CANDIDATES", raising=False)
    if candidates == "bruteforce":
        monkeypatch.setenv("MHAP_CANDIDATES", "bruteforce")
    p = MhapParams(kmer_size=k, ordered_kmer_size=k2, num_hashes=H, ordered_sketch_size=S, min_olap_length=100, threshold=0.78)
    lines, st = _self_lines(fa, p)
    monkeypatch.delenv("MHAP_CANDIDATES", raising=False)
    assert lines == want_lines, (len(lines), len(want_lines), sorted(set(want_lines) - set(lines))[:3], sorted(set(lines) - set(want_lines))[:3])
    assert st["candidates_compared"] == want["compared"]
    assert st["strands_indexed"] == want["strands"] == 240


# ---- the -f filter above the k-mer counter's k -----------------------------------------------------------------------------------
def test_kmer_filter_file_at_k_20(tmp_path):
    """A -f file of twelve 20-mers written by hand (the GPU counter stops at k = 16): six taken from forward reads, six from reverse
    complements, each spelled once as it stands and once as its reverse complement over the twelve lines; the loader hashes the canonical
    spelling (HashUtils.java:246-251), so each one is found on the strand that carries that spelling.  The sketches equal the oracle's
    under its Filter, which gives listed k-mers of both kinds a weight below the unlisted ones'."""
    k, k2 = 20, 12
    rnd = random.Random(2012)
    fa = FastaData.from_strings([_rand_seq(rnd, n) for n in (400, 1043, 1500, 2066, 900, 2500)] + ["ACGTTGCA" * 200])
    picked = []
    for j in range(12):
        seq = fa.sequence(j % 6)
        strand = seq if j < 6 else O.rc(seq)
        at = rnd.randrange(len(strand) - k + 1)
        kmer = strand[at:at + k]
        picked.append(kmer if j % 2 == 0 else O.rc(kmer))
    ffile = tmp_path / "kmers20.txt"
    with open(ffile, "w") as fh:
        fh.write(f"{len(picked)} {len(picked)}\n")
        for j, kmer in enumerate(picked):
            fh.write(f"{kmer}\t{2e-3 - 1e-4 * j:.10f}\n")           # all above the cutoff of 1e-5
    flt = mhap_amd.FrequencyCounts.from_file(str(ffile), filter_cutoff=1e-5, repeat_weight=0.9)
    assert len(flt.hashes) == 12 and len(set(flt.hashes.tolist())) == 12
    oflt = O.Filter(flt.hashes, flt.fractions, 1e-5, 0.9, 3.0, False)
    listed = [0, 0]
    for i in range(6):
        seq = fa.sequence(i)
        for strand, s in enumerate((seq, O.rc(seq))):
            listed[strand] += sum(1 for h in O.kmer_hashes64(s, k).tolist() if oflt.scaled_idf(h) < 3.0)   # (an unlisted k-mer: the full scale)
    assert listed[0] >= 3 and listed[1] >= 3, listed
    p = MhapParams(kmer_size=k, ordered_kmer_size=k2, num_hashes=64, ordered_sketch_size=300, min_olap_length=0)
    plain = [O.minhash(fa.sequence(i), k, 64)[1].tolist() for i in range(6)]
    assert any(O.minhash(fa.sequence(i), k, 64, 0.9, oflt)[1].tolist() != plain[i] for i in range(6))        # the filter changes sketches
    _assert_sketch_parity(fa, p, flt, oflt)
