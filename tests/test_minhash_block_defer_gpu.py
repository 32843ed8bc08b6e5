"""Block-deferred candidates of the weight-1 MinHash kernel (minhash_w1_kernel: w1_row2 / w1_enqueue / w1_flush2) against the oracle.

The slot loops queue one entry per lane and SUB-BLOCK of slots (MH_W1_DEFER_BLOCK, 8 in the shipped library) and the drain walks an entry's
chain through the sub-block.  What can go wrong is at the edges: a sketch shorter than a sub-block (H = 3), a last sub-block cut by H (13, 33,
100), a last 64-slot class block cut by H (33, 100), whole class blocks (16, 512), and the queue window that grows with H (1 024).  Rows: a
strand of one k-mer, one short of / exactly / one past a lane row (63, 64, 65) and a 2 048-k-mer row (2 047, 2 048, 2 049, 4 096, 4 097), and
four rows.  On the full grid every strand is cut into row items (first rows and seeded rows); on two CUs most strands are taken whole (later
rows with the class filters).  A read with a tandem repeat puts a weighted launch next to the weight-1 one.
"""
import random

import pytest

from mhap_amd import FastaData, MhapParams
from test_kernel_variants_gpu import _assert_path, _sketch
from test_small_grids_gpu import _expected_sketches, _rand_seq, _sketch_mismatches, _w1_reads

pytestmark = pytest.mark.gpu

K = 16
EDGE_KMERS = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 6200)
_corpus = []


def _reads():
    if not _corpus:
        rnd = random.Random(40608)
        seqs = []
        for nk in EDGE_KMERS:
            seqs += _w1_reads(rnd, [nk + K - 1])
            seqs += _w1_reads(rnd, [rnd.randrange(120, 900) for _ in range(14)])
        unit = _rand_seq(rnd, 40)
        seqs.append(_rand_seq(rnd, 700) + unit * 5 + _rand_seq(rnd, 600))
        _corpus.append(FastaData.from_strings(seqs))
    return _corpus[0]


@pytest.mark.parametrize("H", [3, 13, 16, 33, 100, 512, 1024])
def test_block_deferred_rows_equal_the_oracle(H, monkeypatch, capfd):
    fa = _reads()
    assert len(fa) == 15 * len(EDGE_KMERS) + 1
    p = MhapParams(kmer_size=K, num_hashes=H, ordered_sketch_size=64, min_olap_length=0)
    exp = _expected_sketches(fa, p)            # the oracle's rows and statuses at this H, shared by the two grids
    for cap in (None, 2):
        sk, wit = _sketch(monkeypatch, capfd, fa, p, {"MHAP_NUM_CUS": cap} if cap else {})
        bad = _sketch_mismatches(fa, p, sk, exp)
        assert not bad, f"H {H}, cap {cap}: {len(bad)} strands differ from the oracle, first {bad[:8]}"
        _assert_path(wit, "default")
        assert len(wit) == 1 and wit[0]["path"] == "w1" and wit[0]["weighted_n"] > 0, wit
        assert wit[0]["rmax"] == 4, wit
        # full grid: more resident waves than strands, every strand goes row by row; two CUs: at most 64 strands do
        assert (wit[0]["n_whole"] > 0) == (cap == 2) and wit[0]["n_tail"] > 0, (cap, wit)
