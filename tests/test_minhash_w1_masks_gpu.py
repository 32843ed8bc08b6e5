"""Scalar class masks of the weight-1 MinHash kernel (minhash_w1_kernel: w1_class_block, MH_W1_CLS 4) against the oracle.

A later row selects each slot's filter code by testing the slot's bit in wave-uniform class masks built once per 64-slot class block, and finds
a class-0 slot (the exact filter) by the number of the block's next one.  What can go wrong is at the edges, hence the sketch sizes: shorter
than a sub-block (3), a sub-block cut by H (7, 9, 13, 33, 65), exactly two sub-blocks (8), a class block cut by H (33, 100), exactly one block
and one slot either side of it (63, 64, 65: the masks' bit 63, and bit 0 of the next block's), whole blocks (16, 512) and the queue window that
grows with H (1 024).  Rows: a strand of one k-mer, one short of / exactly / one past a lane row (63, 64, 65) and a 2 048-k-mer row (2 047,
2 048, 2 049, 4 096, 4 097), and four rows.  On the full grid every strand is cut into row items (first rows and seeded rows); on two CUs the
long strands are taken whole (later rows with the class chain).  A read with a tandem repeat puts a weighted launch next to the weight-1 one.

Two variant builds (mhap_amd/build.py VARIANTS) run the same comparison in a child process, the library path being fixed at import:
  * w1cls0: every seventh slot is class 0, so the exact filter — otherwise one step in a thousand — runs nine or ten times in every class
    block of every later row, between steps of the class chain, and the next-class-0 slot number is advanced each time.  The exact filter is
    a superset of the class's: the rows must not change.
  * qcap64: a queue window of 64 words = 31 entries.  At H = 512 every full row overflows on its count and its strand is redone exactly; at
    H = 16 and 13 a first row queues about 30 entries, a later row fewer: the count often fits and the re-queued rests of multi-chain masks
    run over, which is reported so that the strand is redone.
"""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

from mhap_amd import FastaData, MhapParams, MinHashSearch
from test_kernel_variants_gpu import MINHASH_SWITCHES, _assert_path, _minhash_witness, _sketch
from test_small_grids_gpu import _expected_sketches, _rand_seq, _sketch_mismatches, _w1_reads

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
K = 16
EDGE_KMERS = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 6200)
ALL_H = (3, 7, 8, 9, 13, 16, 33, 63, 64, 65, 100, 512, 1024)
FILL = 6          # short reads between the edge reads: with them two CUs (at most 64 row-item strands) take the long strands whole
CAPS = (None, 2)  # MHAP_NUM_CUS: the full grid, two CUs
_corpus = []


def _reads():
    if not _corpus:
        rnd = random.Random(51217)
        seqs = []
        for nk in EDGE_KMERS:
            seqs += _w1_reads(rnd, [nk + K - 1])
            seqs += _w1_reads(rnd, [rnd.randrange(120, 900) for _ in range(FILL)])
        unit = _rand_seq(rnd, 40)
        seqs.append(_rand_seq(rnd, 700) + unit * 5 + _rand_seq(rnd, 600))
        _corpus.append(FastaData.from_strings(seqs))
    return _corpus[0]


def _params(H):
    return MhapParams(kmer_size=K, num_hashes=H, ordered_sketch_size=64, min_olap_length=0)


def _assert_launch(wit, cap):
    """One launch, the weight-1 kernel beside a weighted one; row items only on the full grid, whole strands too on two CUs."""
    _assert_path(wit, "default")
    assert len(wit) == 1 and wit[0]["path"] == "w1" and wit[0]["weighted_n"] > 0, wit
    assert wit[0]["rmax"] == 4, wit
    assert (wit[0]["n_whole"] > 0) == (cap == 2) and wit[0]["n_tail"] > 0, (cap, wit)


@pytest.mark.parametrize("H", ALL_H)
def test_rows_equal_the_oracle(H, monkeypatch, capfd):
    fa = _reads()
    assert len(fa) == (1 + FILL) * len(EDGE_KMERS) + 1
    p = _params(H)
    exp = _expected_sketches(fa, p)            # the oracle's rows and statuses at this H, shared by the two grids
    for cap in CAPS:
        sk, wit = _sketch(monkeypatch, capfd, fa, p, {"MHAP_NUM_CUS": cap} if cap else {})
        bad = _sketch_mismatches(fa, p, sk, exp)
        assert not bad, f"H {H}, cap {cap}: {len(bad)} strands differ from the oracle, first {bad[:8]}"
        _assert_launch(wit, cap)


# ---- the variant builds, each (variant, H) in a child process of its own ---------------------------------------------------------------
def _child_main(variant, H):
    """Runs in the child on the variant build: both grids against the oracle; the witness lines go to stderr behind a `[case]` line each."""
    import mhap_amd
    assert mhap_amd.api._LIB_PATH.endswith(f"libmhaphip_{variant}.so"), mhap_amd.api._LIB_PATH
    fa, p = _reads(), _params(H)
    exp = _expected_sketches(fa, p)
    os.environ["MHAP_HOST_PROF"] = "1"
    bad = {}
    for cap in CAPS:
        for k in MINHASH_SWITCHES:
            os.environ.pop(k, None)
        if cap:
            os.environ["MHAP_NUM_CUS"] = str(cap)
        sys.stderr.write(f"[case] cap {cap or 0}\n")
        sys.stderr.flush()
        with MinHashSearch(p) as ms:
            sk = ms.sketch(fa)
        bad[str(cap or 0)] = _sketch_mismatches(fa, p, sk, exp)
    print("BAD " + json.dumps(bad))


class _Err:
    """What _minhash_witness reads its lines from."""
    def __init__(self, text):
        self.text = text

    def readouterr(self):
        return "", self.text


@functools.lru_cache(maxsize=None)
def _run_child(variant, H):
    """({cap: mismatching strands}, {cap: witness}) of one child."""
    from mhap_amd import build as B
    lib = B.variant_path(variant)
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() builds it (python -m mhap_amd.build --variants)"
    env = dict(os.environ, MHAP_LIB_PATH=lib, PYTHONPATH=os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")]))
    for k in MINHASH_SWITCHES + ("MHAP_HOST_PROF",):
        env.pop(k, None)
    code = f"import test_minhash_w1_masks_gpu as T; T._child_main({variant!r}, {H})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-4000:] + r.stderr[-4000:])
    bad = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("BAD "))[4:])
    parts = r.stderr.split("[case] cap ")[1:]
    wit = {int(x.split("\n", 1)[0]): _minhash_witness(_Err(x)) for x in parts}
    return {int(c): b for c, b in bad.items()}, wit


def _assert_child(variant, H):
    bad, wit = _run_child(variant, H)
    for cap in CAPS:
        b = bad[cap or 0]
        assert not b, f"{variant}, H {H}, cap {cap}: {len(b)} strands differ from the oracle, first {b[:8]}"
        _assert_launch(wit[cap or 0], cap)


@pytest.mark.parametrize("H", ALL_H)
def test_class0_in_every_block_rows_equal_the_oracle(H):
    _assert_child("w1cls0", H)


@pytest.mark.parametrize("H", [512, 16, 13])
def test_small_queue_rows_equal_the_oracle(H):
    _assert_child("qcap64", H)
