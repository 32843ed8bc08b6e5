"""The corpus of tests/test_ordered_paths_gpu.py, classified on the CPU by the restated path rule (tests/ordered_paths_ref.py): every class of
ordered_kernel's selection paths is reached by a named strand whose class holds for every cut within +-4 096 of the computed one, the keys
the rule says are kept contain the oracle's row, and the build has the `ordpaths` variant the GPU test loads."""
import numpy as np
import pytest

import oracle_lib as O
import ordered_paths_ref as R
from mhap_amd import build as B

CORPORA = {"main": (R.corpus, R.MAIN_S), "wide": (R.wide_corpus, R.WIDE_S)}
_PRED = {}


def _predicted(corpus, S):
    if (corpus, S) not in _PRED:
        _PRED[(corpus, S)] = R.predict(CORPORA[corpus][0](), S)
    return _PRED[(corpus, S)]


@pytest.mark.parametrize("table", ["main", "wide"])
def test_every_class_has_a_margin_stable_strand(table):
    for cls, (corpus, S, names) in (R.TABLE if table == "main" else R.WIDE_TABLE).items():
        reads = CORPORA[corpus][0]()
        pred = _predicted(corpus, S)
        for name in names:
            p = pred[R.strand_index(reads, name)]
            print(f"{corpus} S={S} {name}: {R.describe(p.code)}{'' if p.stable else ' (NOT margin-stable)'}")
            assert R.path_class(p.code) == cls, (corpus, S, name, R.describe(p.code))
            assert p.stable, (corpus, S, name)
            assert bool(p.code & R.BIT_WIDE) == (corpus == "wide"), (corpus, name)


def test_level_endings_and_hash_sources_of_the_corpus():
    """Level 3 as the ENDING level needs more than 2^21 k2-mers in one strand and is not in the corpus; every other level is.  The raw-byte
    reads and the reads beyond the 2-bit-code path carry the MHAP_RD_MAT bit, the others do not."""
    levels = set()
    for S in R.MAIN_S:
        levels |= {p.level for p in _predicted("main", S)}
    assert levels >= {None, 0, 1, 2, 4, 5} and 3 not in levels, levels
    reads = R.wide_corpus()
    pred = _predicted("wide", 1536)
    for name, want in (("r5000/0", False), ("r5000+N/1", True), ("r70000/0", True)):
        assert bool(pred[R.strand_index(reads, name)].code & R.BIT_MAT) == want, name


@pytest.mark.parametrize("corpus", ["main", "wide"])
def test_kept_keys_contain_the_oracle_row(corpus):
    """For every corpus strand and S: the keys the rule keeps (<= bound, below the cut, or all of them) contain the oracle's K-row, and
    are no more than cap (K of n where everything is kept)."""
    reads = CORPORA[corpus][0]()
    for S in CORPORA[corpus][1]:
        pred = _predicted(corpus, S)
        for i, s in enumerate(reads.values()):
            for strand, t in ((0, s), (1, O.rc(s))):
                p = pred[2 * i + strand]
                rc_, row, _ = O.ordered(t, 12, S)
                assert rc_ == 0
                h = O.kmer_hashes32(t, 12)
                assert len(row) == min(S, len(h))
                assert np.array_equal(h[row[:, 1]], row[:, 0]), (corpus, S, i, strand)
                assert np.isin(row[:, 1], p.selected).all(), (corpus, S, i, strand, R.describe(p.code))
                assert len(p.selected) <= max(R.cap_of(S), 0) or len(h) <= R.cap_of(S)


def test_one_pass_is_not_attempted_close_to_a_power_of_two():
    for S in (64, 100, 128, 256, 400, 512, 2048):
        assert R.one_pass_cut(10 * S + 4096, S) is None, S
    for S in (300, 600, 1536):
        assert R.one_pass_cut(10 * S + 4096, S) is not None, S


def test_random_long_strands_are_rejected_as_crowded_at_the_production_size():
    """The finding recorded in EXPERIMENTS.md: at S = 1536 the cut covers about 2048 * 1810 / n bins, so from roughly 50 000 k2-mers up
    some first-level bin passes 32 staged keys and the attempt is thrown away."""
    rng = np.random.default_rng(7)
    for n, want in ((30000, R.ATT_ACCEPTED), (70000, R.ATT_CROWDED), (131000, R.ATT_CROWDED)):
        h = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        assert R.path_class(R.classify(h, 1536, n, True).code)[0] == want, n


def test_witness_line_round_trip():
    line = "[ordered paths] first 4 count 3 cap 2048 S 1536 codes: 021 382 000"
    (w,) = R.parse_witness("noise\n" + line + "\n[ordered prof] x\n")
    assert w == dict(first=4, count=3, cap=2048, S=1536, codes=[0x021, 0x382, 0])
    assert R.path_class(0x382) == (R.ATT_SHORT, R.HOW_NET0 + 4) and 0x382 & R.BIT_WIDE and 0x382 & R.BIT_MAT


def test_build_has_the_ordpaths_variant():
    flags, only = B.VARIANTS["ordpaths"]
    assert flags == ["-DMH_ORD_PATHS"] and only == ["sketch_kernels.hip"]
    assert B.variant_path("ordpaths").endswith("libmhaphip_ordpaths.so")
