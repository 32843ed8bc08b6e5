"""Every selection path of ordered_kernel against the oracle, with a witness of the path each strand took.

ordered_kernel (mhap_amd/csrc/sketch_kernels.hip) chooses per strand between the all-keys network, the one-pass attempt (accepted, or rejected
as short / over / crowded), level-0 buckets and the network after an exact selection that ends at level 0 ... 5, with hashes read from memory
or recomputed from 2-bit codes and with 16- or 32-bit staged positions.  tests/ordered_paths_ref.py restates that rule on the CPU;
tests/test_ordered_paths_cpu.py shows that the corpus reaches every class.  Here every corpus runs twice:
  * on the shipped library, in this process: every strand's ordered row, size and status against the oracle (O.ordered);
  * on the `ordpaths` build (mhap_amd/build.py VARIANTS: -DMH_ORD_PATHS), in a fresh child process (the library path is fixed at import):
    the same comparison with the oracle, and the `[ordered paths]` witness lines, whose per-strand codes must equal the predictor's for every
    strand whose class is stable under the cut margin (all of this corpus are) — so that a failure says "path X was wrong on strand Y".
Agreement between two GPU paths is never what is asserted.

Network level 3 as the ENDING level needs a strand of more than 2^21 k2-mers and is not tested; levels 2 and 3 as passed-through levels are
covered by the level-4 / level-5 strands (poly-A, poly-C, ACGTTGCA repeats).  Level 2 as the ending is covered by the `level2` read at S = 1, 2.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import ordered_paths_ref as R
from mhap_amd import FastaData, MhapParams, MinHashSearch
from test_small_grids_gpu import _expected_sketches, _sketch_mismatches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CHILD_TIMEOUT = 240      # seconds: library start-up + a few sketch() calls of at most 0.3 M bases + the oracle's rows
H = 16                   # MinHash rows are not what this file is about: small, but still compared

CORPORA = {"main": (R.corpus, R.MAIN_S), "wide": (R.wide_corpus, R.WIDE_S)}
# hash sources: 2-bit codes (fused; raw-byte reads and reads beyond the LDS path stay MHAP_RD_MAT), every strand MHAP_RD_MAT, k2 = 13
CONFIGS = {"packed": dict(env={}, k=16, k2=12), "unfused": dict(env={"MHAP_FUSED_HASH": "0"}, k=16, k2=12), "k2_13": dict(env={}, k=15, k2=13)}
ORDERED_SWITCHES = ("MHAP_FUSED_HASH", "MHAP_ORDERED_SPLIT", "MHAP_ORDERED_FIRST", "MHAP_ORDERED_NOWAIT", "MHAP_BATCH_BASES", "MHAP_NUM_CUS")
CASES = [("main", "packed"), ("main", "unfused"), ("main", "k2_13"), ("wide", "packed"), ("wide", "unfused")]


def _params(config, S):
    c = CONFIGS[config]
    return MhapParams(kmer_size=c["k"], num_hashes=H, ordered_kmer_size=c["k2"], ordered_sketch_size=S, min_olap_length=0)


@functools.lru_cache(maxsize=None)
def _fasta(corpus):
    return FastaData.from_strings(list(CORPORA[corpus][0]().values()))


@functools.lru_cache(maxsize=None)
def _expected(corpus, config, S):
    """The oracle's sketches of the corpus: computed once per process, shared by the cases, never modified."""
    return _expected_sketches(_fasta(corpus), _params(config, S))


@functools.lru_cache(maxsize=None)
def _predicted(corpus, config, S):
    c = CONFIGS[config]
    return R.predict(CORPORA[corpus][0](), S, c["k"], c["k2"], fused_env="MHAP_FUSED_HASH" not in c["env"])


def _names(corpus):
    return [f"{n}/{s}" for n in CORPORA[corpus][0]() for s in (0, 1)]


def _sketch_all(corpus, config, extra_env=None):
    """{S: names of the strands that differ from the oracle} for the library this process loaded (the switches are read at every launch)."""
    env = dict(CONFIGS[config]["env"], **(extra_env or {}))
    saved = {k: os.environ.pop(k, None) for k in ORDERED_SWITCHES}
    os.environ.update(env)
    try:
        fa, names, bad = _fasta(corpus), _names(corpus), {}
        for S in CORPORA[corpus][1]:
            p = _params(config, S)
            sys.stderr.write(f"[case] S {S}\n")
            sys.stderr.flush()
            with MinHashSearch(p) as ms:
                sk = ms.sketch(fa)
            bad[S] = [names[e] for e in _sketch_mismatches(fa, p, sk, _expected(corpus, config, S))]
        return bad
    finally:
        for k in ORDERED_SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _two_handles_bad(config="packed"):
    """One handle sketches the wide corpus' short reads, then the main corpus (other reads, other lengths, more of them): names of the
    strands of the SECOND result that differ from the oracle (rows are compared up to ordered_size only)."""
    fa1, fa2, S = FastaData.from_strings([s[37:] for s in list(R.corpus().values())[::-1] if len(s) > 300]), _fasta("main"), 1536
    p = _params(config, S)
    with MinHashSearch(p) as ms:
        first = ms.sketch(fa1)
        second = ms.sketch(fa2)
    assert first["ordered_size"].max() == S
    return [_names("main")[e] for e in _sketch_mismatches(fa2, p, second, _expected("main", config, S))]


def _child_main(mode, corpus, config):
    """Runs in the child process on the ordpaths build: the parity check of the parent, and the witness lines on stderr."""
    import mhap_amd
    assert mhap_amd.api._LIB_PATH.endswith("libmhaphip_ordpaths.so"), mhap_amd.api._LIB_PATH
    if mode == "table":
        bad = _sketch_all(corpus, config)
    elif mode == "split":
        bad = _sketch_all(corpus, config, {"MHAP_ORDERED_SPLIT": "50"})
    elif mode == "first":
        bad = _sketch_all(corpus, config, {"MHAP_ORDERED_FIRST": "1"})
    else:
        bad = {1536: _two_handles_bad(config)}
    print("PARITY " + repr(bad))
    assert not any(bad.values()), bad


@functools.lru_cache(maxsize=None)
def _run_child(mode, corpus, config):
    """{S: witness lines} of one child; asserts that the child ran and that its own comparison with the oracle passed."""
    from mhap_amd import build as B
    lib = B.variant_path("ordpaths")
    assert os.path.exists(lib), f"{lib} missing: __graft_entry__.build() builds it (python -m mhap_amd.build --variants)"
    env = dict(os.environ, MHAP_LIB_PATH=lib, PYTHONPATH=os.pathsep.join([ROOT, TESTS, os.environ.get("PYTHONPATH", "")]))
    for k in ORDERED_SWITCHES:
        env.pop(k, None)
    code = f"import test_ordered_paths_gpu as T; T._child_main({mode!r}, {corpus!r}, {config!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-4000:] + r.stderr[-4000:])
    assert "PARITY " in r.stdout
    by_S, cur = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("[case] S "):
            cur = int(ln.split()[-1])
            by_S[cur] = []
        elif cur is not None:
            by_S[cur] += R.parse_witness(ln)
    return by_S


def _assert_codes(corpus, config, S, lines):
    """The witness lines tile the strands, and every margin-stable strand took the path the restated rule predicts."""
    names, pred = _names(corpus), _predicted(corpus, config, S)
    assert lines, f"S {S}: no [ordered paths] line"
    codes, at = [], 0
    for w in sorted(lines, key=lambda w: w["first"]):
        assert w["first"] == at and w["S"] == S and w["cap"] == R.cap_of(S), (w["first"], at, w["S"], w["cap"])
        assert w["first"] % 2 == 0 and w["count"] % 2 == 0       # both strands of a read in one part
        codes += w["codes"]
        at += w["count"]
    assert at == len(names), (at, len(names))
    wrong = [f"{names[e]} at S {S}: took [{R.describe(codes[e])}], the rule says [{R.describe(pred[e].code)}]"
             for e in range(len(names)) if pred[e].stable and codes[e] != pred[e].code]
    assert not wrong, wrong
    return codes


@pytest.mark.parametrize("corpus,config", CASES)
def test_shipped_kernel_rows_equal_the_oracle(corpus, config):
    bad = _sketch_all(corpus, config)
    assert not any(bad.values()), f"{corpus} / {config}: strands whose sketch differs from the oracle, by S: {bad}"


@pytest.mark.parametrize("corpus,config", CASES)
def test_ordpaths_rows_equal_the_oracle_and_paths_equal_the_rule(corpus, config):
    by_S = _run_child("table", corpus, config)
    for S in CORPORA[corpus][1]:
        codes = _assert_codes(corpus, config, S, by_S.get(S))
        assert len(by_S[S]) == 1                                   # one launch
        mat_all = config != "packed"
        for name, code in zip(_names(corpus), codes):
            assert code != 0, name
            assert bool(code & R.BIT_WIDE) == (corpus == "wide"), (name, hex(code))
            if mat_all or name.split("/")[0].endswith("+N"):
                assert code & R.BIT_MAT, (name, hex(code))
            elif len(CORPORA[corpus][0]()[name.split("/")[0]]) < 20000:
                assert not code & R.BIT_MAT, (name, hex(code))


@pytest.mark.parametrize("config", ["packed", "unfused"])
def test_every_class_of_the_table_appears(config):
    """With hashes from 2-bit codes and with every strand's hashes stored: each class of ordered_paths_ref.TABLE / WIDE_TABLE is taken on the
    GPU by the strands named there (the k2 = 13 run has other hashes: its strands are held to the rule one by one above)."""
    for table in (R.TABLE, R.WIDE_TABLE):
        for cls, (corpus, S, strands) in table.items():
            w = _run_child("table", corpus, config)[S]
            codes = [c for x in sorted(w, key=lambda x: x["first"]) for c in x["codes"]]
            for name in strands:
                got = codes[R.strand_index(CORPORA[corpus][0](), name)]
                assert R.path_class(got) == cls, f"{corpus} S {S} {name}: took [{R.describe(got)}]"
                print(f"{config} {corpus} S {S} {name}: {R.describe(got)}")


@pytest.mark.parametrize("mode,env,parts", [("split", {"MHAP_ORDERED_SPLIT": "50"}, 2), ("first", {"MHAP_ORDERED_FIRST": "1"}, 1)])
def test_two_part_launch(mode, env, parts):
    """MHAP_ORDERED_SPLIT=50: the ordered kernel runs in two launches around the MinHash launch; MHAP_ORDERED_FIRST=1: all of it in front."""
    bad = _sketch_all("main", "packed", env)
    assert not any(bad.values()), bad
    by_S = _run_child(mode, "main", "packed")
    for S in R.MAIN_S:
        _assert_codes("main", "packed", S, by_S.get(S))
        assert len(by_S[S]) == parts, by_S[S]
        assert all(w["count"] > 0 for w in by_S[S])


def test_second_sketch_of_a_handle_leaves_no_stale_rows():
    bad = _two_handles_bad()
    assert not bad, bad
    _run_child("reuse", "main", "packed")      # (asserts the child's own comparison)
