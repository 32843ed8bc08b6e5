"""Homopolymer compression without a GPU: the properties of the restatement (tests/hpc_ref.py), the host rule mhap_hpc_expand_record
against it on records with every edge position, and the figure that motivates the feature, by the CPU oracle alone: with run-length
noise at rate 0.2 the search of the raw reads loses most true overlaps and the search of the compressed reads finds every one."""
import os
import re
import subprocess

import numpy as np
import pytest

from mhap_amd import api

import hpc_cases as hc
import hpc_ref as ref
import oracle_lib as O


@pytest.fixture(scope="module")
def sides():
    """Two tables of reads with different ids, compressed by the restatement: noisy reads, and a few odd ones."""
    rng = np.random.default_rng(11)
    a, _ = hc.noisy_reads(0.2, seed=3, n=6, length=600, genome=3000)
    odd = [np.zeros(0, np.uint8), np.frombuffer(b"A", np.uint8), np.frombuffer(b"AAAAAAA", np.uint8), hc.alternating(50),
           hc.runs_of(rng, 300, [ord("N"), ord("a"), ord("A"), 0, 255])]
    b = hc.table(odd, ids=np.arange(101, 101 + len(odd), dtype=np.int64))
    return (a, ref.compress(a)), (b, ref.compress(b))


def test_restatement_properties():
    rng = np.random.default_rng(1)
    for trial in range(40):
        x = hc.runs_of(rng, int(rng.integers(1, 400)), hc.ACGT, mean=int(rng.integers(1, 6)))
        c, start = ref.compress_read(x)
        c2, start2 = ref.compress_read(c)
        assert c2.tobytes() == c.tobytes() and start2.tolist() == list(range(len(c) + 1))        # compressing twice is compressing once
        assert ref.compress_read(ref.revcomp(x))[0].tobytes() == ref.revcomp(c).tobytes()        # and commutes with the reverse complement
        assert start[0] == 0 and start[-1] == len(x) and (np.diff(start) > 0).all()
        assert (x[start[:-1]] == c).all()
        # the flip: expanding the flipped ends on the forward map is the flip of the ends expanded on the reversed map
        start_rc, L, clen = ref.compress_read(ref.revcomp(x))[1], len(x), len(c)
        for p in range(-1, clen + 1):
            assert L - ref.hi(start_rc, p) - 1 == ref.lo(start, clen - p - 1), (trial, p)
            assert L - ref.lo(start_rc, p) - 1 == ref.hi(start, clen - p - 1), (trial, p)
    assert ref.compress_read(np.zeros(0, np.uint8))[1].tolist() == [0]
    assert ref.compress_read(np.frombuffer(b"aAANNn\x00\x00", np.uint8))[0].tobytes() == b"aANn\x00"


@pytest.mark.parametrize("two_sides", [False, True])
def test_expand_record_against_the_restatement(sides, two_sides):
    (fa, ra), (fb, rb) = sides
    rto, fto = (rb, fb) if two_sides else (ra, None)
    recs = hc.random_records(np.random.default_rng(2 + two_sides), ra, rto, 400)
    assert {0, 1} == set(recs["to_rc"].tolist()) and -1 in recs["a1"] and -1 in recs["b2"]
    assert (recs["a2"] == recs["alen"]).any() and (recs["b1"] == recs["blen"] - 1).any() and (recs["a1"] == 0).any()
    want = ref.expand(recs, ra, rto)
    rows_a = {int(i): r for r, i in enumerate(fa.ids.tolist())}
    rows_b = {int(i): r for r, i in enumerate((fto or fa).ids.tolist())}
    got = np.array([api.hpc_expand_record(q, ref.start_of(ra, rows_a[int(q["from_id"])]), ref.start_of(rto, rows_b[int(q["to_id"])])) for q in recs],
                   dtype=api.RECORD_DTYPE)
    assert got.tobytes() == want.tobytes()
    for k in ("from_id", "to_id", "score", "raw", "to_rc"):
        assert (got[k] == recs[k]).all()
    # the expanded records are records of the raw reads: the realignment's planner takes every one
    pairs = api.realign_plan(got, fa, query_fasta=fto)
    assert pairs.shape == (len(recs), 7)


def test_expand_record_refuses_null_and_negative():
    lib = api.load_library()
    r, s = np.zeros(1, api.RECORD_DTYPE), np.zeros(1, np.int32)
    assert lib.mhap_hpc_expand_record(api._ptr(r), api._ptr(s), 0, api._ptr(s), 0, None) == -1
    assert lib.mhap_hpc_expand_record(api._ptr(r), api._ptr(s), -1, api._ptr(s), 0, api._ptr(r)) == -1
    assert lib.mhap_hpc_expand_record(api._ptr(r), api._ptr(s), 0, api._ptr(s), 0, api._ptr(r)) == 0


def test_constants_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "mhap_hip.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (MHAP_HPC_[A-Z_]+) (\d+)", hdr)}
    assert vals == {"MHAP_HPC_TILE": api.HPC_TILE, "MHAP_HPC_SCAN_BLOCK": api.HPC_SCAN_BLOCK, "MHAP_HPC_COUNTS": len(api.HPC_COUNTS)}


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
KMERS_CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip-kmers")
SMALL = os.path.join(ROOT, "tests", "golden", "small_reads.fasta")


@pytest.mark.parametrize("flags,word", [(["-s", "reads.dat", "--hpc"], ".dat"),
                                        (["-s", SMALL, "-q", "reads.dat", "--hpc"], ".dat"),
                                        (["-s", SMALL, "--hpc", "--gpus", "2"], "one GPU"),
                                        (["-p", ".", "-q", ".", "--hpc"], "-p")])
def test_driver_refuses_before_a_handle_exists(tmp_path, flags, word):
    (tmp_path / "reads.dat").write_bytes(b"")
    p = subprocess.run([CLI] + flags, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert p.returncode == 1 and p.stdout.count("\n") == 1 and "--hpc" in p.stdout and word in p.stdout, (p.stdout, p.stderr[-500:])


def test_tools_say_where_the_parameters_apply():
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    line = re.findall(r"\n\t--hpc, default = false\n\t\t([^\n]*)\n", h.stdout)   # the flag's own help text
    assert h.returncode == 0 and len(line) == 1
    assert all(w in line[0] for w in ("-k", "--min-olap-length", "--min-store-length", "-f file", "mhap-hip-kmers --hpc"))
    k = subprocess.run([KMERS_CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert k.returncode == 0 and "--hpc" in k.stdout and "mhap-hip --hpc" in k.stdout
    bad = subprocess.run([KMERS_CLI, "--hpc", "--assess", SMALL, SMALL], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--assess" in bad.stderr


def test_noise_in_run_lengths_hides_overlaps_and_compression_finds_them():
    """40 reads of 4 000 bases from a 30 kb genome, every second one reverse-complemented, run-length noise at rate 0.2; true pairs
    share at least 1 000 genome bases.  Default parameters.  Measured with this seed: 167 true pairs, of which the raw search reports
    15 and the compressed search 167 (EXPERIMENTS.md, "Homopolymer compression")."""
    fa, true = hc.noisy_reads(0.2, seed=20261020)
    raw = hc.pairs_of(O.run_self(fa, nthreads=4)["records"])
    comp = ref.compress(fa)
    found = hc.pairs_of(O.run_self(comp["fasta"], nthreads=4)["records"])
    print(f"true pairs {len(true)}, found raw {len(true & raw)}, found compressed {len(true & found)}; compressed bases "
          f"{comp['counts']['compressed_bases']} of {comp['counts']['raw_bases']}")
    assert len(true) > 100
    assert true <= found, sorted(true - found)
    assert 2 * len(true & raw) < len(true), (len(true & raw), len(true))
