"""KmerStatSimulator without a GPU: the host replay of Java's trials (mhap_ksim_next) against the literal transcription (ksim_ref.py),
Double.toString, the FASTA output of Usage 2, argument dispatch, messages and exit codes."""
import math
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mhap_amd import kmer_sim as K, roc  # noqa: E402
import ksim_ref as R  # noqa: E402

PACBIO = (0.1188, 0.0183, 0.0129)


def _records(seed=3, lens=(100, 900, 300, 2000, 650), alphabet="ACGT"):
    rng = random.Random(seed)
    return ["".join(rng.choice(alphabet) for _ in range(n)) for n in lens]


def _replay(trials, L, rates, k=12, overlap=40, one_sided=False, ref=None, sim_only=False, length=None):
    err, pi, pd, ps = K._rates(*rates)
    length = float(L) if length is None else length
    g = K._JavaTrials(0, L, K._java_int(2 * length - overlap), err, pi, pd, ps, one_sided, sim_only,
                      [r.encode() for r in ref] if ref is not None else None)
    try:
        rd, meta, done, e = g.next(trials)
    finally:
        g.close()
    roles = 1 if sim_only else 3
    return [(r, rd[t, r].tobytes().decode()) for t in range(done) for r in range(roles)], meta[:done], e


def _transcribe(trials, L, rates, k=12, overlap=40, one_sided=False, ref=None):
    f = R.KmerStatSimulator(0)
    f.totalTrials, f.requestedLength, f.kmer, f.overlap, f.halfError, f.reference = trials, float(L), k, overlap, one_sided, ref
    try:
        f.simulate(*rates)
        e = None
    except R.JavaException as x:
        e = str(x)
    return f, e


def test_next_double_matches_java():
    r = roc.JavaRandom(0)
    assert r.next_double() == 0.730967787376657       # new Random(0).nextDouble()
    assert r.next_double() == 0.24053641567148587


@pytest.mark.parametrize("case", ["plain", "ref", "ref_one_sided", "one_sided", "rate0", "rate1", "all_ins", "all_del_short", "iupac_ref"])
def test_replay_matches_transcription(case):
    L, trials, ref, one, rates = 120, 12, None, False, PACBIO
    if case.startswith("ref"):
        ref = _records(lens=(100, 300, 479, 480, 2000, 240, 239))   # records shorter than 4L and 2L, and at the limits
    one = case in ("ref_one_sided", "one_sided")
    if case == "rate0":
        rates = (0.0, 0.0, 0.0)
    elif case == "rate1":
        rates = (0.5, 0.2, 0.3)
    elif case == "all_ins":
        rates = (0.3, 0.0, 0.0)
    elif case == "all_del_short":
        rates = (0.0, 0.6, 0.0)       # 2L bases lose 60 %: too short, the first getSequence throws
    elif case == "iupac_ref":
        ref = _records(lens=(600, 900), alphabet="ACGTRYKM")
        rates = (0.05, 0.05, 0.3)
    f, e = _transcribe(trials, L, rates, one_sided=one, ref=ref)
    got, meta, ge = _replay(trials, L, rates, one_sided=one, ref=ref)
    assert got == f.reads[:len(got)]
    if e is None:
        assert ge is None and len(got) == 3 * trials
    else:
        assert ge is not None and ge[0] == e and "StringIndexOutOfBounds" in e


def test_replay_too_short_second_read():
    # trimRight's substring(0, L) of the shared partner
    rates = (0.0, 0.55, 0.0)
    f, e = _transcribe(30, 100, rates)
    got, meta, ge = _replay(30, 100, rates)
    assert e is not None and ge is not None and ge[0] == e
    assert got == f.reads[:len(got)]


def test_wrap_and_positions():
    ref = _records(lens=(500, 800))
    f, e = _transcribe(40, 120, PACBIO, overlap=100, ref=ref)
    got, meta, ge = _replay(40, 120, PACBIO, overlap=100, ref=ref)
    assert e is None and got == f.reads
    lens = np.array([len(ref[i]) for i in meta[:, 0]])
    assert (meta[:, 1] + 240 > lens).any()       # some first windows wrap past the end of their record
    assert ((meta[:, 1] + 140) % lens == meta[:, 2]).all()


def _fasta_file(tmp_path, recs, name="ref.fa"):
    p = tmp_path / name
    p.write_text("".join(f">r{i} x\n" + "\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + "\n" for i, r in enumerate(recs)))
    return str(p)


def _cli(*args, env=None):
    return subprocess.run([sys.executable, "-m", "mhap_amd.kmer_sim", *map(str, args)], cwd=ROOT, capture_output=True, text=True,
                          env=env, timeout=600)


def test_usage2_cli_stdout_equals_transcription():
    r = _cli(30, 400, *PACBIO)
    assert r.returncode == 0, r.stderr
    want, _ = R.run(30, 400, *PACBIO)
    assert r.stdout == want
    assert r.stderr.splitlines() == ["Started...", "Loaded reference", "Done 0/30"]


def test_usage2_cli_reference_with_n(tmp_path):
    recs = _records(lens=(1000, 2500, 700))
    raw = [recs[0][:300] + "NNnn" + recs[0][300:], recs[1].lower(), recs[2][:50] + "N" + recs[2][50:]]
    path = _fasta_file(tmp_path, raw)
    r = _cli(25, 250, 0.1, 0.05, 0.05, path, "--seed", 0)
    assert r.returncode == 0, r.stderr
    want, _ = R.run(25, 250, 0.1, 0.05, 0.05, reference=recs)
    assert r.stdout == want
    assert K.load_reference(path) == [x.encode() for x in recs]


def test_usage2_api_and_seed():
    reads, ids = K.simulate_reads(5, 90, *PACBIO, seed=7)
    f = R.KmerStatSimulator(7)
    f.totalTrials, f.requestedLength = 5, 90.0
    f.simulate(*PACBIO)
    assert [reads[i].tobytes().decode() for i in range(5)] == [x for _, x in f.reads]
    assert (ids[:, 0] == 0).all() and (ids[:, 1] == 90).all()


def test_convert_to_fasta():
    assert K.convert_to_fasta("A" * 60) == "A" * 60
    assert K.convert_to_fasta("A" * 61) == "A" * 60 + "\nA"
    assert K.convert_to_fasta("A" * 120) == "A" * 60 + "\n" + "A" * 60
    assert K.convert_to_fasta("") == ""


# ---- Double.toString ----------------------------------------------------------------------------------------------------
TABLE = [(0.0, "0.0"), (-0.0, "-0.0"), (1.0, "1.0"), (1e7, "1.0E7"), (9999999.0, "9999999.0"), (0.001, "0.001"), (9.99e-4, "9.99E-4"),
         (1e-5, "1.0E-5"), (5e-324, "4.9E-324"), (1.7976931348623157e308, "1.7976931348623157E308"), (math.nan, "NaN"),
         (math.inf, "Infinity"), (-math.inf, "-Infinity"), (100.0, "100.0"), (0.1, "0.1"), (-2.5e-8, "-2.5E-8"), (1e21, "1.0E21"),
         (2e-3, "0.002"), (123456.789, "123456.789"), (1.0e-3 * 0.5, "5.0E-4"), (2.0 ** -1074 * 2, "1.0E-323")]


@pytest.mark.parametrize("x,s", TABLE)
def test_java_double_table(x, s):
    assert K.java_double(x) == s


def test_java_double_random_round_trip_and_shortest():
    rng = random.Random(11)
    vals = [struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0] for _ in range(1500)]
    vals += [rng.random() for _ in range(1500)] + [rng.random() * 10 ** rng.randint(-8, 9) for _ in range(1000)]
    for x in vals:
        if x != x or math.isinf(x):
            continue
        s = K.java_double(x)
        assert float(s) == x, (x, s)
        mant = s.lstrip("-").split("E")[0]
        ds = mant.replace(".", "").lstrip("0").rstrip("0") or "0"
        assert len(ds) <= max(len(repr(abs(x)).split("e")[0].replace(".", "").lstrip("0").rstrip("0")), 2), (x, s)
        a = abs(x)
        assert ("E" in s) == (not (1e-3 <= a < 1e7)), (x, s)


def test_output_stats_single_trial_is_nan():
    m, sd = K.output_stats([3.0])
    assert m == 3.0 and math.isnan(sd)
    assert K.output_stats([1.0, 2.0, 4.0]) == R.KmerStatSimulator.outputStats([1.0, 2.0, 4.0])


def test_jaccard_to_identity():
    assert K.jaccard_to_identity(0.0, 16) == 0.0
    assert K.jaccard_to_identity(1.0, 16) == 1.0
    j = 0.3
    assert K.jaccard_to_identity(j, 16) == math.exp(-(-1.0 / 16 * math.log(2.0 * j / (1.0 + j))))
    assert math.isnan(K.jaccard_to_identity(math.nan, 16))


# ---- dispatch, messages, exit codes (all decided before the GPU is needed) -------------------------------------------------
def test_too_few_arguments_prints_usage():
    r = _cli(1, 2, 3, 4)
    assert r.returncode == 1 and r.stdout == "" and r.stderr == K.USAGE


def test_overlap_longer_than_length():
    r = _cli(3, 16, 400, 401, *PACBIO)
    assert r.returncode == 1 and r.stderr == "Cannot have overlap > sequence length\n"


@pytest.mark.parametrize("rates", [(0.5, 0.4, 0.2), (-0.5, 0.1, 0.1)])
def test_error_rate_outside_unit_interval(rates):
    r = _cli(3, 16, 400, 100, *rates)
    assert r.returncode == 1 and r.stderr == "Error rate must be between 0 and 1\n"
    r = _cli(3, 400, *rates)
    assert r.returncode == 1 and r.stderr == "Error rate must be between 0 and 1\n"


@pytest.mark.parametrize("args,bad", [(("x", 16, 400, 100, *PACBIO), "x"), ((3, "1.5", 400, 100, *PACBIO), "1.5"),
                                      ((3, 16, "abc", 100, *PACBIO), "abc"), ((3, 16, 400, 100, "0.1q", 0.0, 0.0), "0.1q"),
                                      ((3, "4e2", *PACBIO), "4e2x")])
def test_parse_errors(args, bad):
    if bad == "4e2x":
        r = _cli(3, "4e2x", *PACBIO)
    else:
        r = _cli(*args)
    assert r.returncode == 1
    assert r.stderr.endswith(f'java.lang.NumberFormatException: For input string: "{bad}"\n')


def test_non_integral_length():
    r = _cli(3, 16, "400.5", 100, *PACBIO)
    assert r.returncode == 1
    assert r.stderr == "Started...\nLoaded reference\nDone 0/3\nError wrong length first: 400 second: 400 requested 400.5\n"
    assert r.stdout == ""


def test_k_zero_refused_and_negative_k_simulates():
    r = _cli(3, 0, 400, 100, *PACBIO)
    assert r.returncode == 1 and "k-mer size of 0" in r.stderr
    r = _cli(6, -1, 200, 100, *PACBIO)
    assert r.returncode == 0, r.stderr
    assert r.stdout == R.run(6, 200, *PACBIO)[0]


def test_load_skip_mers_errors(tmp_path):
    p = tmp_path / "skip.txt"
    p.write_text("ACGTACGTACGTACGT 5\nCCCC\n")
    with pytest.raises(K.KsimError, match="ArrayIndexOutOfBounds"):
        K.load_skip_mers(str(p))
    p.write_text("ACGT 5\n  TTTT\t7  \n")
    assert K.load_skip_mers(str(p)) == {"ACGT": 5, "TTTT": 7}
    p.write_text("ACGT five\n")
    with pytest.raises(K.KsimError, match="NumberFormatException"):
        K.load_skip_mers(str(p))


def test_reference_without_a_long_record(tmp_path):
    path = _fasta_file(tmp_path, _records(lens=(300, 500)))
    with pytest.raises(K.KsimError, match="loops forever"):
        K.simulate_reads(3, 200, *PACBIO, reference=path)


def test_never_ending_insertions_refused():
    with pytest.raises(K.KsimError, match="loops forever"):
        K.simulate_reads(3, 100, 1.0, 0.0, 0.0)


def test_own_options_removed_before_dispatch():
    r = _cli("--rng", "java", 4, 100, *PACBIO, "--seed=3")
    assert r.returncode == 0, r.stderr
    assert r.stdout == R.run(4, 100, *PACBIO, seed=3)[0]
    r = _cli("--rng", "philox", 4, 100, *PACBIO)
    assert r.returncode == 2 and "unknown --rng" in r.stderr
