"""GetHistogramStats (mhap_amd.histogram_stats, the C export mhap_histogram_stats) against a line-for-line Python restatement of
J/main/GetHistogramStats.java (tests/histogram_stats_ref.py): the statistics bit for bit on seeded random histograms, the file reading's
edges as Java's parsing has them, the percent's edges, the worked example, and the module run as a program.  No GPU needed."""
import bz2
import gzip
import math
import os
import random
import subprocess
import sys
from fractions import Fraction

import pytest

import histogram_stats_ref as R
from mhap_amd import histogram_stats as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING_LINE = "0\t�\t\t0\t�"


def _c(hist, percent):
    keys = sorted(hist)
    return H.histogram_stats(keys, [hist[k] for k in keys], percent)


def _same(got, want, what):
    gm, gs, gc = got
    wm, ws, wc = want
    assert (float.hex(gm), float.hex(gs), gc) == (float.hex(wm), float.hex(ws), wc), what


def _write(path, text, opener=open):
    with opener(path, "wt") as fh:
        fh.write(text)
    return str(path)


def _line(hist, percent):
    return R.to_string(*R.process(hist, percent))


# ---- the arithmetic, bit for bit ------------------------------------------------------------------------------------------------

def test_worked_example():
    assert H.format_line(*_c({1: 3, 2: 1}, 0.5)) == "1.25\t.4330127\t\t1\t4.28108891"
    assert _line({1: 3, 2: 1}, 0.5) == "1.25\t.4330127\t\t1\t4.28108891"


@pytest.mark.parametrize("seed", range(12))
def test_random_histograms_match_the_restatement(seed):
    rnd = random.Random(seed)
    kind = seed % 4
    hist = {}
    for _ in range(rnd.randint(1, 40)):
        if kind == 0:     # a meryl-like histogram: small counts, many k-mers at the low end
            c = rnd.randint(1, 200)
            hist[c] = rnd.randint(0, 3000 // c)
        elif kind == 1:   # zero and negative numbers, negative counts
            hist[rnd.randint(-50, 50)] = rnd.randint(-5, 30)
        elif kind == 2:   # counts near 2^31
            hist[(1 << 31) - 1 - rnd.randint(0, 1000)] = rnd.randint(0, 40)
            hist[-(1 << 31) + rnd.randint(0, 1000)] = rnd.randint(0, 3)
        else:             # anything an int and a long can be, few steps
            hist[rnd.randint(-(1 << 31), (1 << 31) - 1)] = rnd.choice([0, 1, 2, -1, -(1 << 40), rnd.randint(0, 50)])
    for percent in (0.0, 0.5, 0.99, rnd.random(), -1.0):
        _same(_c(hist, percent), R.process(hist, percent), (seed, percent))


def test_running_sum_past_2_53():
    # (double) val * count and the running sum pass 2^53: the product is rounded as Java rounds it
    hist = {3: 5, (1 << 31) - 1: (1 << 22) + 3, (1 << 31) - 2: 7}
    assert ((1 << 31) - 1) * ((1 << 22) + 3) > 1 << 53
    for percent in (0.5, 0.99, 0.999999999):
        _same(_c(hist, percent), R.process(hist, percent), percent)


def test_negative_numbers_still_enter_the_running_sum():
    # a negative number steps the Welford loop zero times, but (double) val * count still goes into runningSum
    hist = {2: 4, 5: -3, 9: 2}
    got = _c(hist, 0.0)
    _same(got, R.process(hist, 0.0), "neg")
    assert got[2] == 2
    # runningSum / sum: 8 / 26, then (8 - 15) / 26 < 0, then (-7 + 18) / 26: the cut at 0.4 is 9, not 5
    assert _c(hist, 0.4)[2] == 9 == R.process(hist, 0.4)[2]


def test_ties_at_the_percent_are_not_above_it():
    hist = {1: 1, 3: 1}                                  # runningSum / sum: 0.25, then 1.0
    assert _c(hist, 0.25)[2] == 3 == R.process(hist, 0.25)[2]
    assert _c(hist, 0.2499)[2] == 1


def test_empty_and_all_zero_histograms():
    for hist in ({}, {5: 0}, {0: 4}, {-3: 2, 3: 2}):
        for percent in (0.5, -1.0):
            got = _c(hist, percent)
            _same(got, R.process(hist, percent), (hist, percent))
    assert H.format_line(*_c({}, 0.99)) == MISSING_LINE


# ---- the percent ----------------------------------------------------------------------------------------------------------------

def test_percent_edges():
    hist = {1: 10, 2: 5, 7: 3, 40: 1}
    assert _c(hist, 1.0)[2] == 0 and _c(hist, 1.5)[2] == 0     # never above 1
    assert _c(hist, -0.1)[2] == 1                               # the first count
    assert _c(hist, math.nan)[2] == 0                           # no comparison with NaN is true
    for p in (1.0, 1.5, -0.1, math.nan, 0.99):
        _same(_c(hist, p), R.process(hist, p), p)


def test_percent_is_parsed_as_java_parses_it(tmp_path):
    path = _write(tmp_path / "h.txt", "1 10\n2 5\n7 3\n40 1\n")
    want = _line({1: 10, 2: 5, 7: 3, 40: 1}, 0.99)
    for arg in ("0.99", "0.99d", "0.99D", " 0.99 ", ".99", "99e-2", "0.99f"):
        assert H.get_histogram_stats(path, H.parse_double(arg))[0] == want, arg
    assert H.get_histogram_stats(path, H.parse_double("NaN"))[0] == _line({1: 10, 2: 5, 7: 3, 40: 1}, math.nan)
    with pytest.raises(ValueError):
        H.parse_double("0,99")


# ---- reading the file -----------------------------------------------------------------------------------------------------------

PARSE_CASES = [
    # (file text, the TreeMap read, whether the reading ended at an exception)
    ("1 3\n2 1\n", {1: 3, 2: 1}, False),
    ("1 3\n\n2 1\n", {1: 3}, True),                              # a blank line in the middle: parseInt("") throws
    ("1 3\n4\n2 1\n", {1: 3}, True),                             # a single column: split[1] throws
    ("+5 2\n1 +3\n", {5: 2, 1: 3}, False),                       # parseInt / parseLong take a leading +
    ("1 3\n2147483648 1\n2 1\n", {1: 3}, True),                  # a count past 2^31 - 1
    ("2147483647 1\n-2147483648 2\n", {2147483647: 1, -2147483648: 2}, False),
    ("3 1\n3 7\n1 2\n", {3: 7, 1: 2}, False),                    # a repeated count replaces the earlier one
    ("  1\t\t3  \n2 \t 1\r\n\t4   5 extra\r6 12\n", {1: 3, 2: 1, 4: 5, 6: 12}, False),   # tabs, mixed whitespace, \r\n and \r
    ("1 3\n2 9223372036854775808\n", {1: 3}, True),             # a number past Long.MAX_VALUE
    ("1 3.0\n", {}, True),
    ("1 3\n2 1", {1: 3, 2: 1}, False),                           # no final newline
    ("", {}, False),
]


@pytest.mark.parametrize("i", range(len(PARSE_CASES)))
def test_parse_edges(tmp_path, i):
    text, hist, failed = PARSE_CASES[i]
    path = _write(tmp_path / "h.txt", text)
    got, ok, err = H.read_histogram(path)
    assert got == hist and ok == (not failed) and (err is not None) == failed
    # after an exception the percent argument is never taken: percent stays 0.99
    line, err2 = H.get_histogram_stats(path, 0.5)
    assert line == _line(hist, 0.99 if failed else 0.5) and err2 == err


def test_long_max_is_read(tmp_path):
    path = _write(tmp_path / "h.txt", "7 9223372036854775807\n8 -9223372036854775808\n")
    assert H.read_histogram(path) == ({7: (1 << 63) - 1, 8: -(1 << 63)}, True, None)


def test_compressed_files(tmp_path):
    text = "1 30\n2 10\n3 4\n60 1\n"
    want = _line({1: 30, 2: 10, 3: 4, 60: 1}, 0.9)
    cases = [("h.gz", gzip.open), ("h.txt.gz", gzip.open), ("h.bz2", bz2.open), ("hgz", gzip.open), ("hbz2", bz2.open)]
    for name, opener in cases:                                   # (endsWith("gz"): no dot required)
        path = _write(tmp_path / name, text, opener)
        assert H.get_histogram_stats(path, 0.9) == (want, None), name
    plain = _write(tmp_path / "h.gzip", text)                    # a name that does not end in gz is read as text
    assert H.get_histogram_stats(plain, 0.9) == (want, None)
    not_gz = _write(tmp_path / "plain.gz", text)                 # not gzip data: the stream fails at once
    line, err = H.get_histogram_stats(not_gz, 0.9)
    assert line == MISSING_LINE and err


def test_missing_file(tmp_path):
    line, err = H.get_histogram_stats(str(tmp_path / "nope.txt"), 0.5)
    assert line == "0\t�\t\t0\t�" and "nope.txt" in err


# ---- the program ----------------------------------------------------------------------------------------------------------------

def _run(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "mhap_amd.histogram_stats", *args], capture_output=True, text=True, env=env, timeout=120)


def test_module_as_a_program(tmp_path):
    good = _write(tmp_path / "h.txt", "1 3\n2 1\n")
    r = _run(good, "0.5")
    assert (r.returncode, r.stdout, r.stderr) == (0, "1.25\t.4330127\t\t1\t4.28108891\n", "")
    bad = _write(tmp_path / "bad.txt", "1 3\n2 x\n5 5\n")
    r = _run(bad, "0.5")
    assert r.returncode == 0 and r.stdout == _line({1: 3}, 0.99) + "\n"
    assert len(r.stderr.strip().split("\n")) == 1 and "line 2" in r.stderr and '"x"' in r.stderr
    r = _run(str(tmp_path / "nope.txt"), "0.5")
    assert r.returncode == 0 and r.stdout == MISSING_LINE + "\n" and len(r.stderr.strip().split("\n")) == 1
    r = _run(good, "half")                                        # Double.parseDouble throws before the file is read
    assert r.returncode == 1 and r.stdout == "" and "half" in r.stderr
    r = _run(good)
    assert r.returncode == 1 and r.stdout == "" and "Usage" in r.stderr


def test_stats_loop_is_not_contracted():
    # variance += delta * (val - mean) rounded twice, as Java does: on these histograms one fused multiply-add gives another stdev
    rnd = random.Random(99)
    differs = 0
    for _ in range(200):
        hist = {rnd.randint(1, 10 ** 6): rnd.randint(1, 3) for _ in range(6)}
        want = R.process(hist, 0.5)
        _same(_c(hist, 0.5), want, hist)
        mean = var = 0.0
        total = 0
        for v in sorted(hist):
            for _ in range(hist[v]):
                total += 1
                d = v - mean
                mean += d / total
                var = _fma(d, v - mean, var)
        differs += math.sqrt(var / total) != want[1]
    assert differs > 0


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))
