"""Overlap selection without a GPU: the restatement tests/select_ref.py against tables worked out by hand, the host entry point
mhap_select_judge_record against the restatement (random records, products that are exactly integral, products just below an integer,
scores above 1, NaN and 0, spans at min_span and one below), the refusals of parameters, driver and tools, and the table text."""
import math
import os
import subprocess

import numpy as np
import pytest

from mhap_amd import api, best_overlaps, correct

import select_ref as ref
import trim_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
SMALL = os.path.join(ROOT, "tests", "golden", "small_reads.fasta")

# the worked example: four reads, best_n 2, min_span 10.  Views by read (key = 1 + floor(span * score)):
#   read 1: A of r0 (span 20, 0.5 -> 11), A of r1 (span 40, 0.25 -> 11), B of r2 (span 30, 1.0 -> 31), A of r3 (span 12, 0.9 -> 11)
#           four entries, keys 31 11 11 11: the 2nd greatest is 11, the tie at the last place keeps all four
#   read 2: B of r0 (span 20 -> 11), A of r2 (span 30 -> 31), B of r4 (span 50, 0.8 -> 41): keys 41 31 11, thr 31, kept 2
#   read 3: B of r1 (span 9 < min_span: no view), B of r3 (span 12 -> 11), A of r4 (span 50 -> 41): two entries, thr 1
#   read 4: nothing.   r5 is a self overlap, r6 has score 0, r7 a NaN score: not eligible
HAND_P = dict(best_n=2, min_span=10, min_identity=0.0)
HAND_IDS = np.array([1, 2, 3, 4], np.int64)
HAND_LEN = np.array([100, 100, 100, 100], np.int32)


def hand_records():
    return tc.recs([tc.rec(1, 2, 0, 19, 100, 10, 29, 100, 0, 0.5),
                    tc.rec(1, 3, 5, 44, 100, 0, 8, 100, 1, 0.25),
                    tc.rec(2, 1, 0, 29, 100, 70, 99, 100, 0, 1.0),
                    tc.rec(1, 3, 0, 11, 100, 50, 61, 100, 0, 0.9),
                    tc.rec(3, 2, 0, 49, 100, 50, 99, 100, 1, 0.8),
                    tc.rec(4, 4, 0, 49, 100, 50, 99, 100, 0, 0.9),
                    tc.rec(4, 1, 0, 49, 100, 0, 49, 100, 0, 0.0),
                    tc.rec(4, 2, 0, 49, 100, 0, 49, 100, 0, float("nan"))])


def test_restatement_against_the_hand_computed_table():
    P = ref.params(**HAND_P)
    records = hand_records()
    assert [ref.judge_record(r, P) for r in records] == [(11, 11), (11, 0), (31, 31), (11, 11), (41, 41), (0, 0), (0, 0), (0, 0)]
    m = ref.select(HAND_IDS, HAND_LEN, records, P)
    assert m["rows"].tolist() == [[4, 4, 11, 31], [3, 2, 31, 41], [2, 2, 1, 41], [0, 0, 1, 0]]
    assert m["counts"] == dict(reads=4, reads_with_entry=3, reads_over=2, entries=9, kept=8, eligible_records=5)
    assert ref.apply(HAND_IDS, m["thr"], records, P).tolist() == [1, 1, 3, 3, 3, 0, 0, 0]
    # the next key one below the best_n-th: it goes
    m1 = ref.select(HAND_IDS, HAND_LEN, records, ref.params(best_n=1, min_span=10))
    assert m1["rows"].tolist() == [[4, 1, 31, 31], [3, 1, 41, 41], [2, 1, 41, 41], [0, 0, 1, 0]]
    assert ref.apply(HAND_IDS, m1["thr"], records, ref.params(best_n=1, min_span=10)).tolist() == [0, 0, 2, 0, 3, 0, 0, 0]


def test_restatement_vectorised_keys_equal_the_scalar_ones():
    rng = np.random.default_rng(3)
    records = _random_records(rng, 500)
    P = ref.params(min_span=300, min_identity=0.6)
    el, ka, kb = ref.keys_of(records, P)
    for q, r in enumerate(records):
        assert (int(ka[q]), int(kb[q])) == ref.judge_record(r, P) and bool(el[q]) == ref.eligible(r, P)


def _random_records(rng, n):
    out = []
    for _ in range(n):
        la, lb = int(rng.integers(600, 60000)), int(rng.integers(600, 60000))
        sa, sb = int(rng.integers(1, la + 1)), int(rng.integers(1, lb + 1))
        a1, b1 = int(rng.integers(0, la - sa + 1)), int(rng.integers(0, lb - sb + 1))
        cols = max(sa, sb) + int(rng.integers(0, 50))
        score = 1.0 - int(rng.integers(0, cols)) / cols       # 1 - errors / columns, as the realignment reports it
        out.append(tc.rec(int(rng.integers(1, 50)), int(rng.integers(1, 50)), a1, a1 + sa - 1, la, b1, b1 + sb - 1, lb, int(rng.integers(0, 2)), score))
    return tc.recs(out)


def test_host_keys_against_restatement_on_random_records():
    rng = np.random.default_rng(11)
    records = _random_records(rng, 3000)
    for kw in (dict(), dict(min_span=0), dict(min_span=2000, min_identity=0.7)):
        P = ref.params(**kw)
        seen = set()
        for r in records:
            el, ka, kb = api.select_judge_record(r, **P)
            assert (ka, kb) == ref.judge_record(r, P) and el == ref.eligible(r, P), r
            seen.add((ka > 0, kb > 0))
        assert len(seen) == (2 if P["min_span"] == 0 else 4)     # both views, one of either side, none


def _one(span, score, alen=1 << 22):
    return tc.rec(1, 2, 7, 7 + span - 1, alen, 0, span - 1, alen, 0, score)


@pytest.mark.parametrize("span,score,key", [(1000, 0.5, 501), (1000, 0.25, 251), (1000, 1.0, 1001), (4096, 0.5, 2049), (3, 1.0, 4),
                                            (3, 1 - 1 / 3, 3),          # 3 * 0.6666666666666667 is 2.0 in double
                                            (999, 1 - 1 / 3, 667),      # 666.0000000000001
                                            (15, 1 - 4 / 5, 3),         # 15 / 5 = 3, but 15 * 0.19999999999999996 is 2.999999999999999: floor 2
                                            (18, 1 - 5 / 6, 3),         # 2.999999999999999 again
                                            (10, 1 - 8 / 10, 2),        # 1.9999999999999996
                                            (100, 0.57, 57),            # 56.99999999999999
                                            (1000, 0.7, 701), (1000, 0.29, 291),
                                            (1000, 1.5, 1001), (1000, 7e300, 1001), (1000, float("inf"), 1001),
                                            (2 ** 22 - 8, 1.0, 2 ** 22 - 7), (1, 1e-9, 1)])
def test_host_keys_at_hand_values(span, score, key):
    """Exactly integral products, products just below an integer, and scores above 1 (capped at 1)."""
    P = ref.params(min_span=0)
    r = _one(span, score)
    assert ref.judge_record(r, P) == (key, key)
    assert api.select_judge_record(r, min_span=0) == (True, key, key)


def test_host_keys_of_ineligible_records_and_span_edges():
    for score in (0.0, float("nan"), -0.0):
        assert api.select_judge_record(_one(1000, score)) == (False, 0, 0) and ref.judge_record(_one(1000, score), ref.params()) == (0, 0)
    self_rec = tc.rec(5, 5, 0, 999, 2000, 0, 999, 2000, 0, 0.9)
    assert api.select_judge_record(self_rec) == (False, 0, 0)
    assert api.select_judge_record(_one(1000, 0.59), min_identity=0.6) == (False, 0, 0)
    assert api.select_judge_record(_one(1000, 0.6), min_identity=0.6) == (True, 601, 601)
    # a span of min_span is a view, one below is none, and the two sides are judged apart
    assert api.select_judge_record(_one(500, 0.9)) == (True, 451, 451)
    assert api.select_judge_record(_one(499, 0.9)) == (True, 0, 0)
    mixed = tc.rec(1, 2, 0, 499, 5000, 100, 598, 5000, 1, 0.9)
    assert api.select_judge_record(mixed) == (True, 451, 0) == (True,) + ref.judge_record(mixed, ref.params())
    # a negative score that a negative min_identity lets through counts no match
    assert api.select_judge_record(_one(1000, -0.5), min_identity=-1.0) == (True, 1, 1) == (True,) + ref.judge_record(_one(1000, -0.5), ref.params(min_identity=-1.0))
    with pytest.raises(api.MhapError):     # an eligible record outside its read
        api.select_judge_record(tc.rec(1, 2, 0, 100, 100, 0, 50, 100, 0, 0.9))


def test_bad_parameters_are_refused():
    for kw in (dict(best_n=0), dict(best_n=-3), dict(min_span=-1)):
        with pytest.raises(ValueError):
            ref.params(**kw)
        with pytest.raises(api.MhapError):
            api.select_judge_record(_one(1000, 0.9), **kw)


def test_counts_line_and_table_text():
    line = api.select_counts_line([10, 8, 2, 500, 300, 260])
    assert line == "Best overlaps: 10 reads, 8 with a view, 2 cut; 300 of 500 views kept; 260 eligible overlaps"
    assert line == ref.counts_line(dict(zip(ref.COUNTS, [10, 8, 2, 500, 300, 260])))
    rows = np.array([[4, 4, 11, 31], [0, 0, 1, 0]], np.int32)
    assert api.select_table_text([7, 9], rows) == "7 4 4 11\n9 0 0 1\n" == ref.table_text([7, 9], rows)


BEST = ["--realign", "--best-overlaps", "5"]


@pytest.mark.parametrize("flags,word", [(["-s", SMALL, "--best-overlaps", "5"], "--realign too"),
                                        (["-s", SMALL, "-q", SMALL] + BEST, "no -q"),
                                        (["-s", SMALL, "--gpus", "2"] + BEST, "one GPU"),
                                        (["-s", SMALL, "--realign", "--best-overlaps", "-1"], ">=0"),
                                        (["-s", SMALL, "--realign", "--best-min-span", "100"], "--best-overlaps too"),
                                        (["-s", SMALL, "--realign", "--best-table", "t.tsv"], "--best-overlaps too"),
                                        (["-s", SMALL, "--realign", "--best-overlaps", "0", "--best-table", "t.tsv"], "--best-overlaps too"),
                                        (["-s", SMALL, "--best-min-span", "-1"] + BEST, ">=0"),
                                        (["-s", SMALL, "--best-table", ""] + BEST, "name of the file")])
def test_driver_refusals(tmp_path, flags, word):
    """One line and exit 1, before a handle exists."""
    p = subprocess.run([CLI] + flags, capture_output=True, timeout=60, cwd=tmp_path)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--best" in out and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "t.tsv").exists()


def test_driver_refuses_dat_input(tmp_path):
    (tmp_path / "reads.dat").write_bytes(b"")
    p = subprocess.run([CLI, "-s", "reads.dat"] + BEST, capture_output=True, timeout=60, cwd=tmp_path)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--best-overlaps" in out and ".dat" in out, (out, p.stderr[-500:])


def test_help_lists_the_flags():
    h = subprocess.run([CLI, "--help"], capture_output=True, timeout=60, text=True)
    assert h.returncode == 0 and all(f"\t{n}," in h.stdout for n in ("--best-overlaps", "--best-min-span", "--best-table"))


@pytest.mark.parametrize("tool,argv,word", [(best_overlaps, ["-n", "0"], "-n"), (best_overlaps, ["--min-span", "-1"], "--min-span"),
                                            (best_overlaps, ["--band", "-1"], "--band"),
                                            (correct, ["--best-overlaps", "-1"], "--best-overlaps"),
                                            (correct, ["--best-min-span", "100"], "--best-overlaps"),
                                            (correct, ["--best-overlaps", "3", "--best-min-span", "-1"], "--best-min-span")])
def test_tools_refuse_values(tool, argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        tool.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and word in capsys.readouterr().err
