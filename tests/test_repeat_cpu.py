"""Repeat marking without a GPU: the restatement tests/repeat_ref.py against tables worked out by hand, the host entry point
mhap_repeat_judge_record against the restatement on crafted interval lists, and the condition test — on exact records over a genome
with four copies of a repeat, every false record is void and no true record with a good anchor is."""
import os
import subprocess

import numpy as np
import pytest

from mhap_amd import api, graph, repeats, trim

import repeat_cases as rc
import repeat_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
SMALL = os.path.join(ROOT, "tests", "golden", "small_reads.fasta")


@pytest.mark.parametrize("name", list(rc.HAND))
def test_restatement_against_hand_computed_tables(name):
    ids, lengths, records, c = rc.hand_case(name)
    P = ref.params(**c["P"])
    m = ref.mark(ids, lengths, records, P)
    assert (m["counts"]["depth"], m["counts"]["threshold"]) == (c["D"], c["T"])
    got = [[tuple(x) for x in m["intervals"][m["offsets"][r]:m["offsets"][r + 1]].tolist()] for r in range(len(ids))]
    assert got == c["intervals"]
    assert m["counts"]["eligible_records"] == len(records) and m["counts"]["intervals"] == sum(len(x) for x in c["intervals"])
    assert int(m["hist"].sum()) == int(lengths.sum()) and m["counts"]["bases"] == int(lengths.sum())
    for r, iv in enumerate(c["intervals"]):
        assert m["rows"][r].tolist()[:2] == [len(iv), sum(e - s for s, e in iv)] and m["rows"][r, 3] == (iv[0][0] if iv else -1)
        assert m["flags"][r] == (ref.SOME if iv else 0) | (ref.WHOLE if iv == [(0, int(lengths[r]))] else 0)


def test_restatement_whole_read_row_and_flags():
    ids, lengths, records, c = rc.hand_case("the whole read")
    m = ref.mark(ids, lengths, records, ref.params(**c["P"]))
    assert m["rows"].tolist() == [[1, 8, 5, 0], [0, 0, 1, -1], [0, 0, 6, -1]] and m["flags"].tolist() == [ref.SOME | ref.WHOLE, 0, 0]
    assert m["counts"] == dict(reads=3, reads_with_interval=1, whole_reads=1, intervals=1, repeat_bases=8, bases=59, eligible_records=6,
                               depth=1, threshold=2)
    assert m["hist"][[0, 1, 5, 6]].tolist() == [0, 50, 8, 1]


def test_restatement_clamped_last_bin_and_its_refusal():
    ids, lengths, records = rc.clamp_case(5000)
    cov, n_el = ref.coverage(ids, lengths, records, ref.params())
    assert n_el == 5000 and cov[0].tolist() == [5000] * 3
    hist = ref.histogram(cov)
    assert hist[ref.BINS - 1] == 6 and int(hist.sum()) == 6 and ref.depth(hist) == ref.BINS - 1
    with pytest.raises(ref.NeedMaxCov):
        ref.mark(ids, lengths, records, ref.params())
    m = ref.mark(ids, lengths, records, ref.params(max_cov=4999, min_run=3))     # given, the threshold is exact above the clamp
    assert m["intervals"].tolist() == [[0, 3], [0, 3]] and m["rows"][0].tolist() == [1, 3, 5000, 0]
    assert ref.mark(ids, lengths, records, ref.params(max_cov=5000, min_run=1))["counts"]["intervals"] == 0
    # one below the last bin is no refusal
    ids, lengths, records = rc.clamp_case(ref.BINS - 2)
    assert ref.mark(ids, lengths, records, ref.params())["counts"]["depth"] == ref.BINS - 2


def test_bad_parameters_are_refused():
    for kw in (dict(factor_pct=99), dict(max_cov=-1), dict(min_run=0), dict(min_unique=-1)):
        with pytest.raises(ValueError):
            ref.params(**kw)
        with pytest.raises(api.MhapError):
            api.repeat_judge_record(rc.judge_records()[0][0], [], [], **kw)


def test_host_judgement_against_restatement_and_hand_values():
    P = ref.params(**rc.JUDGE_P)
    cases = rc.judge_records()
    assert len(cases) == 25
    for record, keep, ua, ub in cases:
        iva, ivb = rc.JUDGE_IV[int(record["from_id"])], rc.JUDGE_IV[int(record["to_id"])]
        want = ref.judge_record(record, iva, ivb, P)
        assert want == (keep, ua, ub), record
        got = api.repeat_judge_record(record, iva, ivb, **rc.JUDGE_P)
        assert (int(got[0]), got[1], got[2]) == want, record
    assert api.repeat_judge_record(cases[0][0], [], [], **rc.JUDGE_P) == (True, 1000, 1000)     # reads without intervals
    for bad in ([(5, 5)], [(10, 20), (15, 30)], [(0, 20001)], [(30, 40), (10, 20)]):               # empty, overlapping, outside, descending
        with pytest.raises(api.MhapError):
            api.repeat_judge_record(cases[0][0], bad, [], **rc.JUDGE_P)


def test_counts_line():
    line = api.repeat_counts_line([10, 3, 1, 4, 2000, 90000, 77, 20, 40])
    assert line == ("Repeats: 10 reads, 3 with a repeat, 1 repeat throughout; 4 intervals, 2000 of 90000 bases; 77 eligible overlaps, "
                    "depth 20, threshold 40")


@pytest.mark.parametrize("seed", range(6))
def test_condition_four_copies_default_parameters(seed):
    """Every false record is void, and no true record whose anchor outside the copies is at least min_unique + 500 is."""
    ids, lengths, records, false, anchor = rc.generate(seed)
    P = ref.params()
    m = ref.mark(ids, lengths, records, P)
    keep, unique = ref.apply(ids, m["offsets"], m["intervals"], records, P)
    lost = int(((keep == 0) & ~false & (anchor >= P["min_unique"] + 500)).sum())
    print(f"seed {seed}: {len(ids)} reads, {int((~false).sum())} true and {int(false.sum())} false records, D {m['counts']['depth']}, "
          f"T {m['counts']['threshold']}, {m['counts']['intervals']} intervals; false kept {int((keep[false] != 0).sum())}, "
          f"true with a good anchor void {lost}, true void in all {int(((keep == 0) & ~false).sum())}")
    assert false.sum() > 100 and (~false).sum() > 3000
    assert not keep[false].any()
    assert lost == 0


@pytest.mark.parametrize("flags,word", [(["-s", SMALL, "--repeat-filter"], "--realign too"),
                                        (["-s", SMALL, "-q", SMALL, "--realign", "--repeat-filter"], "no -q"),
                                        (["-s", SMALL, "--realign", "--repeat-filter", "--gpus", "2"], "one GPU"),
                                        (["-s", SMALL, "--realign", "--repeat-factor", "150"], "--repeat-filter too"),
                                        (["-s", SMALL, "--realign", "--repeat-table", "t.tsv"], "--repeat-filter too"),
                                        (["-s", SMALL, "--realign", "--repeat-filter", "--repeat-factor", "99"], ">=100"),
                                        (["-s", SMALL, "--realign", "--repeat-filter", "--repeat-min-run", "0"], ">=1"),
                                        (["-s", SMALL, "--realign", "--repeat-filter", "--trim-penalty", "-1"], ">=0"),
                                        (["-s", SMALL, "--realign", "--repeat-filter", "--repeat-table", ""], "name of the file")])
def test_driver_refuses_flags_wherever_trim_is_refused(tmp_path, flags, word):
    """One line and exit 1, before a handle exists."""
    p = subprocess.run([CLI] + flags, capture_output=True, timeout=60, cwd=tmp_path)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--repeat" in out and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "t.tsv").exists()


def test_driver_refuses_dat_input(tmp_path):
    (tmp_path / "reads.dat").write_bytes(b"")
    p = subprocess.run([CLI, "-s", "reads.dat", "--realign", "--repeat-filter"], capture_output=True, timeout=60, cwd=tmp_path)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--repeat-filter" in out and ".dat" in out, (out, p.stderr[-500:])


@pytest.mark.parametrize("tool,argv", [(repeats, ["--factor", "99"]), (repeats, ["--min-run", "0"]), (repeats, ["--max-cov", "-1"]), (repeats, ["--min-unique", "-1"]),
                                       (graph, ["--repeat-factor", "150"]), (graph, ["--repeat-filter", "--repeat-min-run", "0"]),
                                       (trim, ["--repeat-min-unique", "100"]), (trim, ["--repeat-filter", "--repeat-factor", "50"])])
def test_tools_refuse_values(tool, argv, capsys):
    with pytest.raises(SystemExit) as e:
        tool.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and argv[-2].lstrip("-").split("-")[0] in capsys.readouterr().err


def test_table_text():
    assert repeats.format_table([7, 8, 9], [0, 2, 2, 3], [[1, 5], [10, 20], [0, 4]]) == "7\t1\t5\n7\t10\t20\n9\t0\t4\n"
