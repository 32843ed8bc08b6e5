"""Read trimming without a GPU: the reference restatement (tests/trim_ref.py) against results written out by hand, every boundary of
the contract on a record of its own, mhap_trim_clip_record (host code of the library, the function the apply kernel runs) against
the reference, the properties of the rewrite rule, the tools' refusals, and the ideal-records experiment."""
import os
import subprocess

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, graph, trim, workloads

import trim_cases as tc
import trim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("to_rc", [0, 1])
def test_hand_worked_example(to_rc):
    records = tc.hand_records(to_rc)
    rows, flags, counts, cov = ref.trim(tc.HAND_IDS, tc.HAND_LEN, records, tc.HAND_P)
    assert [c.tolist() for c in cov] == tc.HAND_COV
    assert rows.tolist() == tc.HAND_ROWS and flags.tolist() == tc.HAND_FLAGS and counts == tc.HAND_COUNTS
    want = tc.HAND_CLIPPED0[to_rc]
    for kept, out in (ref.clip_record(records[0], rows[0, :2], rows[1, :2], tc.HAND_P),
                      api.trim_clip_record(records[0], rows[0, :2], rows[1, :2], **tc.HAND_P)):
        assert kept and tuple(int(out[k]) for k in ("a1", "a2", "alen", "b1", "b2", "blen")) == want
        assert all(out[k] == records[0][k] for k in ("from_id", "to_id", "score", "raw", "to_rc"))
    out, keep = ref.apply(tc.HAND_IDS, rows, flags, records, tc.HAND_P)
    assert keep.tolist() == tc.HAND_KEEP and out[2] == records[2] and out[0] == ref.clip_record(records[0], rows[0, :2], rows[1, :2], tc.HAND_P)[1]


def _cov_sums(records, P, n=2, length=40):
    """The covered positions (cov >= 1 counted with multiplicity) of reads 1 .. n of `length` bases, and the eligible records."""
    cov, el = ref.coverage(np.arange(1, n + 1), [length] * n, records, P)
    return [int(c.sum()) for c in cov], el


@pytest.mark.parametrize("to_rc", [0, 1])
def test_every_boundary_on_a_record_of_its_own(to_rc):
    P = ref.params(min_cov=1, end_clip=2, min_span=6)
    one = lambda **kw: tc.recs([tc.rec(1, 2, kw.pop("a1", 0), kw.pop("a2", 9), 40, kw.pop("b1", 0), kw.pop("b2", 9), 40, to_rc, **kw)])
    # span min_span - 1 gives nothing, span min_span gives its 2 positions; the two sides are judged on their own
    assert _cov_sums(one(a2=4, b2=4), P) == ([0, 0], 1)
    assert _cov_sums(one(a2=5, b2=4), P) == ([2, 0], 1)
    assert _cov_sums(one(a2=4, b1=30, b2=35), P) == ([0, 2], 1)
    # an interval of exactly 2 end_clip is empty, one of 2 end_clip + 1 holds one position
    Q = ref.params(min_cov=1, end_clip=5, min_span=6)
    assert _cov_sums(one(a1=3, a2=12, b1=3, b2=12), Q) == ([0, 0], 1)
    assert _cov_sums(one(a1=3, a2=13, b1=3, b2=12), Q) == ([1, 0], 1)
    cov, _ = ref.coverage([1, 2], [40, 40], one(a1=3, a2=13, b1=3, b2=12), Q)
    assert np.flatnonzero(cov[0]).tolist() == [8]
    # score 0, below min_identity and equal to it; from_id == to_id
    I = ref.params(min_cov=1, end_clip=2, min_span=6, min_identity=0.5)
    assert _cov_sums(one(score=0.0), I) == ([0, 0], 0)
    assert _cov_sums(one(score=0.4999), I) == ([0, 0], 0)
    assert _cov_sums(one(score=0.5), I) == ([6, 6], 1)
    same = tc.recs([tc.rec(1, 1, 0, 9, 40, 20, 29, 40, to_rc)])
    assert _cov_sums(same, P) == ([0, 0], 0)
    # the library's eligibility is the same rule
    full = np.array([0, 40], np.int32)
    for r, p, want in ((one(score=0.0), I, False), (one(score=0.4999), I, False), (one(score=0.5), I, True), (same, P, False), (one(), P, True)):
        assert api.trim_clip_record(r[0], full, full, **p)[0] == want == ref.clip_record(r[0], full, full, p)[0]


def test_tie_first_run_wins_and_runs_at_the_edges():
    P = ref.params(min_cov=1, end_clip=2, min_span=6)
    two = tc.recs([tc.rec(1, 2, 18, 27, 40, 0, 4, 40), tc.rec(1, 3, 0, 9, 40, 0, 4, 40)])     # read 1: [20, 26) and [2, 8)
    rows, flags, counts, _ = ref.trim([1, 2, 3], [40, 40, 40], two, P)
    assert rows[0].tolist() == [0, 10, 2, 12] and flags[0] == api.TRIM_CUT3 | api.TRIM_GAPPED
    assert flags[1] == flags[2] == api.TRIM_DELETED and rows[1].tolist() == [0, 0, 0, 0]
    assert counts["deleted"] == 2 and counts["gapped"] == 1 and counts["bases_kept"] == 10
    # a run at position 0 of the shrunk coverage (end_clip 0) and one that ends at length - end_clip
    Z = ref.params(min_cov=1, end_clip=0, min_span=6)
    rows, flags, _, _ = ref.trim([1, 2], [40, 40], tc.recs([tc.rec(1, 2, 0, 9, 40, 30, 39, 40)]), Z)
    assert rows.tolist() == [[0, 10, 1, 10], [30, 40, 1, 10]] and flags.tolist() == [api.TRIM_CUT3, api.TRIM_CUT5]
    rows, flags, _, _ = ref.trim([1, 2], [40, 40], tc.recs([tc.rec(1, 2, 30, 39, 40, 0, 39, 40)]), P)
    assert rows.tolist() == [[30, 40, 1, 6], [0, 40, 1, 36]] and flags.tolist() == [api.TRIM_CUT5, 0]
    for row, n in zip(rows.tolist(), [40, 40]):
        assert 0 <= row[0] <= row[1] <= n


def _random_records(rng, n):
    out, clears = [], []
    for _ in range(n):
        alen, blen = int(rng.integers(50, 400)), int(rng.integers(50, 400))
        a1, a2 = np.sort(rng.integers(0, alen, 2)).tolist()
        b1, b2 = np.sort(rng.integers(0, blen, 2)).tolist()
        score = float(rng.choice([0.0, 0.3, 0.5, 0.9]))
        frm, to = (7, 7) if rng.integers(0, 20) == 0 else (7, 8)
        out.append(tc.rec(frm, to, a1, a2, alen, b1, b2, blen, int(rng.integers(0, 2)), score))
        cl = []
        for L in (alen, blen):
            k = int(rng.integers(0, 6))
            cl.append((0, 0) if k == 0 else (0, L) if k == 1 else tuple(np.sort(rng.integers(0, L + 1, 2)).tolist()))
        clears.append(cl)
    return tc.recs(out), clears


def test_clip_record_matches_the_reference_on_random_records():
    rng = np.random.default_rng(5)
    records, clears = _random_records(rng, 4000)
    P = ref.params(min_identity=0.5)
    kept_lib = kept_ref = 0
    for r, (ca, cb) in zip(records, clears):
        kl, ol = api.trim_clip_record(r, ca, cb, **P)
        kr, orr = ref.clip_record(r, ca, cb, P)
        assert kl == kr and ol.tobytes() == orr.tobytes(), (r, ca, cb)
        kept_lib += kl
        kept_ref += kr
        if kl:
            assert 0 <= ol["a1"] <= ol["a2"] < ol["alen"] == ca[1] - ca[0] and 0 <= ol["b1"] <= ol["b2"] < ol["blen"] == cb[1] - cb[0]
    assert kept_lib == kept_ref and 500 < kept_lib < 3500


def test_identity_on_untouched_reads_and_mirror_property():
    rng = np.random.default_rng(6)
    records, clears = _random_records(rng, 1500)
    P = ref.params()
    n_id = n_mirror = 0
    for r, (ca, cb) in zip(records, clears):
        if ref.eligible(r, P):
            k, o = api.trim_clip_record(r, (0, r["alen"]), (0, r["blen"]), **P)
            assert k and o.tobytes() == r.tobytes()
            n_id += 1
        # B's coordinates reverse-complemented together with to_rc: the output is the mirror image on B and the same on A
        m = r.copy()
        m["b1"], m["b2"], m["to_rc"] = r["blen"] - 1 - r["b2"], r["blen"] - 1 - r["b1"], 1 - r["to_rc"]
        k0, o0 = api.trim_clip_record(r, ca, cb, **P)
        k1, o1 = api.trim_clip_record(m, ca, (r["blen"] - cb[1], r["blen"] - cb[0]), **P)
        assert k0 == k1
        if k0:
            assert (o1["a1"], o1["a2"], o1["alen"], o1["blen"]) == (o0["a1"], o0["a2"], o0["alen"], o0["blen"])
            assert (o1["b1"], o1["b2"]) == (o0["blen"] - 1 - o0["b2"], o0["blen"] - 1 - o0["b1"])
            n_mirror += 1
    assert n_id > 500 and n_mirror > 200


def test_reference_is_invariant_under_permutation_and_repeats_count_twice():
    ids, lengths, records, _ = tc.ideal_experiment(3, n_reads=60, genome=12000, n_chimeras=3)
    P = ref.params(min_cov=3, end_clip=100, min_span=500)
    rows, flags, counts, _ = ref.trim(ids, lengths, records, P)
    perm = np.random.default_rng(1).permutation(len(records))
    rows2, flags2, counts2, _ = ref.trim(ids, lengths, records[perm], P)
    assert rows.tolist() == rows2.tolist() and flags.tolist() == flags2.tolist() and counts == counts2
    cov1, _ = ref.coverage(ids, lengths, records[:50], P)
    cov2, el2 = ref.coverage(ids, lengths, np.concatenate([records[:50], records[:50]]), P)
    assert all((2 * a == b).all() for a, b in zip(cov1, cov2)) and el2 == 100


def test_ideal_records_split_every_chimera_and_spare_ordinary_reads():
    """The coverage rule on ideal records: a 20 kb circular genome, 170 reads of 2 500 - 3 500 bases, 12 planted two-piece chimeras,
    +-30 bases of noise on the interval ends; min_cov 3, end_clip 100, min_span 500.  Every chimera must be split and no ordinary read
    may lose more than 2 x noise bases."""
    noise, P = 30, ref.params(min_cov=3, end_clip=100, min_span=500)
    ids, lengths, records, junctions = tc.ideal_experiment(0, noise=noise)
    rows, flags, counts, _ = ref.trim(ids, lengths, records, P)
    assert len(junctions) == 12
    split = [r for r, j in junctions.items() if not tc.crosses(rows[r], j, P["end_clip"]) and not flags[r] & api.TRIM_DELETED]
    lost = [int(lengths[r]) - int(rows[r, 1] - rows[r, 0]) for r in range(len(ids)) if r not in junctions]
    print(f"split {len(split)} of {len(junctions)}; the most an ordinary read lost: {max(lost)}; {counts}")
    assert len(split) == 12
    assert all(flags[r] & api.TRIM_GAPPED for r in junctions)
    assert max(lost) <= 2 * noise
    for row, n in zip(rows.tolist(), lengths.tolist()):
        assert 0 <= row[0] <= row[1] <= n


@pytest.mark.parametrize("to_rc", [0, 1])
def test_refinement_by_hand_and_against_the_reference(to_rc):
    r, ops = tc.refine_record(to_rc), tc.encode(tc.REFINE_RUNS)
    for ok, out in (ref.refine_record(r, ops, 2), api.trim_refine_record(r, ops, 2)):
        assert ok and (out["a1"], out["a2"], out["b1"], out["b2"]) == tc.REFINE_WANT[to_rc] and out["score"] == 1.0 - 3 / 38
        assert all(out[k] == r[k] for k in ("from_id", "to_id", "raw", "alen", "blen", "to_rc"))
    # with a penalty of 1 the sum never falls to 0 (4, 1, 11, 10, 30, 28, 33, 25, 29): the stretch begins where the path does
    assert (api.trim_refine_record(r, ops, 1)[1]["a1"], api.trim_refine_record(r, ops, 1)[1]["a2"]) == (5, 47)
    # a path without a match column leaves the record as it is
    nothing = tc.encode([(3, "X"), (2, "D")])
    assert api.trim_refine_record(r, nothing, 2) == (False, r) and ref.refine_record(r, nothing, 2)[0] is False
    assert not api.trim_refine_record(r, nothing[:0], 2)[0]
    with pytest.raises(mhap_amd.MhapError):
        api.trim_refine_record(r, ops, 0)
    records, offs, ops = tc.random_paths(np.random.default_rng(8 + to_rc), 1500)
    n = 0
    for q, rec in enumerate(records):
        for pen in (1, 2, 3):
            got, want = api.trim_refine_record(rec, ops[offs[q]:offs[q + 1]], pen), ref.refine_record(rec, ops[offs[q]:offs[q + 1]], pen)
            assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes(), (q, pen)
            n += got[0]
    assert n > 3000


def test_plant_chimeras():
    fa = api.FastaData.from_strings(["ACGT" * 30, "TTGCA" * 30, "GGA" * 50, "CATG" * 40, "A" * 100])
    got, rows = workloads.plant_chimeras(fa, 2, seed=3)
    assert got.lengths.tolist() == fa.lengths.tolist() and got.offsets.tolist() == fa.offsets.tolist() and got.ids.tolist() == fa.ids.tolist()
    assert rows.shape == (2, 3) and len(set(rows[:, 0].tolist()) | set(rows[:, 2].tolist())) == 4
    for v, j, p in rows.tolist():
        L = int(fa.lengths[v])
        assert 2 * L // 5 <= j <= 3 * L // 5 or L - j == fa.lengths[p]
        assert got.sequence(v)[:j] == fa.sequence(v)[:j] and got.sequence(v)[j:] == fa.sequence(p)[-(L - j):]
    untouched = set(range(len(fa))) - set(rows[:, 0].tolist())
    assert all(got.sequence(i) == fa.sequence(i) for i in untouched)
    got2, rows2 = workloads.plant_chimeras(fa, 2, seed=3)
    assert rows2.tolist() == rows.tolist() and got2.bases.tobytes() == got.bases.tobytes()
    with pytest.raises(ValueError):
        workloads.plant_chimeras(fa, 3, seed=0)


def test_texts():
    assert api.trim_counts_line(range(1, 9)) == "Trim: 1 reads, 2 deleted, 3 cut at 5', 4 cut at 3', 5 gapped; 7 of 6 bases kept, 8 eligible overlaps"
    fa = api.FastaData.from_strings(["ACGTACGTAC", "GGGGG", "TTTTTTTT"])
    rows, flags = [[2, 7, 1, 3], [0, 0, 0, 0], [0, 8, 2, 4]], [6, 1, 8]
    assert trim.format_fasta(fa, rows, flags) == ">1 len=5 begin=2 end=7 runs=1\nGTACG\n>3 len=8 begin=0 end=8 runs=2\nTTTTTTTT\n"
    assert trim.format_table(fa.ids, fa.lengths, rows, flags) == "1\t10\t2\t7\t1\t3\t6\n2\t5\t0\t0\t0\t0\t1\n3\t8\t0\t8\t2\t4\t8\n"
    assert api.TRIM_COUNTS == ref.COUNTS and (api.TRIM_DELETED, api.TRIM_CUT5, api.TRIM_CUT3, api.TRIM_GAPPED) == (ref.DELETED, ref.CUT5, ref.CUT3, ref.GAPPED)


@pytest.mark.parametrize("argv", [["--min-cov", "0"], ["--end-clip", "-1"], ["--min-span", "-5"], ["--band", "-1"], ["--penalty", "-1"]])
def test_trim_tool_refuses_values(argv, capsys):
    with pytest.raises(SystemExit) as e:
        trim.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and argv[0] in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--trim-min-cov", "4"], ["--trim-end-clip", "100"], ["--trim-min-span", "500"], ["--trim-penalty", "3"], ["--trim", "--trim-min-cov", "0"], ["--trim", "--trim-penalty", "-1"]])
def test_graph_tool_refuses_flags(argv, capsys):
    with pytest.raises(SystemExit) as e:
        graph.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and "--trim" in capsys.readouterr().err


def _driver(tmp_path, flags):
    return subprocess.run([CLI] + flags, capture_output=True, timeout=60, cwd=tmp_path)


SMALL = os.path.join(GOLD, "small_reads.fasta")


@pytest.mark.parametrize("flags,word", [(["-s", SMALL, "--trim"], "--realign too"),
                                        (["-s", SMALL, "-q", SMALL, "--realign", "--trim"], "no -q"),
                                        (["-s", SMALL, "--realign", "--trim", "--gpus", "2"], "one GPU"),
                                        (["-s", SMALL, "--realign", "--trim-fasta", "t.fa"], "--trim too"),
                                        (["-s", SMALL, "--realign", "--trim-min-cov", "3"], "--trim too"),
                                        (["-s", SMALL, "--realign", "--trim-penalty", "2"], "--trim too"),
                                        (["-s", SMALL, "--realign", "--trim", "--trim-min-cov", "0"], ">=1"),
                                        (["-s", SMALL, "--realign", "--trim", "--trim-penalty", "-1"], ">=0"),
                                        (["-s", SMALL, "--realign", "--trim", "--trim-table", ""], "name of the file")])
def test_driver_refuses_flags(tmp_path, flags, word):
    p = _driver(tmp_path, flags)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--trim" in out and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "t.fa").exists()


def test_driver_refuses_dat_input(tmp_path):
    (tmp_path / "reads.dat").write_bytes(b"")
    p = _driver(tmp_path, ["-s", "reads.dat", "--realign", "--trim"])
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--trim" in out and ".dat" in out, (out, p.stderr[-500:])


def test_tools_list_the_flags_and_the_header_has_the_section():
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0
    assert all(f"\t{n}," in h.stdout for n in ("--trim", "--trim-min-cov", "--trim-end-clip", "--trim-min-span", "--trim-penalty", "--trim-fasta", "--trim-table"))
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = fh.read()
    assert f"#define MHAP_TRIM_COUNTS {len(ref.COUNTS)}\n" in text and f"#define MHAP_TRIM_TILE {api.TRIM_TILE}\n" in text and "read trimming" in text
    lib = api.load_library()
    assert all(getattr(lib, n) is not None for n in api.EXPORTED_SYMBOLS if n.startswith("mhap_trim_"))
    assert mhap_amd.TrimSession is api.TrimSession
