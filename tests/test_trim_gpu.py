"""Read trimming on the GPU (trim_kernels.hip) against tests/trim_ref.py, byte for byte: the add kernel's coverage, the run kernel's
rows, flags and counts at every edge of its tiles (MHAP_TRIM_TILE positions, four loads of 1 024 per tile, 256 per wave and load),
the apply kernel's records, the session's refusals, and one end-to-end case with planted chimeras through the library, the driver
and the tools."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, trim, workloads
from mhap_amd.correct import select_paths
from mhap_amd.realign import kept_rows, read_overlaps

import trim_cases as tc
import trim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
pytestmark = pytest.mark.gpu
T = api.TRIM_TILE


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _check(ts, ids, lengths, records, P, coverage_of=None):
    """A finish of `ts` against the reference on `records`: counts, rows, flags, and the coverage of the reads asked for."""
    counts = ts.finish()
    rows, flags = ts.table()
    erows, eflags, ecounts, ecov = ref.trim(ids, lengths, records, P)
    assert counts == ecounts
    assert rows.dtype == np.int32 and flags.dtype == np.uint8 and rows.tobytes() == erows.tobytes() and flags.tobytes() == eflags.tobytes()
    for r in (range(len(ids)) if coverage_of is None else coverage_of):
        assert ts.coverage(r).tobytes() == ecov[r].astype(np.int32).tobytes(), r
    for row, n in zip(rows.tolist(), np.asarray(lengths).tolist()):     # the clear range lies in the read by construction: nothing clamps
        assert 0 <= row[0] <= row[1] <= n
    return rows, flags, counts


@pytest.mark.parametrize("to_rc", [0, 1])
def test_hand_worked_example(ms, to_rc):
    records = tc.hand_records(to_rc)
    with api.TrimSession(tc.HAND_IDS, tc.HAND_LEN, handle=ms, **tc.HAND_P) as ts:
        ts.add(records)
        rows, flags, counts = _check(ts, tc.HAND_IDS, tc.HAND_LEN, records, tc.HAND_P)
        assert rows.tolist() == tc.HAND_ROWS and flags.tolist() == tc.HAND_FLAGS and counts == tc.HAND_COUNTS
        assert [ts.coverage(r).tolist() for r in range(3)] == tc.HAND_COV
        out, keep = ts.apply(records)
        assert keep.tolist() == tc.HAND_KEEP and out[2] == records[2]
        assert tuple(int(out[0][k]) for k in ("a1", "a2", "alen", "b1", "b2", "blen")) == tc.HAND_CLIPPED0[to_rc]


def _random_records(rng, ids, lengths, n, span_max=3000):
    """Records between random pairs of reads of at least 20 bases, with intervals of every size up to span_max."""
    ok = np.flatnonzero(np.asarray(lengths) >= 20)
    out = []
    for _ in range(n):
        x, y = rng.choice(ok, 2, replace=False).tolist()
        iv = []
        for L in (int(lengths[x]), int(lengths[y])):
            n1 = int(rng.integers(1, min(L, span_max) + 1))
            s = int(rng.integers(0, L - n1 + 1))
            iv += [s, s + n1 - 1]
        out.append(tc.rec(int(ids[x]), int(ids[y]), iv[0], iv[1], int(lengths[x]), iv[2], iv[3], int(lengths[y]), int(rng.integers(0, 2)),
                          float(rng.choice([0.0, 0.4, 0.7, 0.9]))))
    return tc.recs(out)


def test_read_lengths_round_the_tile_size_and_apply(ms):
    """Reads of length 0, 1, 2 end_clip, T - 1, T, T + 1 and 2 T + 1 in one table under random records; then the apply kernel on the
    same records and on void ones against the reference."""
    P = ref.params(min_cov=2, end_clip=5, min_span=12, min_identity=0.5)
    lengths = np.array([0, 1, 10, T - 1, T, T + 1, 2 * T + 1, 700, 20], np.int32)
    ids = np.arange(11, 11 + len(lengths), dtype=np.int64)
    rng = np.random.default_rng(7)
    records = _random_records(rng, ids, lengths, 150)
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
        ts.add(records)
        rows, flags, counts = _check(ts, ids, lengths, records, P)
        assert counts["deleted"] >= 3 and counts["gapped"] >= 1 and 0 < counts["eligible_records"] < len(records)
        extra = tc.recs([tc.rec(14, 14, 0, 99, T - 1, 100, 199, T - 1), tc.rec(14, 15, 0, 0, T - 1, 0, 0, T, 0, 0.0),
                         tc.rec(13, 14, 0, 9, 10, 0, 99, T - 1), tc.rec(14, 16, 0, T - 2, T - 1, 1, T - 1, T + 1, 1)])
        both = np.concatenate([records, extra])
        out, keep = ts.apply(both)
        eout, ekeep = ref.apply(ids, rows, flags, both, P)
        assert keep.tobytes() == ekeep.tobytes() and out.tobytes() == eout.tobytes()
        assert 0 < int(keep.sum()) < len(both) and keep[-4:-1].tolist() == [0, 0, 0]
        assert ts.apply(both[:0])[0].shape == (0,)


# interval lists on a read of 3 T + 100 positions, min_cov 1, end_clip 0, min_span 1: every interval is a run as it stands
EDGE = 3 * T + 100
EDGE_CASES = {
    "ends on the last position of a tile": [(T - 96, T)],
    "begins on the first position of a tile": [(T, T + 104)],
    "one position apart across a tile edge": [(T - 96, T), (T + 1, T + 104)],
    "spans three tiles": [(T - 1000, 3 * T + 50)],
    "wholly in the last 16 positions of a tile": [(T - 16, T)],
    "wholly in the last lane's last word": [(2 * T - 4, 2 * T - 1)],
    "equal runs in different tiles": [(100, 600), (T + 900, T + 1400)],
    "equal runs, three tiles": [(2 * T + 7, 2 * T + 57), (T + 7, T + 57), (7, 57)],
    "a better run after an open run carried over the edge": [(T - 96, T + 104), (T + 300, T + 1000)],
    "an open run carried over the edge beats a later one": [(T - 1000, T + 200), (T + 300, T + 400)],
    "a run to the very end": [(3 * T, EDGE)],
    "a run from the very start": [(0, 1)],
    "the whole read": [(0, EDGE)],
    "across a load of 1024 and a wave of 256": [(1000, 1024), (1024 + 256 - 3, 1024 + 256 + 3), (2048, 2049)],
    "runs in every tile": [(k * 512 + 10, k * 512 + 300) for k in range(24)],
    "single positions at every word edge": [(p, p + 1) for p in (3, 4, 255, 256, 1023, 1024, T - 1, T, T + 3, 2 * T - 1, 2 * T, EDGE - 1)],
}


@pytest.mark.parametrize("end_clip", [0, 3])
def test_runs_at_every_tile_edge(ms, end_clip):
    """One read per case of EDGE_CASES and a short partner; with end_clip 3 every interval is given 3 wider at both ends where
    the read has room, so the runs are the same and the clear ranges are 3 wider."""
    P = ref.params(min_cov=1, end_clip=end_clip, min_span=1)
    names = list(EDGE_CASES)
    lengths = np.array([EDGE] * len(names) + [50], np.int32)
    ids = np.arange(1, len(lengths) + 1, dtype=np.int64)
    partner = int(ids[-1])
    records = []
    for k, name in enumerate(names):
        for s, e in EDGE_CASES[name]:
            s, e = s - end_clip, e + end_clip
            if s < 0 or e > EDGE:
                continue     # (no room: the case keeps its other runs)
            records.append(tc.rec(int(ids[k]), partner, s, e - 1, EDGE, 0, 2 * end_clip, 50, k & 1))
    records = tc.recs(records)
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
        ts.add(records)
        rows, flags, _ = _check(ts, ids, lengths, records, P, coverage_of=[0, 3, len(names) - 2])
        if end_clip == 0:     # what the cases are named after, written out
            by = dict(zip(names, rows.tolist()))
            assert by["ends on the last position of a tile"] == [T - 96, T, 1, 96]
            assert by["one position apart across a tile edge"] == [T + 1, T + 104, 2, 199]
            assert by["spans three tiles"] == [T - 1000, 3 * T + 50, 1, 2 * T + 1050]
            assert by["equal runs in different tiles"] == [100, 600, 2, 1000]
            assert by["equal runs, three tiles"] == [7, 57, 3, 150]
            assert by["a better run after an open run carried over the edge"] == [T + 300, T + 1000, 2, 900]
            assert by["an open run carried over the edge beats a later one"] == [T - 1000, T + 200, 2, 1300]
            assert by["a run to the very end"] == [3 * T, EDGE, 1, 100] and by["the whole read"] == [0, EDGE, 1, EDGE]
            assert by["runs in every tile"] == [10, 300, 24, 24 * 290]
            assert by["single positions at every word edge"] == [3, 5, 7, 12]


def test_seventy_thousand_records_on_one_read(ms):
    """The per-base counters are not 16 bits wide: 70 000 identical records reach a min_cov of 66 000."""
    P = ref.params(min_cov=66000, end_clip=10, min_span=100)
    ids, lengths = np.array([5, 6], np.int64), np.array([5000, 300], np.int32)
    records = np.repeat(tc.recs([tc.rec(5, 6, 4000, 4199, 5000, 50, 249, 300, 1)]), 70000)
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
        ts.add(records)
        rows, flags, counts = _check(ts, ids, lengths, records, P)
        assert rows.tolist() == [[4000, 4200, 1, 180], [50, 250, 1, 180]] and counts["eligible_records"] == 70000
        assert int(ts.coverage(0).max()) == 70000 and int(ts.coverage(1)[60]) == 70000


def test_split_adds_and_a_repeated_finish(ms):
    P = ref.params(min_cov=3, end_clip=20, min_span=100)
    rng = np.random.default_rng(11)
    lengths = rng.integers(300, 9000, 40).astype(np.int32)
    ids = np.arange(100, 140, dtype=np.int64)
    records = _random_records(rng, ids, lengths, 6000, span_max=2500)
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
        with pytest.raises(mhap_amd.MhapError):
            ts.table()                                      # no finish yet
        ts.add(records[:0])
        for q0 in range(0, 3000, 700):
            ts.add(records[q0:min(q0 + 700, 3000)])
        half = _check(ts, ids, lengths, records[:3000], P, coverage_of=[0, 17])
        again = _check(ts, ids, lengths, records[:3000], P, coverage_of=[])          # a finish may be repeated
        assert again[0].tobytes() == half[0].tobytes() and again[2] == half[2]
        ts.add(records[3000:])
        whole = _check(ts, ids, lengths, records, P, coverage_of=[0, 17])            # and records may follow it
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:                        # any order, one call
        ts.add(records[rng.permutation(len(records))])
        one = _check(ts, ids, lengths, records, P, coverage_of=[])
    assert one[0].tobytes() == whole[0].tobytes() and one[1].tobytes() == whole[1].tobytes() and one[2] == whole[2]


def test_refused_calls_add_nothing(ms):
    P = ref.params(min_cov=1, end_clip=0, min_span=1)
    ids, lengths = np.array([1, 2], np.int64), np.array([100, 200], np.int32)
    good = tc.rec(1, 2, 10, 59, 100, 20, 69, 200)
    with api.TrimSession(ids, lengths, handle=ms, **P) as ts:
        for bad, word in ((tc.rec(1, 3, 10, 59, 100, 20, 69, 200), "not among the reads"), (tc.rec(1, 2, 10, 59, 101, 20, 69, 200), "the length 101"),
                          (tc.rec(1, 2, 10, 100, 100, 20, 69, 200), "100 bases"), (tc.rec(1, 2, 10, 59, 100, -1, 69, 200), "200 bases"),
                          (tc.rec(1, 2, 60, 59, 100, 20, 69, 200), "100 bases")):
            with pytest.raises(mhap_amd.MhapError) as e:
                ts.add(tc.recs([good, good, bad]))
            assert "record 2" in str(e.value) and word in str(e.value)
        counts = ts.finish()
        assert counts["eligible_records"] == 0 and counts["deleted"] == 2 and not ts.coverage(0).any() and not ts.coverage(1).any()
        with pytest.raises(mhap_amd.MhapError):
            ts.apply(tc.recs([tc.rec(1, 3, 10, 59, 100, 20, 69, 200)]))
        with pytest.raises(mhap_amd.MhapError):
            ts.coverage(2)
        ts.add(tc.recs([good]))
        _check(ts, ids, lengths, tc.recs([good]), P)
    for kw in (dict(min_cov=0), dict(end_clip=-1), dict(min_span=-1)):
        with pytest.raises(mhap_amd.MhapError):
            api.TrimSession(ids, lengths, handle=ms, **kw)
    with api.TrimSession(ids[:0], lengths[:0], handle=ms) as ts:     # no reads at all
        assert ts.finish()["reads"] == 0 and ts.table()[0].shape == (0, 4)


def test_refine_kernel_against_the_reference(ms):
    """mhap_trim_refine on random paths, records without a path among them, for three penalties; and the worked example."""
    records, offs, ops = tc.random_paths(np.random.default_rng(21), 3000)
    assert (np.diff(offs) == 0).sum() > 20
    for pen in (1, 2, 3):
        got = api.trim_refine(records, offs, ops, penalty=pen, handle=ms)
        assert got.tobytes() == ref.refine(records, offs, ops, pen).tobytes()
    for to_rc in (0, 1):
        r = tc.recs([tc.refine_record(to_rc)])
        out = api.trim_refine(r, [0, len(tc.REFINE_RUNS)], tc.encode(tc.REFINE_RUNS), handle=ms)[0]
        assert (out["a1"], out["a2"], out["b1"], out["b2"]) == tc.REFINE_WANT[to_rc] and out["score"] == 1.0 - 3 / 38
    assert api.trim_refine(records[:0], offs[:1], ops[:0], handle=ms).shape == (0,)
    for bad in (dict(penalty=0), dict(op_offsets=offs[:-1])):
        with pytest.raises(mhap_amd.MhapError):
            api.trim_refine(records, bad.get("op_offsets", offs), ops, penalty=bad.get("penalty", 2), handle=ms)


# ---- end to end: a drawn genome, reads at 10 % error, planted chimeras --------------------------------------------------------------
E2E_P = dict(min_cov=3, end_clip=100, min_span=500)
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]
TRIM_FLAGS = ["--trim", "--trim-end-clip", "100", "--trim-min-span", "500"]


def _unitig_line(stderr):
    return [l for l in stderr.split("\n") if l.startswith("Unitigs: ")]


class E2E:
    """Reads of 2 500 - 3 500 bases at 10 % error, about 25 x over a drawn circular genome of 20 kb, 12 of them made chimeric by
    workloads.plant_chimeras; the driver's plain overlaps of them, realigned and trimmed through the library with end_clip 100 and
    min_span 500, and the reference on the GPU's own records."""

    def __init__(self, tmp):
        rng = np.random.default_rng(41)
        codes = rng.integers(0, 4, 20000).astype(np.uint8)
        plain = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 170).astype(np.int32), seed=9, error_rate=0.10)
        self.tmp = tmp
        self.fa, self.junctions = workloads.plant_chimeras(plain, 12, seed=5)
        self.fasta = str(tmp / "reads.fasta")
        with open(self.fasta, "w") as fh:
            for i in range(len(self.fa)):
                fh.write(f">read{i}\n{self.fa.sequence(i)}\n")
        run = subprocess.run([CLI, "-s", self.fasta], capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        self.overlaps = str(tmp / "ovl.txt")
        with open(self.overlaps, "wb") as fh:
            fh.write(run.stdout)
        found = read_overlaps(self.overlaps)
        self.res = trim.trim_overlaps(found, self.fa, **E2E_P)
        self.unrefined = trim.trim_overlaps(found, self.fa, penalty=0, **E2E_P)
        self.P = ref.params(**E2E_P)
        self.rows, self.flags, self.counts, _ = ref.trim(self.fa.ids, self.fa.lengths, self.res["records"], self.P)
        with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:     # the refined records from the reference
            out, _, offs, ops = api.realign_records_paths(found, self.fa, handle=h)
        rows = kept_rows(out)
        self.refined = ref.refine(out[rows], *select_paths(offs, ops, rows), api.TRIM_PENALTY)

    def still_crossed(self, rows, flags):
        return [v for v, j, _ in self.junctions.tolist() if not flags[v] & ref.DELETED and tc.crosses(rows[v], j, self.P["end_clip"])]


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return E2E(tmp_path_factory.mktemp("trim_e2e"))


def test_end_to_end_table_driver_and_tools(e2e):
    """The GPU's table is the reference's on the GPU's own records, the rewritten records and the trimmed reads follow it, and the
    driver and the tools write the same files; without --trim nothing of the trimming shows."""
    fa, res, erows, eflags, ecounts, P, tmp_path, fasta = e2e.fa, e2e.res, e2e.rows, e2e.flags, e2e.counts, e2e.P, e2e.tmp, e2e.fasta
    assert res["rows"].tobytes() == erows.tobytes() and res["flags"].tobytes() == eflags.tobytes() and res["counts"] == ecounts
    assert ecounts["eligible_records"] > 1000
    assert res["records"].tobytes() == e2e.refined.tobytes()                      # the records the table stands on: the reference's refinement
    assert e2e.unrefined["records"].tobytes() != res["records"].tobytes()
    eout, ekeep = ref.apply(fa.ids, erows, eflags, res["records"], P)
    assert res["applied"].tobytes() == eout[ekeep != 0].tobytes()
    cut = res["reads"]
    live = np.flatnonzero((eflags & ref.DELETED) == 0)
    assert cut.ids.tolist() == fa.ids[live].tolist() and cut.lengths.tolist() == (erows[live, 1] - erows[live, 0]).tolist()
    assert np.shares_memory(cut.bases, fa.bases)
    assert all(cut.sequence(k) == fa.sequence(r)[erows[r, 0]:erows[r, 1]] for k, r in enumerate(live.tolist()))
    # the driver: stdout is what it is without --trim, the table and the trimmed reads are the library's, the graph is built on them
    g0, u0, g1, u1, tf, tt = (str(tmp_path / n) for n in ("plain.gfa", "plain.utg.gfa", "trim.gfa", "trim.utg.gfa", "trim.fasta", "trim.tsv"))
    r0 = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", g0, "--gfa-unitigs", u0] + SCALED, capture_output=True, timeout=600)
    r1 = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", g1, "--gfa-unitigs", u1] + SCALED + TRIM_FLAGS + ["--trim-fasta", tf, "--trim-table", tt],
                        capture_output=True, timeout=600)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    assert b"Trim" not in r0.stderr and b"--trim" not in r0.stderr
    assert sorted(r1.stdout.split(b"\n")) == sorted(r0.stdout.split(b"\n"))
    e1 = r1.stderr.decode()
    assert [l for l in e1.split("\n") if l.startswith("Trim: ")] == [api.trim_counts_line([ecounts[k] for k in api.TRIM_COUNTS])]
    assert open(tt).read() == trim.format_table(fa.ids, fa.lengths, erows, eflags)
    assert open(tf).read() == trim.format_fasta(fa, erows, eflags)
    gfa = open(g1).read()
    assert all(f"S\t{i}\t" not in gfa for i in fa.ids[(eflags & ref.DELETED) != 0].tolist())
    by_id = dict(zip(cut.ids.tolist(), cut.lengths.tolist()))
    for l in gfa.split("\n"):
        if l.startswith("S\t"):
            assert l.split("\t")[3] == f"LN:i:{by_id[int(l.split(chr(9))[1])]}"
    print(f"without --trim: {_unitig_line(r0.stderr.decode())}; with: {_unitig_line(e1)}")
    # the tools write the same files from the driver's plain overlaps
    pf, pt, pg, pu = (str(tmp_path / n) for n in ("tool.fasta", "tool.tsv", "tool.gfa", "tool.utg.gfa"))
    p = subprocess.run([sys.executable, "-m", "mhap_amd.trim", e2e.overlaps, fasta, "--end-clip", "100", "--min-span", "500", "-o", pf,
                        "--table", pt, "--records", str(tmp_path / "tool.txt")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(pf).read() == open(tf).read() and open(pt).read() == open(tt).read()
    assert sorted(open(tmp_path / "tool.txt").read().split("\n")) == sorted([""] + api.records_to_lines(res["applied"]))
    p = subprocess.run([sys.executable, "-m", "mhap_amd.graph", e2e.overlaps, fasta, "--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300",
                        "-o", pg, "--unitigs", pu, "--trim", "--trim-end-clip", "100", "--trim-min-span", "500"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert open(pg).read() == gfa and open(pu).read() == open(u1).read()
    assert [l for l in p.stderr.split("\n") if l.startswith("Trim: ")] == [l for l in e1.split("\n") if l.startswith("Trim: ")]


def test_end_to_end_at_most_five_junctions_still_crossed(e2e):
    """Untrimmed, all 12 clear ranges cross their junction by construction; at most 5 may still cross after trimming.  The figures of
    the same records as realigned, not cut to their best stretch (penalty 0), are printed next to those of the default: there the
    aligner's overlaps run through every junction and none is split (EXPERIMENTS.md, "Read trimming")."""
    fa, junctions, P = e2e.fa, e2e.junctions, e2e.P
    assert len(junctions) == 12 and len(e2e.still_crossed(np.stack([np.zeros_like(fa.lengths), fa.lengths], 1), np.zeros(len(fa), np.uint8))) == 12
    ordinary = sorted(set(range(len(fa))) - set(junctions[:, 0].tolist()))
    for name, res in (("as realigned (penalty 0)", e2e.unrefined), (f"refined (penalty {api.TRIM_PENALTY})", e2e.res)):
        rows, flags, counts = res["rows"], res["flags"], res["counts"]
        lost = [int(fa.lengths[r]) - int(rows[r, 1] - rows[r, 0]) for r in ordinary]
        print(f"{name}: {api.trim_counts_line([counts[k] for k in api.TRIM_COUNTS])} | {12 - len(e2e.still_crossed(rows, flags))} of 12 junctions "
              f"split; ordinary reads: {sum(1 for x in lost if x > 0)} trimmed, {sum(1 for x in lost if x > 200)} by more than 200 bases, most {max(lost)}")
    assert len(e2e.still_crossed(e2e.rows, e2e.flags)) <= 5
