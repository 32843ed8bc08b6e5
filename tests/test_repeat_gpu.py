"""Repeat marking on the GPU (repeat_kernels.hip) against tests/repeat_ref.py, byte for byte: rows, flags, offsets, intervals,
histogram, counts, keep bytes and uA / uB — at every read length round the tile size, with runs laid against every tile edge, with
more intervals in a tile than the workgroup has lanes, past the 1 024-entry step of the prefix sum, above the clamp of the
histogram, under any order and split of the records — then the crafted judgements, the refusals, the generator of
tests/repeat_cases.py, and one case end to end through the Python pipeline, the driver and the tools."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, graph, repeats
from mhap_amd.realign import read_overlaps

import repeat_cases as rc
import repeat_ref as ref
import trim_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
pytestmark = pytest.mark.gpu
T = api.TRIM_TILE     # the tile of the shared pile-up: 4 096 positions


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _same(rs, m):
    """The last finish of `rs` and its tables against the restatement's dict `m`, byte for byte."""
    rows, flags, offsets, iv = rs.table()
    assert rs.counts == m["counts"]
    assert (rows.dtype, flags.dtype, offsets.dtype, iv.dtype) == (np.int32, np.uint8, np.int64, np.int32)
    assert offsets.tobytes() == m["offsets"].tobytes()
    assert iv.tobytes() == m["intervals"].tobytes()
    assert rows.tobytes() == m["rows"].tobytes() and flags.tobytes() == m["flags"].tobytes()
    assert rs.histogram().tobytes() == m["hist"].tobytes()
    return rows, flags, offsets, iv


def _check(ms, ids, lengths, records, P, apply_to=None):
    m = ref.mark(ids, lengths, records, P)
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:
        rs.add(records)
        rs.finish()
        _same(rs, m)
        if apply_to is not None:
            keep, unique = rs.apply(apply_to)
            ekeep, eunique = ref.apply(ids, m["offsets"], m["intervals"], apply_to, P)
            assert keep.tobytes() == ekeep.tobytes() and unique.tobytes() == eunique.tobytes()
    return m


@pytest.mark.parametrize("name", list(rc.HAND))
def test_hand_computed_tables(ms, name):
    ids, lengths, records, c = rc.hand_case(name)
    m = _check(ms, ids, lengths, records, ref.params(**c["P"]), apply_to=records)
    assert (m["counts"]["depth"], m["counts"]["threshold"]) == (c["D"], c["T"])


def _random_records(rng, ids, lengths, n, span_max=3000):
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
    return out


def test_read_lengths_round_the_tile_size(ms):
    """Reads of 0, 1, 3, 4, 5, T - 1, T, T + 1, 2 T, 2 T + 1 and 3 T + 5 bases in one table: random records on the longer ones, whole-read
    records on the short ones; the threshold derived (factor 120) and given."""
    lengths = np.array([0, 1, 3, 4, 5, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 700, 20], np.int32)
    ids = np.arange(11, 11 + len(lengths), dtype=np.int64)
    rng = np.random.default_rng(7)
    out = _random_records(rng, ids, lengths, 400)
    for r in (1, 2, 3, 4):     # the short reads, whole, at depths 1 .. 8
        out += [tc.rec(int(ids[r]), int(ids[11]), 0, int(lengths[r]) - 1, int(lengths[r]), 10 * r, 10 * r + 5, 700)] * (2 * r)
    records = tc.recs(out)
    for kw in (dict(factor_pct=120, min_run=3, min_identity=0.5), dict(max_cov=3, min_run=1), dict(factor_pct=100, min_run=40, min_unique=30)):
        m = _check(ms, ids, lengths, records, ref.params(**kw), apply_to=records)
        assert m["counts"]["intervals"] > 5 and 0 < m["counts"]["eligible_records"] < len(records)


# interval lists on a read of 3 T + 100 positions; every interval is piled up twice and max_cov is 1, so each is a run as it stands
EDGE = 3 * T + 100
MIN_RUN = 50
EDGE_CASES = {
    "begins at 0": [(0, 60)],
    "open at the read's end": [(EDGE - 70, EDGE)],
    "the whole read": [(0, EDGE)],
    "crosses one tile edge": [(T - 100, T + 100)],
    "begins in tile 0, ends in tile 2": [(T - 1000, 2 * T + 50)],
    "ends exactly at T": [(T - 96, T)],
    "begins exactly at T": [(T, T + 104)],
    "one position apart across a tile edge": [(T - 96, T), (T + 1, T + 104)],
    "min_run and min_run - 1 in front of an edge": [(T - MIN_RUN, T), (2 * T - MIN_RUN + 1, 2 * T)],
    "min_run and min_run - 1 behind an edge": [(T, T + MIN_RUN), (2 * T, 2 * T + MIN_RUN - 1)],
    "min_run and min_run - 1 across an edge": [(T - 25, T + MIN_RUN - 25), (2 * T - 25, 2 * T + MIN_RUN - 26)],
    "across a load of 1024 and a wave of 256": [(1000, 1060), (1024 + 256 - 30, 1024 + 256 + 30), (2048 - 50, 2048)],
    "runs in every tile": [(k * 512 + 10, k * 512 + 300) for k in range(24)],
    "short runs among long ones": [(k * 100, k * 100 + (MIN_RUN if k % 3 else MIN_RUN - 1)) for k in range(120)],
}


def test_runs_at_every_tile_edge(ms):
    """One read per case of EDGE_CASES, so the offsets are checked past the first read, and a partner that every record touches."""
    P = ref.params(max_cov=1, min_run=MIN_RUN, min_unique=10)
    names = list(EDGE_CASES)
    lengths = np.array([EDGE] * len(names) + [50], np.int32)
    ids = np.arange(1, len(lengths) + 1, dtype=np.int64)
    out = []
    for k, name in enumerate(names):
        for s, e in EDGE_CASES[name]:
            out += [tc.rec(int(ids[k]), int(ids[-1]), s, e - 1, EDGE, 0, 0, 50, k & 1)] * 2
    records = tc.recs(out)
    m = _check(ms, ids, lengths, records, P, apply_to=records)
    by = {n: m["intervals"][m["offsets"][k]:m["offsets"][k + 1]].tolist() for k, n in enumerate(names)}
    assert by["begins at 0"] == [[0, 60]] and by["open at the read's end"] == [[EDGE - 70, EDGE]]
    assert by["the whole read"] == [[0, EDGE]] and m["flags"][names.index("the whole read")] == ref.SOME | ref.WHOLE
    assert by["begins in tile 0, ends in tile 2"] == [[T - 1000, 2 * T + 50]]
    assert by["one position apart across a tile edge"] == [[T - 96, T], [T + 1, T + 104]]
    assert by["min_run and min_run - 1 in front of an edge"] == [[T - MIN_RUN, T]]
    assert by["min_run and min_run - 1 behind an edge"] == [[T, T + MIN_RUN]]
    assert by["min_run and min_run - 1 across an edge"] == [[T - 25, T + MIN_RUN - 25]]
    assert len(by["runs in every tile"]) == 24 and len(by["short runs among long ones"]) == 80
    assert (np.diff(m["offsets"]) > 0).sum() == len(names)


def test_more_intervals_in_a_tile_than_the_workgroup_has_lanes(ms):
    """min_run 1 and the depth alternating above and below the threshold at every position of a tile: 2 048 intervals in tile 1 of
    a read, behind an interval carried in from tile 0 and in front of one in tile 2."""
    L = 2 * T + 300
    ids, lengths = np.array([1, 2, 3], np.int64), np.array([L, 64, L], np.int32)
    out = [tc.rec(1, 2, T - 10, T, L, 0, 10, 64)] * 2     # [T - 10, T + 1): carried over the edge, closed at the tile's second position
    out += [x for p in range(T + 2, 2 * T, 2) for x in [tc.rec(1, 2, p, p, L, 1, 1, 64)] * 2]
    out += [tc.rec(1, 2, 2 * T + 100, 2 * T + 199, L, 0, 63, 64)] * 2
    out += [tc.rec(3, 2, 5, 9, L, 0, 4, 64)] * 2            # a read behind it: its offset is past all of them
    records = tc.recs(out)
    m = _check(ms, ids, lengths, records, ref.params(max_cov=1, min_run=1, min_unique=1), apply_to=records[::37])
    assert m["rows"][0].tolist() == [1 + 2047 + 1, 11 + 2047 + 100, 2, T - 10] and m["offsets"].tolist() == [0, 2049, 2050, 2051]


def test_eleven_hundred_reads(ms):
    """The per-read counts are prefix-summed 1 024 at a time: a table of 1 100 reads, two in three of them with intervals."""
    n = 1100
    lengths = np.full(n, 60, np.int32)
    ids = np.arange(1, n + 1, dtype=np.int64)
    out = []
    for r in range(0, n - 1):
        if r % 3:
            out += [tc.rec(int(ids[r]), int(ids[n - 1]), 5, 24, 60, 0, 0, 60)] * 2
        if r % 3 == 2:
            out += [tc.rec(int(ids[r]), int(ids[n - 1]), 40, 54, 60, 1, 1, 60)] * 2
    records = tc.recs(out)
    m = _check(ms, ids, lengths, records, ref.params(max_cov=1, min_run=10, min_unique=5), apply_to=records[::5])
    assert m["counts"]["intervals"] == 366 * 3 and m["offsets"][1025] > 1000


def test_depth_above_the_last_bin(ms):
    """One position with 5 000 intervals falls into the last bin and is still above any threshold; when the typical depth itself sits
    there the finish says to give max_cov, and with max_cov given the threshold is exact above the clamp."""
    ids, lengths = np.array([1, 2], np.int64), np.array([100, 100], np.int32)
    records = tc.recs([tc.rec(1, 2, 0, 99, 100, 0, 99, 100)] + [tc.rec(1, 2, 50, 50, 100, 20, 29, 100)] * 5000)
    m = _check(ms, ids, lengths, records, ref.params(min_run=1))
    assert m["hist"][ref.BINS - 1] == 11 and m["counts"]["depth"] == 1 and m["rows"][0].tolist() == [1, 1, 5001, 50]
    ids, lengths, records = rc.clamp_case(5000)
    with api.RepeatSession(ids, lengths, handle=ms) as rs:
        rs.add(records)
        with pytest.raises(mhap_amd.MhapError) as e:
            rs.finish()
        assert "max_cov" in str(e.value)
        with pytest.raises(mhap_amd.MhapError):
            rs.table()
    _check(ms, ids, lengths, records, ref.params(max_cov=4999, min_run=3))
    _check(ms, ids, lengths, records, ref.params(max_cov=5000, min_run=1))


def test_no_eligible_record(ms):
    ids, lengths = np.array([1, 2], np.int64), np.array([5000, 300], np.int32)
    records = tc.recs([tc.rec(1, 2, 0, 99, 5000, 0, 99, 300, 0, 0.0), tc.rec(1, 1, 0, 99, 5000, 0, 99, 5000), tc.rec(1, 2, 0, 99, 5000, 0, 99, 300, 0, 0.3)])
    m = _check(ms, ids, lengths, records, ref.params(min_identity=0.5), apply_to=records)
    assert m["counts"]["eligible_records"] == 0 and m["counts"]["depth"] == 0 and m["hist"][0] == 5300
    _check(ms, ids, lengths, records[:0], ref.params())
    _check(ms, ids[:0], lengths[:0], records[:0], ref.params())


def test_any_order_and_split_of_the_records(ms):
    P = ref.params(factor_pct=130, min_run=20, min_unique=50)
    rng = np.random.default_rng(11)
    lengths = rng.integers(300, 9000, 40).astype(np.int32)
    ids = np.arange(100, 140, dtype=np.int64)
    records = tc.recs(_random_records(rng, ids, lengths, 6000, span_max=2500))
    whole, half = ref.mark(ids, lengths, records, P), ref.mark(ids, lengths, records[:3000], P)
    assert whole["counts"]["intervals"] > 20

    def tables(rs):
        return [a.tobytes() for a in rs.table()] + [rs.histogram().tobytes(), rs.counts]
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:
        rs.add(records)
        rs.finish()
        _same(rs, whole)
        one = tables(rs)
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:     # permuted
        rs.add(records[rng.permutation(len(records))])
        rs.finish()
        assert tables(rs) == one
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:     # three adds, an empty one among them
        rs.add(records[:1700])
        rs.add(records[:0])
        rs.add(records[1700:])
        rs.finish()
        assert tables(rs) == one
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:     # a finish, more adds, a second finish; and a finish repeated
        rs.add(records[:3000])
        rs.finish()
        _same(rs, half)
        rs.finish()
        _same(rs, half)
        rs.add(records[3000:])
        rs.finish()
        assert tables(rs) == one


def test_crafted_judgements_on_the_device(ms):
    P = ref.params(**rc.JUDGE_P)
    fillers = rc.judge_fillers()
    cases = rc.judge_records()
    judged = tc.recs([c[0] for c in cases])
    with api.RepeatSession(rc.JUDGE_IDS, rc.JUDGE_LEN, handle=ms, **P) as rs:
        rs.add(fillers)
        rs.finish()
        rows, flags, offsets, iv = _same(rs, ref.mark(rc.JUDGE_IDS, rc.JUDGE_LEN, fillers, P))
        for rid, want in rc.JUDGE_IV.items():
            assert [tuple(x) for x in iv[offsets[rid - 1]:offsets[rid]].tolist()] == want
        assert rows[3, 0] == 1000
        keep, unique = rs.apply(judged)
        assert keep.tolist() == [c[1] for c in cases] and unique.tolist() == [[c[2], c[3]] for c in cases]
        ekeep, eunique = ref.apply(rc.JUDGE_IDS, offsets, iv, judged, P)
        assert keep.tobytes() == ekeep.tobytes() and unique.tobytes() == eunique.tobytes()
        assert rs.apply(judged[:0])[0].shape == (0,)


def test_refusals(ms):
    ids, lengths = np.array([1, 2], np.int64), np.array([100, 200], np.int32)
    good = tc.rec(1, 2, 10, 59, 100, 20, 69, 200)
    P = ref.params(max_cov=1, min_run=1)
    for kw in (dict(factor_pct=99), dict(max_cov=-1), dict(min_run=0), dict(min_unique=-1)):
        with pytest.raises(mhap_amd.MhapError):
            api.RepeatSession(ids, lengths, handle=ms, **kw)
    with api.RepeatSession(ids, lengths, handle=ms, **P) as rs:
        with pytest.raises(mhap_amd.MhapError):
            rs.apply(tc.recs([good]))                    # no finish yet
        with pytest.raises(mhap_amd.MhapError):
            rs.table()
        with pytest.raises(mhap_amd.MhapError):
            rs.histogram()
        for bad, word in ((tc.rec(1, 3, 10, 59, 100, 20, 69, 200), "not among the reads"), (tc.rec(1, 2, 10, 59, 101, 20, 69, 200), "the length 101"),
                          (tc.rec(1, 2, 10, 100, 100, 20, 69, 200), "100 bases"), (tc.rec(1, 2, 10, 59, 100, -1, 69, 200), "200 bases"),
                          (tc.rec(1, 2, 60, 59, 100, 20, 69, 200), "100 bases")):
            with pytest.raises(mhap_amd.MhapError) as e:
                rs.add(tc.recs([good, good, bad]))
            assert "record 2" in str(e.value) and word in str(e.value)
        counts = rs.finish()                             # nothing was added by the refused calls
        assert counts["eligible_records"] == 0 and counts["depth"] == 0 and rs.histogram()[0] == 300
        with pytest.raises(mhap_amd.MhapError):
            rs.apply(tc.recs([tc.rec(1, 3, 10, 59, 100, 20, 69, 200)]))
        rs.add(tc.recs([good, good]))
        rs.finish()
        _same(rs, ref.mark(ids, lengths, tc.recs([good, good]), P))


def test_generator_seed_0(ms):
    ids, lengths, records, false, anchor = rc.generate(0)
    P = ref.params()
    m = _check(ms, ids, lengths, records, P, apply_to=records)
    keep, _ = ref.apply(ids, m["offsets"], m["intervals"], records, P)
    assert not keep[false].any() and not ((keep == 0) & ~false & (anchor >= P["min_unique"] + 500)).any()


# ---- end to end: a drawn genome with four copies of a repeat, reads at 5 % error ------------------------------------------------------
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]
GRAPH_P = dict(max_hang=300, min_ovlp=1000, fuzz=300)
G, REPEAT, COPIES = 60000, 3000, (5000, 20000, 35000, 50000)


class E2E:
    """Reads of 4 000 - 6 000 bases at 5 % error, about 25 x over a drawn circular genome of 60 kb with four copies of a 3-kb repeat;
    the driver's plain overlaps of them, realigned, refined and judged through the library with the default parameters."""

    def __init__(self, tmp):
        rng = np.random.default_rng(43)
        codes = rng.integers(0, 4, G).astype(np.uint8)
        for c in COPIES[1:]:
            codes[c:c + REPEAT] = codes[COPIES[0]:COPIES[0] + REPEAT]
        lengths = rng.integers(4000, 6001, 25 * G // 5000).astype(np.int32)
        self.fa = mhap_amd.synth_reads_from_genome(codes, lengths, seed=9, error_rate=0.05)
        self.truth, _ = api.synth_truth(len(lengths), lengths=lengths, genome_len=G, seed=9, error_rate=0.05)
        self.tmp = tmp
        self.fasta = str(tmp / "reads.fasta")
        with open(self.fasta, "w") as fh:
            for i in range(len(self.fa)):
                fh.write(f">read{i}\n{self.fa.sequence(i)}\n")
        run = subprocess.run([CLI, "-s", self.fasta], capture_output=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        self.overlaps = str(tmp / "ovl.txt")
        with open(self.overlaps, "wb") as fh:
            fh.write(run.stdout)
        self.found = read_overlaps(self.overlaps)
        self.res = repeats.repeat_overlaps(self.found, self.fa)
        self.P = ref.params()

    def false_arcs(self, arcs):
        """(false, true) among the final arcs: an arc is false when the genome intervals of its two reads do not intersect."""
        s, n = self.truth["start"], self.truth["span"]
        false = true = 0
        for u, v in arcs[arcs[:, 6] != 0][:, :2].tolist():
            a, b = u >> 1, v >> 1
            d = (int(s[b]) - int(s[a])) % G
            meet = d < int(n[a]) or (G - d) % G < int(n[b])
            false, true = false + (not meet), true + meet
        return false, true


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    return E2E(tmp_path_factory.mktemp("repeat_e2e"))


def test_end_to_end_session_against_restatement_and_fewer_false_arcs(e2e):
    """The session's tables on the GPU's own refined records are the restatement's, every void record has uA or uB below min_unique
    by the restatement, and the graph of the survivors has no more false arcs than the graph of all records.  The four figures are
    printed (EXPERIMENTS.md, "Repeat marking")."""
    res, fa, P = e2e.res, e2e.fa, e2e.P
    m = ref.mark(fa.ids, fa.lengths, res["refined"], P)
    assert res["counts"] == m["counts"] and res["offsets"].tobytes() == m["offsets"].tobytes()
    assert res["intervals"].tobytes() == m["intervals"].tobytes() and res["rows"].tobytes() == m["rows"].tobytes()
    assert res["flags"].tobytes() == m["flags"].tobytes() and res["hist"].tobytes() == m["hist"].tobytes()
    ekeep, eunique = ref.apply(fa.ids, m["offsets"], m["intervals"], res["refined"], P)
    assert res["keep"].tobytes() == ekeep.tobytes() and res["unique"].tobytes() == eunique.tobytes()
    void = res["keep"] == 0
    assert (eunique[void].min(axis=1) < P["min_unique"]).all() and (eunique[~void].min(axis=1) >= P["min_unique"]).all()
    assert len(res["refined"]) == len(res["realigned"]) > 1000 and m["counts"]["eligible_records"] == len(res["refined"])
    plain = graph.graph_overlaps(e2e.found, fa, **GRAPH_P)
    filtered = graph.graph_overlaps(e2e.found, fa, repeat={}, **GRAPH_P)     # the defaults
    assert filtered[-1] == m["counts"]
    f0, t0 = e2e.false_arcs(plain[1])
    f1, t1 = e2e.false_arcs(filtered[1])
    print(f"{api.repeat_counts_line([m['counts'][k] for k in api.REPEAT_COUNTS])}; {int(void.sum())} of {len(void)} overlaps void; "
          f"final arcs without the filter: {f0} false, {t0} true; with: {f1} false, {t1} true")
    assert f1 <= f0


GRAPH_FLAGS = ["--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300"]


def _tool(tool, argv, capsys):
    """A tool's main in this process (no interpreter to start): its stderr lines."""
    capsys.readouterr()
    assert tool.main(argv) == 0
    return capsys.readouterr().err.split("\n")


def test_end_to_end_driver_and_tools(e2e, capsys):
    """mhap-hip --realign --gfa with and without --repeat-filter: the same stdout, the session's table, and the GFA of
    `python -m mhap_amd.graph` with the same flags (which, without the flag, is the path this stage has not touched)."""
    tmp, fasta, fa, res = e2e.tmp, e2e.fasta, e2e.fa, e2e.res
    g0, g1, tt = (str(tmp / n) for n in ("plain.gfa", "repeat.gfa", "repeat.tsv"))
    r0 = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", g0] + SCALED, capture_output=True, timeout=600)
    r1 = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", g1] + SCALED + ["--repeat-filter", "--repeat-table", tt], capture_output=True, timeout=600)
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    assert b"Repeats" not in r0.stderr and b"--repeat" not in r0.stderr
    assert sorted(r1.stdout.split(b"\n")) == sorted(r0.stdout.split(b"\n"))
    line = [l for l in r1.stderr.decode().split("\n") if l.startswith("Repeats: ")]
    assert line == [api.repeat_counts_line([res["counts"][k] for k in api.REPEAT_COUNTS])]
    assert open(tt).read() == repeats.format_table(fa.ids, res["offsets"], res["intervals"]) and res["counts"]["intervals"] > 0
    for flags, want in (([], g0), (["--repeat-filter"], g1)):
        pg = str(tmp / "tool.gfa")
        err = _tool(graph, [e2e.overlaps, fasta, "-o", pg] + GRAPH_FLAGS + flags, capsys)
        assert open(pg).read() == open(want).read()
        assert [l for l in err if l.startswith("Repeats: ")] == (line if flags else [])
    assert open(g0).read() != open(g1).read()
    # the tool of the stage itself: the same table, and the kept overlaps as realigned
    pt, po = str(tmp / "tool.tsv"), str(tmp / "kept.txt")
    err = _tool(repeats, [e2e.overlaps, fasta, "--table", pt, "-o", po], capsys)
    assert open(pt).read() == open(tt).read() and [l for l in err if l.startswith("Repeats: ")] == line
    assert open(po).read().split("\n") == api.records_to_lines(res["realigned"][res["keep"] != 0]) + [""]


def test_end_to_end_with_trimming_behind_it(e2e, capsys):
    """With --trim too the trimming piles up the survivors only: the driver and the tool write the same graph and the same two lines."""
    tmp, fasta = e2e.tmp, e2e.fasta
    t1, t2 = str(tmp / "both.gfa"), str(tmp / "both_tool.gfa")
    both = ["--repeat-filter", "--trim", "--trim-end-clip", "100", "--trim-min-span", "500"]
    r = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", t1] + SCALED + both, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    err = _tool(graph, [e2e.overlaps, fasta, "-o", t2] + GRAPH_FLAGS + both, capsys)
    assert open(t1).read() == open(t2).read()
    e = r.stderr.decode().split("\n")
    assert [l for l in e if l.startswith("Repeats: ")] == [api.repeat_counts_line([e2e.res["counts"][k] for k in api.REPEAT_COUNTS])]
    assert [l for l in e if l.startswith(("Repeats: ", "Trim: "))] == [l for l in err if l.startswith(("Repeats: ", "Trim: "))] and len(err) > 2
    plain = subprocess.run([CLI, "-s", fasta, "--realign", "--gfa", str(tmp / "trim_only.gfa")] + SCALED + both[1:], capture_output=True, timeout=600)
    assert plain.returncode == 0 and [l for l in plain.stderr.decode().split("\n") if l.startswith("Trim: ")] != [l for l in e if l.startswith("Trim: ")]
