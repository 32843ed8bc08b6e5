"""The unitig consensus on the GPU (mhap_consensus_*, consensus_kernels.hip) against its CPU restatement
(tests/unitig_consensus_ref.py), byte for byte: the placement table, the vote counters, the consensus bytes, the six counts per
unitig, the position map and the counts.  The reads are cut from drawn genomes and the records hand-made from the truth positions;
the unitig tables and the spelled drafts the restatement is given are the graph session's own, which tests/test_unitigs_gpu.py pins."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import align_paths_ref as apr  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import unitig_consensus_ref as ucr  # noqa: E402
import unitig_ref as ur  # noqa: E402
from align_ref import rc_bytes  # noqa: E402
from mhap_amd import api  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096
PARAMS = dict(max_hang=100, int_frac_permille=800, min_ovlp=200, fuzz=100)
BAND = 24


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def test_the_tile_is_the_headers():
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        assert f"#define MHAP_CONSENSUS_TILE {TILE}\n" in fh.read()
    assert api.CONSENSUS_TILE == TILE == ucr.TILE


class Case:
    """Reads (stored bytes) with ids, and records."""

    def __init__(self, first_id=1):
        self.ids, self.reads, self.recs, self.next_id = [], [], [], first_id

    def read(self, seq):
        self.ids.append(self.next_id)
        self.reads.append(bytes(seq))
        self.next_id += 1
        return self.ids[-1]

    def cut(self, genome, s, e, strand):
        """The read genome[s:e] on `strand`; returns (id, (s, e, strand)) for placed()."""
        return self.read(rc_bytes(genome[s:e]) if strand else genome[s:e]), (s, e, strand)

    def rec(self, r):
        if r is not None:
            self.recs.append(r)

    def placed(self, x, y, trim=(0, 0, 0, 0), score=0.9):
        self.rec(sg.placed(x[0], y[0], x[1], y[1], trim, score))

    def chain(self, genome, spans, strands):
        """Members cut at `spans`, a record per consecutive pair, which is `from` alternating."""
        ms_ = [self.cut(genome, s, e, f) for (s, e), f in zip(spans, strands)]
        for i in range(len(ms_) - 1):
            self.placed(*((ms_[i], ms_[i + 1]) if i % 2 == 0 else (ms_[i + 1], ms_[i])))
        return ms_

    @property
    def lengths(self):
        return [len(r) for r in self.reads]

    def records(self):
        return np.concatenate(self.recs) if self.recs else np.zeros(0, sg.RECORD_DTYPE)

    def fasta(self):
        offsets = np.concatenate([[0], np.cumsum(self.lengths)])[:len(self.reads)].astype(np.int64)
        return mhap_amd.FastaData(np.frombuffer(b"".join(self.reads), np.uint8), offsets, np.array(self.lengths, np.int32), np.array(self.ids, np.int64))


def check(ms, case, recs=None, adds=None, clean=False, band=BAND, min_cov=4):
    """Run the library and the restatement on one case and compare everything; returns (the restatement's result, the unitig tables,
    what the library returned)."""
    recs = case.records() if recs is None else recs
    fasta = case.fasta()
    with api.GraphSession(case.ids, case.lengths, handle=ms, **PARAMS) as gs:
        gs.add(recs)
        gs.finish()
        if clean:
            gs.clean()
        else:
            gs.unitigs()
        tables = gs.unitigs_table
        drafts = gs.unitig_sequences(fasta)
        with api.ConsensusSession(gs, fasta, band=band, min_cov=min_cov) as cs:
            for part in (adds if adds is not None else [recs]):
                cs.add(part)
            counts = cs.run()
            got = dict(placements=cs.placements(), seqs=cs.sequences(), stats=cs.stats.copy(), maps=cs.position_maps(),
                       votes=[cs.votes(k) for k in range(len(drafts))], gfa=cs.gfa(), drafts=drafts)
    ref = ucr.consensus(case.ids, case.lengths, case.reads, recs, tables, drafts, sg.Params(**PARAMS), band=band, max_shift=0.2, min_cov=min_cov)
    bad = np.flatnonzero((got["placements"] != ref.placements).any(axis=1))
    assert len(bad) == 0, (bad[:5], got["placements"][bad[:5]], ref.placements[bad[:5]])
    for k in range(len(drafts)):
        v = got["votes"][k].astype(np.int64)
        rows = np.flatnonzero((v != ref.votes[k]).any(axis=1))
        assert len(rows) == 0, (k, rows[:5], v[rows[:3]], ref.votes[k][rows[:3]])
        assert got["seqs"][k] == ref.seqs[k], k
        assert np.array_equal(got["maps"][k], ref.maps[k]), k
    assert got["stats"].tolist() == ref.stats.tolist()
    assert counts == ref.counts
    assert got["gfa"] == ucr.gfa(case.ids, tables, ref.seqs, ref.maps)
    return ref, tables, got


def steps(n, step, length, total=None):
    """n spans [i * step, i * step + length), the last one ending at `total` when given."""
    out = [(i * step, i * step + length) for i in range(n)]
    if total is not None:
        out[-1] = (out[-1][0], total)
    return out


# ---- 1. placement ---------------------------------------------------------------------------------------------------------------------

def placement_case():
    g = ur.draw_bases(2600, 11)
    c = Case(first_id=101)
    m = c.chain(g, [(200 + 300 * i, 800 + 300 * i) for i in range(6)], [0, 1, 0, 0, 1, 1])
    named = {}
    # X as `from` and as `to`, to_rc 0 / 1, through a member on an even and on an odd vertex (m[0] and m[1] have different strands)
    for mi, base in ((0, 220), (1, 560)):
        for k, (sx, x_from) in enumerate(((0, True), (0, False), (1, True), (1, False))):
            x = c.cut(g, base + 20 * k, base + 20 * k + 400, sx)
            c.placed(*((x, m[mi]) if x_from else (m[mi], x)))
            named[("combo", mi, sx, x_from)] = x[0]
    # W, contained in m[0]; X_neg begins before the unitig: contained by a record with W (two non-members: it places nobody), placed by
    # its dovetail-shaped record with m[0] at a negative p
    w = c.cut(g, 250, 750, 0)
    c.placed(w, m[0])
    x_neg = c.cut(g, 50, 500, 0)
    c.rec(sg.record(x_neg[0], w[0], 0, 449, 450, 10, 459, 500, 0))
    c.placed(x_neg, m[0])
    named["neg"] = x_neg[0]
    # the same beyond the end, through the last member, on the other strand
    w2 = c.cut(g, 1750, 2250, 1)
    c.placed(m[5], w2)
    x_end = c.cut(g, 2000, 2450, 1)
    c.rec(sg.record(x_end[0], w2[0], 0, 449, 450, 20, 469, 500, 0))
    c.placed(m[5], x_end)
    named["end"] = x_end[0]
    # a tie on xe - xs broken by the vertex: whole on m[1] and on m[2], the record with m[2] shifted by 7
    x_tie = c.cut(g, 820, 1080, 0)
    c.placed(x_tie, m[1])
    r = sg.placed(x_tie[0], m[2][0], x_tie[1], m[2][1])
    r["b1"] += 7
    r["b2"] += 7
    c.rec(r)
    named["tie_vertex"] = x_tie[0]
    # a full key tie broken by (p, sX): the same member, the same extent, p and p + 4; and (p, 1) against (p + 4, 0)
    x_p = c.cut(g, 1450, 1850, 0)
    for shift in (4, 0):
        r = sg.placed(x_p[0], m[4][0], x_p[1], m[4][1])
        r["b1"] += shift
        r["b2"] += shift
        c.rec(r)
    named["tie_p"] = x_p[0]
    x_s = c.cut(g, 1160, 1560, 0)
    r0, r1 = sg.placed(x_s[0], m[3][0], x_s[1], m[3][1]), sg.placed(x_s[0], m[3][0], x_s[1], m[3][1])
    r0["b1"] += 4
    r0["b2"] += 4
    r1["to_rc"] ^= 1
    c.rec(r0)
    c.rec(r1)
    named["tie_strand"] = x_s[0]
    # a record given twice
    c.rec(c.recs[len(m) - 1 + 2].copy())
    # U: contained by a record with the non-member W; its records with a member are of class NONE and INTERNAL: unplaced
    u = c.cut(g, 300, 700, 0)
    c.rec(sg.record(u[0], w[0], 0, 399, 400, 50, 449, 500, 0))
    c.rec(sg.record(u[0], m[0][0], 0, 399, 400, 100, 499, 600, 0, score=0.0))
    c.rec(sg.record(u[0], m[0][0], 150, 299, 400, 250, 399, 600, 0))
    c.rec(sg.record(u[0], u[0], 0, 399, 400, 0, 399, 400, 0))
    named["unplaced"] = u[0]
    return c, named


def test_placement_every_case(ms):
    c, named = placement_case()
    ref, tables, got = check(ms, c)
    row = {i: ref.placements[k].tolist() for k, i in enumerate(c.ids)}
    vertex_of = {int(v) >> 1: int(v) for v in tables["vertex"]}
    assert len(tables["unitig_len"]) == 1 and len(tables["vertex"]) == 6 and int(tables["vertex"][0]) == 0
    assert {vertex_of[0] & 1, vertex_of[1] & 1} == {0, 1}                  # the eight combinations see an even and an odd member vertex
    for key, i in named.items():
        if key[0] == "combo":
            assert row[i][3] == ucr.RECORD and row[i][4] == 1, key
    ps = sorted((row[named["neg"]][2], row[named["end"]][2]))
    assert ps[0] < 0 and ps[1] + 450 > int(tables["unitig_len"][0])           # one before the start, one beyond the end
    assert row[named["neg"]][4] == 1 and row[named["end"]][4] == 1
    assert row[named["unplaced"]] == [-1, 0, 0, ucr.UNPLACED, 0]
    assert ref.counts["unplaced"] == 1 and ref.counts["members"] == 6
    # the tie on the extent went to the smaller vertex, whatever that was
    k_tie = c.ids.index(named["tie_vertex"])
    lo = min(vertex_of[1], vertex_of[2])
    recs = c.records()
    only = recs[~((recs["from_id"] == named["tie_vertex"]) & (recs["to_id"] == c.ids[(lo ^ vertex_of[1] ^ vertex_of[2]) >> 1]))]
    assert ucr.place(c.ids, c.lengths, only, tables, sg.Params(**PARAMS))[k_tie].tolist()[:4] == row[named["tie_vertex"]][:4]
    # (p, sX): the smaller p of p and p + 4; and strand 1 at p before strand 0 at p + 4
    mine = lambda name: recs[recs["from_id"] == named[name]]
    alone = lambda name: [ucr.place(c.ids, c.lengths, mine(name)[k:k + 1], tables, sg.Params(**PARAMS))[c.ids.index(named[name])].tolist() for k in (0, 1)]
    for name in ("tie_p", "tie_strand"):
        a, b = alone(name)
        assert abs(a[2] - b[2]) == 4 and row[named[name]][:3] == min(a, b, key=lambda r: (r[2], r[1]))[:3], name
    a, b = alone("tie_strand")
    assert {a[1], b[1]} == {0, 1} and row[named["tie_strand"]][1] == 1                 # strand 1 at p comes before strand 0 at p + 4
    # the same records in three adds and shuffled
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(recs))
    ref2, _, got2 = check(ms, c, recs=recs[perm], adds=[recs[perm][:5], recs[perm][5:5], recs[perm][5:20], recs[perm][20:]])
    assert np.array_equal(got2["placements"], got["placements"]) and got2["seqs"] == got["seqs"]
    assert all(np.array_equal(a, b) for a, b in zip(got2["votes"], got["votes"]))


# ---- 2. call tiles ----------------------------------------------------------------------------------------------------------------------

def planted(L, kind, sites, seed):
    """(draft genome D of L bases, truth T, where): the members are cut from D, the evidence from T.  kind: "sub", "del" (D has an extra
    base at the site) or ("ins", n) (D lacks the n bases after the site).  where[site] = the site's position in T."""
    rng = np.random.default_rng(seed)
    D = ur.draw_bases(L, seed)
    T, where = bytearray(), {}
    for t in range(L):
        if t in sites:
            where[t] = len(T)
        if t in sites and kind == "del":
            continue
        if t in sites and kind == "sub":
            T.append(next(x for x in b"ACGT" if x != D[t]))
        else:
            T.append(D[t])
        if t in sites and isinstance(kind, tuple):
            T += bytes(int(x) for x in rng.choice(list(b"ACGT"), kind[1]))
    return D, bytes(T), where


def tile_unitig(c, L, kind, sites, seed, step=500, length=1000, evidence=4, elen=400):
    """A chain unitig of draft length L with planted sites and `evidence` contained reads from the truth over each site."""
    D, T, where = planted(L, kind, set(sites), seed)
    n = (L - length + step - 1) // step + 1                               # the last read is longer than a step: it ends outside its predecessor
    spans = steps(n, step, length, total=L)
    m = c.chain(D, spans, [i % 2 for i in range(len(spans))])
    for gi, site in enumerate(sites):
        for e in range(evidence):
            ln = elen + 20 * e
            at = where[site]
            ts = min(max(0, at - ln // 2 + 15 * e), len(T) - ln)
            ds = min(max(0, ts + (site - at)), L - ln)                     # the same stretch in the draft's coordinates, nearly
            inside = [mm for mm, (s, e_) in zip(m, spans) if s <= ds and ds + ln <= e_]
            if not inside:
                continue
            x = (c.read(rc_bytes(T[ts:ts + ln]) if e % 2 else T[ts:ts + ln]), (ds, ds + ln, e % 2))
            c.placed(x, inside[0])
    return m


@pytest.mark.parametrize("kind", ["sub", "del", ("ins", 1), ("ins", 4), ("ins", 5)], ids=lambda k: k if isinstance(k, str) else f"ins{k[1]}")
def test_call_tiles_two_tiles_and_a_position(ms, kind):
    L = 2 * TILE + 1
    c = Case()
    tile_unitig(c, L, kind, [0, TILE - 1, TILE, L - 1], seed=40 + (kind[1] if isinstance(kind, tuple) else len(kind)))
    ref, tables, got = check(ms, c)
    assert tables["unitig_len"].tolist() == [L]
    st = ref.stats[0].tolist()
    col = {"sub": 2, "del": 3}.get(kind, 4)
    assert st[col] >= 2, st                                                 # the two interior sites at least are called
    assert got["seqs"][0] != got["drafts"][0]


def members_of(c, tables):
    """read id -> unitig, for the members."""
    start = tables["unitig_start"].tolist()
    return {c.ids[int(v) >> 1]: k for k in range(len(start) - 1) for v in tables["vertex"][start[k]:start[k + 1]]}


@pytest.mark.parametrize("L,kind,seed", [(TILE - 1, "sub", 51), (TILE, "del", 52), (TILE + 1, ("ins", 4), 53)], ids=["4095", "4096", "4097"])
def test_call_lengths_round_the_tile(ms, L, kind, seed):
    c = Case(first_id=7)
    lone = c.read(b"A")                                                      # a unitig of one base: a read no arc touches
    m = tile_unitig(c, L, kind, [0, L // 2, TILE - 1, L - 1] if L > TILE else [0, L // 2, L - 1], seed)
    ref, tables, got = check(ms, c)
    assert sorted(tables["unitig_len"].tolist()) == [1, L]
    of = members_of(c, tables)
    assert ref.seqs[of[lone]] == b"A" and ref.stats[of[lone]].tolist() == [1, 1, 0, 0, 0, 1]
    col = {"sub": 2, "del": 3}.get(kind, 4)
    assert ref.stats[of[m[0][0]]][col] >= 1                                   # the site in the middle at least is called


def test_no_evidence_and_neighbouring_depths(ms):
    c = Case()
    # a unitig without evidence, and one where the depth is min_cov up to a position and min_cov - 1 from the next on
    g = ur.draw_bases(1500, 54)
    plain = c.chain(g, steps(2, 500, 1000), [0, 1])
    g2 = ur.draw_bases(1500, 55)
    deep = c.chain(g2, steps(2, 500, 1000), [1, 0])
    for end in (430, 431, 431):
        c.placed(c.cut(g2, 30, end, 0), deep[0])
    ref, tables, got = check(ms, c)
    of = members_of(c, tables)
    kp, kd = of[plain[0][0]], of[deep[0][0]]
    assert ref.stats[kp].tolist() == [1500, 1500, 0, 0, 0, 1500] and got["seqs"][kp] == got["drafts"][kp]
    depth = (ref.votes[kd][:, :4].sum(axis=1) + ref.votes[kd][:, 4]).tolist()
    assert [(a, b) for a, b in zip(depth, depth[1:]) if {a, b} == {3, 4}], "min_cov and min_cov - 1 at neighbouring positions"
    assert ref.stats[kd].tolist()[1:] == [1500, 0, 0, 0, 1500 - depth.count(4)] and depth.count(4) == 400


# ---- 3. a long path, the reverse strand ------------------------------------------------------------------------------------------------

def test_a_path_of_more_than_64_runs_on_the_reverse_strand(ms):
    g = ur.draw_bases(1500, 61)
    c = Case()
    m = c.chain(g, steps(2, 500, 1000), [0, 0])
    noisy = bytearray(g[100:900])
    for t in range(5, 800, 6):                                               # a substitution every six bases: '=' and 'X' alternate
        noisy[t] = next(x for x in b"ACGT" if x != noisy[t])
    x = (c.read(rc_bytes(bytes(noisy))), (100, 900, 1))
    c.placed(x, m[0])
    for s in (120, 140, 160):
        c.placed(c.cut(g, s, s + 700, s // 20 % 2), m[0])
    ref, tables, got = check(ms, c)
    row = ref.placements[c.ids.index(x[0])].tolist()
    k, strand, p, how, aligned = row
    assert how == ucr.RECORD and aligned == 1
    d = got["drafts"][0]
    bd, w0, w1 = ucr.window(p, 800, len(d), BAND, 0.2)
    s2 = rc_bytes(c.reads[c.ids.index(x[0])]) if strand else c.reads[c.ids.index(x[0])]
    _, runs = apr.align_path(d[w0:w1], s2, w0 - p, bd)
    assert len(runs) > 64
    strands = {int(r[1]) for r in ref.placements if r[3] != ucr.UNPLACED}
    assert strands == {0, 1}


# ---- 4. a circular unitig ---------------------------------------------------------------------------------------------------------------

def test_circular_unitig_and_reads_over_the_cut(ms):
    C, n, step, ln = 2400, 6, 400, 800
    g = ur.draw_bases(C, 71)
    gg = g + g
    c = Case()
    m = [c.read(gg[i * step:i * step + ln]) for i in range(n)]
    for i in range(n):
        c.rec(sg.dove(m[i], m[(i + 1) % n], step, read_len=ln))
    # contained in the last member, running over the cut: placed at 2 200, its last 300 bases hang over the end
    x1 = c.read(gg[2200:2700])
    c.rec(sg.record(x1, m[5], 0, 499, 500, 200, 699, ln, 0))
    # contained by its record with the last member, and tied on the extent with its record with the first, which wins on the vertex and
    # gives p = -100: reduced modulo the length
    x2 = c.read(gg[2300:2800])
    c.rec(sg.record(x2, m[5], 50, 449, 500, 350, 749, ln, 0))
    c.rec(sg.record(x2, m[0], 100, 499, 500, 0, 399, ln, 0))
    for s in (2250, 2290, 2330):                                            # more of them, from both sides of the cut
        x = c.read(gg[s:s + 450])
        c.rec(sg.record(x, m[5], 0, 449, 450, s - 2000, s - 2000 + 449, ln, 0))
    ref, tables, got = check(ms, c)
    assert tables["circular"].tolist() == [1] and tables["unitig_len"].tolist() == [C] and int(tables["vertex"][0]) == 0
    assert ref.placements[c.ids.index(x1)].tolist()[:4] == [0, 0, 2200, ucr.RECORD]
    assert ref.placements[c.ids.index(x2)].tolist()[:4] == [0, 0, 2300, ucr.RECORD]
    assert ref.seqs[0] == g                                                    # error-free reads change nothing


# ---- 5. several unitigs, links, cleaning ------------------------------------------------------------------------------------------------

def tip_case():
    g = ur.draw_bases(2500, 81)
    c = Case()
    m = c.chain(g, [(300 * i, 300 * i + 600) for i in range(6)], [0, 0, 1, 0, 1, 0])
    # a tip: 350 bases of the line from 950 on, then 250 bases of its own; a dovetail with m[2], an internal match with m[3]
    tip_seq = g[950:1300] + ur.draw_bases(250, 82)
    tip = (c.read(tip_seq), (950, 1550, 0))
    c.rec(sg.placed(m[2][0], tip[0], m[2][1], tip[1], (0, 0, 0, 0)))
    c.rec(sg.record(tip[0], m[3][0], 0, 349, 600, 50, 399, 600, int(m[3][1][2] != 0)))
    for s in (620, 660, 700, 960, 1000):
        c.placed(c.cut(g, s, s + 450, s // 20 % 2), m[2] if s < 900 else m[3])
    return c, tip


def test_several_unitigs_links_and_cleaning(ms):
    c, tip = tip_case()
    ref, tables, _ = check(ms, c)
    assert len(tables["unitig_len"]) == 3 and len(tables["links"]) == 4
    assert ref.placements[c.ids.index(tip[0])][3] == ucr.MEMBER
    ref2, tables2, _ = check(ms, c, clean=True)
    assert len(tables2["unitig_len"]) == 1 and len(tables2["vertex"]) == 6
    row = ref2.placements[c.ids.index(tip[0])].tolist()
    assert row[3] == ucr.RECORD and row[4] == 1                               # the dropped read votes as a non-member
    assert ref2.counts["placed_by_record"] == ref.counts["placed_by_record"] + 1


# ---- 6. the guard -----------------------------------------------------------------------------------------------------------------------

def test_guard(ms, monkeypatch):
    g = ur.draw_bases(700, 91)
    c = Case()
    m = c.cut(g, 0, 700, 0)
    xs = [c.cut(g, 50 + 10 * k, 500 + 10 * k, 0) for k in range(3)]
    for x in xs:
        c.placed(x, m)
    fasta = c.fasta()
    with api.GraphSession(c.ids, c.lengths, handle=ms, **PARAMS) as gs:
        gs.add(c.records())
        gs.finish()
        gs.unitigs()
        monkeypatch.setenv("MHAP_CONSENSUS_TILE_CAP", "3")
        with api.ConsensusSession(gs, fasta, band=BAND) as cs:
            cs.add(c.records())
            with pytest.raises(api.MhapError, match="unitig 0 tile 0 is met by 4 reads, more than 3"):
                cs.run()
            with pytest.raises(api.MhapError, match="no mhap_consensus_run has completed"):
                cs.placements()
            monkeypatch.delenv("MHAP_CONSENSUS_TILE_CAP")
            assert cs.run()["aligned"] == 4                                  # after a refusal the session still runs
        monkeypatch.setenv("MHAP_CONSENSUS_TILE_CAP", "3")
        with api.ConsensusSession(gs, fasta, band=BAND) as cs:
            cs.add(c.records()[:2])                                          # three reads on the tile pass
            assert cs.run()["aligned"] == 3
    with pytest.raises(ucr.Refused, match="unitig 0 tile 0 is met by 4 reads, more than 3"):
        ucr.consensus(c.ids, c.lengths, c.reads, c.records(), ur.of_graph(ur.graph_of(c.ids, c.lengths, c.records(), **PARAMS)).tables(),
                      [g], sg.Params(**PARAMS), band=BAND, tile_cap=3)


# ---- 7. call order ----------------------------------------------------------------------------------------------------------------------

def test_call_order(ms):
    g = ur.draw_bases(1500, 95)
    c = Case()
    c.chain(g, steps(2, 500, 1000), [0, 1])
    fasta, recs = c.fasta(), c.records()
    with api.GraphSession(c.ids, c.lengths, handle=ms, **PARAMS) as gs:
        gs.add(recs)
        gs.finish()
        with api.ConsensusSession(gs, fasta) as cs:                          # before the unitigs exist
            with pytest.raises(api.MhapError, match="serves no unitigs"):
                cs.run()
        gs.unitigs()
        with api.ConsensusSession(gs, fasta) as cs:
            cs.add(recs)
            with pytest.raises(api.MhapError, match="no mhap_consensus_run has completed"):   # copy before run
                cs.sequences()
            with pytest.raises(api.MhapError, match="no mhap_consensus_run has completed"):
                cs._ms._chk(cs._lib.mhap_consensus_votes(cs._s, 0, None))
            bad = recs[:1].copy()
            bad["alen"] += 1
            with pytest.raises(api.MhapError, match="record 0 gives read"):
                cs.add(bad)
            assert cs.run()["members"] == 2 and cs.info()[0] == 1
            cs.add(recs[:0])
            assert cs.run()["members"] == 2                                   # run may be repeated
            gs.finish()                                                        # a later finish invalidates the session
            for call in (cs.run, cs.sequences, cs.placements, lambda: cs.add(recs)):
                with pytest.raises(api.MhapError, match="since mhap_consensus_begin"):
                    call()
            assert cs.info()[0] == -1
        gs.unitigs()
        with api.ConsensusSession(gs, fasta) as cs:
            cs.run()
            gs.unitigs()                                                       # and so does building the unitigs again
            with pytest.raises(api.MhapError, match="since mhap_consensus_begin"):
                cs.sequences()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------

import subprocess  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]


def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


def _errors_against(genome, seqs):
    """(errors, columns) of `seqs` against the doubled genome and its reverse complement, the better strand each, with the project's
    own aligner; the bases of a sequence left outside its alignment count as errors."""
    g2 = genome + genome
    bases = np.frombuffer(g2 + b"".join(seqs), np.uint8)
    pairs, at = [], len(g2)
    for s in seqs:
        pairs += [(at, len(s), 0, len(g2), 0), (at, len(s), 0, len(g2), 1)]
        at += len(s)
    res = mhap_amd.align_pairs(bases, np.array(pairs, np.int64))
    errors = columns = 0
    for k, s in enumerate(seqs):
        best = max(res[2 * k].tolist(), res[2 * k + 1].tolist(), key=lambda r: r[0])
        errors += best[6] + len(s) - (best[2] - best[1] + 1)
        columns += best[5]
    return errors, columns


def _unitig_seqs(text, min_members=2):
    return [l.split("\t")[2].encode() for l in text.split("\n") if l.startswith("S\t") and int(l.split("\t")[4][5:]) >= min_members]


def test_end_to_end_consensus_has_fewer_errors_than_the_draft(tmp_path):
    """Reads of 2 500 - 3 500 bases at 10 % error, about 25 x over a drawn circular genome of 20 kb, through the driver and the tool.
    Measured on an MI355X, over the 4 unitigs of two reads or more: draft 3 137 errors in 32 896 columns, consensus 778 in 31 058
    (EXPERIMENTS.md)."""
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    genome = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 170).astype(np.int32), seed=9, error_rate=0.10)
    fasta = str(tmp_path / "reads.fasta")
    with open(fasta, "w") as fh:
        for i in range(len(fa)):
            fh.write(f">read{i}\n{fa.sequence(i)}\n")
    g0, u0, g1, u1, f1 = (tmp_path / n for n in ("draft.gfa", "draft.utg.gfa", "cons.gfa", "cons.utg.gfa", "cons.fasta"))
    plain = _cli(["-s", fasta])
    r0 = _cli(["-s", fasta, "--realign", "--gfa", str(g0), "--gfa-unitigs", str(u0)] + SCALED)
    r1 = _cli(["-s", fasta, "--realign", "--gfa", str(g1), "--gfa-unitigs", str(u1), "--gfa-consensus", "--gfa-consensus-fasta", str(f1)] + SCALED)
    assert plain.returncode == 0 and r0.returncode == 0 and r1.returncode == 0, r1.stderr[-2000:]
    # without the flag nothing of the consensus shows; with it the overlaps and the read graph are what they were
    assert b"Consensus" not in r0.stderr and b"--gfa-consensus" not in r0.stderr
    assert sorted(r1.stdout.split(b"\n")) == sorted(r0.stdout.split(b"\n")) and g1.read_bytes() == g0.read_bytes()
    line = [l for l in r1.stderr.decode().split("\n") if l.startswith("Consensus: ")]
    assert len(line) == 1
    draft_text, cons_text = u0.read_text(), u1.read_text()
    other = lambda t: [l for l in t.split("\n") if not l.startswith(("S\t", "a\t"))]
    assert other(draft_text) == other(cons_text)
    names = lambda t: [l.split("\t")[1] for l in t.split("\n") if l.startswith("S\t")]
    assert names(draft_text) == names(cons_text)
    for l in cons_text.split("\n"):
        if l.startswith("S\t"):
            assert l.split("\t")[3] == f"LN:i:{len(l.split(chr(9))[2])}"
    assert f1.read_text() == "".join(f">{l.split(chr(9))[1]}\n{l.split(chr(9))[2]}\n" for l in cons_text.split("\n") if l.startswith("S\t"))
    # the tool writes the same files
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tg, tu, tf = tmp_path / "tool.gfa", tmp_path / "tool.utg.gfa", tmp_path / "tool.fasta"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.graph", str(tmp_path / "ovl.txt"), fasta, "--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300",
                        "-o", str(tg), "--unitigs", str(tu), "--consensus", "--consensus-fasta", str(tf)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tg.read_bytes() == g1.read_bytes() and tu.read_bytes() == u1.read_bytes() and tf.read_bytes() == f1.read_bytes()
    assert [l for l in p.stderr.split("\n") if l.startswith("Consensus: ")] == line
    # fewer errors against the genome than the draft has, over the unitigs of at least two reads
    drafts, cons = _unitig_seqs(draft_text), _unitig_seqs(cons_text)
    assert len(drafts) == len(cons) > 0
    de, dc = _errors_against(genome, drafts)
    ce, cc = _errors_against(genome, cons)
    print(f"{line[0]} | {len(drafts)} unitigs of two reads or more: draft {de} errors / {dc} columns, consensus {ce} errors / {cc} columns")
    assert ce < de
