"""Variant sites on the GPU (variant_kernels.hip) against tests/variant_ref.py, byte for byte: the six counters of every position, the
rows, offsets, site list (and through it the site bytes), the counts, and every record's tallies and keep.  The cases put sites on
both sides of the site kernel's tile edges, informative columns on the first and last column of the walk's chunks of 64 runs and
deals of 64 columns, and take the add apart; then the cap, the refusals, and the error-free planted diploid as the truth gate.  Every
test names its six parameters."""
import numpy as np
import pytest

import mhap_amd
from mhap_amd import api
from mhap_amd.realign import kept_rows

import consensus_ref as cr
import handmade_paths as hp
import variant_cases as vc
import variant_ref as vr
from align_ref import rc_bytes

pytestmark = pytest.mark.gpu
TILE = api.VARIANT_TILE


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def fasta_of(reads, ids):
    lengths = np.array([len(r) for r in reads], np.int32)
    offsets = (np.cumsum(lengths, dtype=np.int64) - lengths).astype(np.int64)
    return mhap_amd.FastaData(np.frombuffer(b"".join(reads), np.uint8), offsets, lengths, np.array(ids, np.int64))


def same_as_restatement(ms, reads, ids, adds, p, judged=None):
    """One session and one restatement over the same adds; everything either makes is compared.  Returns (session outputs, restatement)."""
    ref = vr.Variants(reads, ids, **p)
    with api.VariantSession(fasta_of(reads, ids), handle=ms, **p) as vs:
        for recs, off, ops in adds:
            vs.add(recs, off, ops)
            ref.add(recs, off, ops)
        for r in range(len(reads)):
            assert vs.votes(r).astype(np.int64).tolist() == ref.votes(r).tolist(), r
        counts = vs.finish()
        assert [counts[k] for k in api.VARIANT_COUNTS] == ref.finish()
        rows, offsets, sites = vs.table()
        assert rows.tolist() == ref.rows.tolist() and offsets.tolist() == ref.offsets.tolist() and sites.tolist() == ref.sites.tolist()
        out = []
        for recs, off, ops in (judged or adds):
            keep, tallies = vs.apply(recs, off, ops)
            want_keep, want = ref.apply(recs, off, ops)
            assert tallies.tolist() == want.tolist() and keep.tolist() == want_keep.tolist()
            out.append((keep, tallies))
        return dict(counts=counts, rows=rows, offsets=offsets, sites=sites, judged=out), ref


def mixed_table(seed=3):
    """Paths with every kind of run on both strands, and a pile-up on one read of each."""
    t = vc.Table(seed)
    for k, (text, to_rc) in enumerate([("5= 2I 3= 1X 4= 3D 6=", 0), ("4= 1X 1D 2= 6I 9=", 1), ("40= 1X 30=", 0), ("3= 70D 2= 1X 5=", 1)]):
        runs = hp.cigar(text)
        s1, s2 = hp.pair_from_runs(t.rng, runs, (k, 2), (1, k))
        x, y = t.read(s1), t.read(rc_bytes(s2) if to_rc else s2)
        t.record(x, y, s2, k, 1, runs, to_rc)
        t.pile(x, {k + 1: vc.other_base(s1[k + 1]), len(s1) - 3: vc.other_base(s1[-3], 2)}, to_rc=k % 2)
    return t


def test_the_six_counters_are_the_corrections_first_six(ms):
    t = mixed_table()
    got, _ = same_as_restatement(ms, t.reads, t.ids, [t.add()], vc.SMALL)
    assert got["counts"]["sites"] > 0
    with api.VariantSession(fasta_of(t.reads, t.ids), handle=ms, **vc.SMALL) as vs, api.CorrectSession(fasta_of(t.reads, t.ids), handle=ms) as cs:
        vs.add(*t.add())
        cs.add(*t.add())
        for r in range(len(t.reads)):
            assert vs.votes(r).tolist() == cs.votes(r)[:, :6].tolist(), r


LENGTHS = [0, 1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5]


def test_sites_on_both_sides_of_every_tile_edge(ms):
    """Reads of every length at which the site kernel's tiles change, in one table; a read's sites sit at its ends and on both sides
    of every tile edge, of every wave's 64 positions inside the first tile and of the four loads of a lane; read `full` is a site
    at every position (more sites in a tile than the workgroup has lanes) and read `none` has votes and no site."""
    t = vc.Table(17)
    wanted = {}
    for n in LENGTHS:
        x = t.random_read(n)
        if n == 0:
            continue
        edges = {0, n - 1} | {e + d for e in range(64, n, 64) for d in (-1, 0) if e < 2 * 256 or e % 256 == 0}
        wanted[x] = sorted(e for e in edges if 0 <= e < n)
        t.pile(x, {e: vc.other_base(t.reads[x][e], 1 + e % 3) for e in wanted[x]}, to_rc=n % 2)
    full = t.random_read(2 * TILE + 1)
    t.pile(full, {e: vc.other_base(t.reads[full][e], 1 + e % 3) for e in range(2 * TILE + 1)})
    none = t.random_read(TILE + 7)
    t.pile(none, {})
    order = sorted(range(len(t.recs)), key=lambda q: (q * 7) % len(t.recs))          # the records of the reads interleaved
    got, ref = same_as_restatement(ms, t.reads, t.ids, [t.add(order)], vc.SMALL)
    off, sites = got["offsets"], got["sites"]
    for x, want in wanted.items():                                                   # the preconditions: the sites are where they were put
        assert sites[off[x]:off[x + 1], 0].tolist() == want, x
    assert sites[off[full]:off[full + 1], 0].tolist() == list(range(2 * TILE + 1)) and 2 * TILE + 1 > 256
    assert off[none + 1] == off[none] and got["rows"][none].tolist() == [0, TILE + 7]
    assert got["rows"][0].tolist() == [0, 0] and len(t.reads[0]) == 0


def chunked_table(to_rc, seed):
    """Paths of 1, 63, 64, 65 and 129 runs, one with a run of 200 columns, one whose runs are long enough that a chunk spells several
    deals of 64 columns; read A has a site on the first and last column of every chunk of runs and of every deal of columns, read B on
    two more, and an N stands in either read on a site column of the other."""
    t = vc.Table(seed)
    specs = [(1, None), (63, None), (64, None), (65, None), (129, None), (5, (2, 200)), (65, (32, 70))]
    checks = []
    for k, (n, long_run) in enumerate(specs):
        runs = vc.alternating_runs(t.rng, n, long_run)
        fa, fb = k % 3, (k + 1) % 2
        s1, s2 = (bytearray(s) for s in hp.pair_from_runs(t.rng, runs, (fa, 2), (fb, 1)))
        cols, i, j, c0 = [], fa, fb, 0                                                # every '=' / 'X' column: (path column in its chunk, i, j)
        for u, r in enumerate(runs):
            length, code = int(r) >> 4, int(r) & 15
            if u % 64 == 0:
                c0 = 0
            for c in range(length):
                if code in (cr.OP_EQ, cr.OP_X):
                    cols.append((c0 + c, i + c, j + c))
            c0 += length
            i += length if code != cr.OP_D else 0
            j += length if code != cr.OP_I else 0
        edge = vc.chunk_edge_columns(runs, fa, fb)
        assert all(code in (cr.OP_EQ, cr.OP_X) for _, _, code in edge)               # the first and last column of a chunk are '=' / 'X'
        on_a = {i for i, _, _ in edge} |{i for c, i, _ in cols if c % 64 in (0, 63)}
        free = [col for col in cols if col[1] not in on_a]
        mid = free[len(free) // 2] if len(cols) > 8 else None
        on_b = {cols[0][2], mid[2]} if mid else set()
        blen = len(s2)
        if mid:                                                                      # an N in B on a site column of A, and in A on one of B
            s2[next(jj for _, ii, jj in cols if ii in on_a and jj not in on_b)] = ord("N")
            s1[mid[1]] = ord("N")
        x = t.read(bytes(s1))
        y = t.read(rc_bytes(bytes(s2)) if to_rc else bytes(s2))
        t.record(x, y, bytes(s2), fa, fb, runs, to_rc)
        j_of = {ii: jj for _, ii, jj in cols}
        # A's second allele is B's byte where the column is an 'X' (the column then disagrees), else another base (it agrees)
        t.pile(x, {i: s2[j_of[i]] if s2[j_of[i]] in vc.ACGT and s2[j_of[i]] != s1[i] else vc.other_base(s1[i], 1 + i % 3) for i in on_a})
        own_b = t.reads[y]
        t.pile(y, {(blen - 1 - jj if to_rc else jj): vc.other_base(own_b[blen - 1 - jj if to_rc else jj], 2) for jj in on_b})
        checks.append((x, y, runs, edge, [i for c, i, _ in cols if c % 64 in (0, 63)], sum(int(r) >> 4 for r in runs[:64]), mid))
    return t, checks


@pytest.mark.parametrize("to_rc", [0, 1], ids=["forward", "reverse"])
def test_informative_columns_on_the_edges_of_chunks_and_deals(ms, to_rc):
    t, checks = chunked_table(to_rc, 23 + to_rc)
    got, ref = same_as_restatement(ms, t.reads, t.ids, [t.add()], vc.SMALL)
    assert [len(c[2]) for c in checks] == [1, 63, 64, 65, 129, 5, 65]
    assert max(int(r) >> 4 for r in checks[5][2]) == 200 and checks[6][5] > 64 and checks[2][5] > 64   # a long run; chunks of more than 64 columns
    kinds = np.zeros(4, np.int64)
    for x, y, runs, edge, deal_edges, _, mid in checks:                               # the preconditions, from the restatement's site bytes
        for i in [i for i, _, _ in edge] + deal_edges:
            assert ref.byte[x][i] is not None, (x, i)
        if mid:                                                                       # A's N stands on a site of B
            assert t.reads[x][mid[1]] == ord("N") and ref.byte[y][len(t.reads[y]) - 1 - mid[2] if to_rc else mid[2]] is not None
    for keep, tallies in got["judged"]:
        kinds += tallies.sum(axis=0)
    assert (kinds > 0).all()                                                          # informative, agree, disagree and other all occur
    assert any(ord("N") in r for r in t.reads)


def test_the_same_records_in_one_call_one_by_one_and_reversed(ms):
    t = mixed_table(9)
    n = len(t.recs)
    whole, _ = same_as_restatement(ms, t.reads, t.ids, [t.add()], vc.SMALL)
    single, _ = same_as_restatement(ms, t.reads, t.ids, [t.add([q]) for q in range(n)], vc.SMALL, judged=[t.add()])
    turned, _ = same_as_restatement(ms, t.reads, t.ids, [t.add(list(range(n))[::-1])], vc.SMALL, judged=[t.add()])
    for other in (single, turned):
        assert other["counts"] == whole["counts"]
        for k in ("rows", "offsets", "sites"):
            assert other[k].tolist() == whole[k].tolist(), k
        assert other["judged"][0][0].tolist() == whole["judged"][0][0].tolist() and other["judged"][0][1].tolist() == whole["judged"][0][1].tolist()


def test_the_cap_of_65535_views_per_target(ms):
    """65 537 records between two reads of 4 bases: each read is the target of 65 537 views, the last two of which are skipped whole."""
    t = vc.Table(1)
    x, y = t.read(b"ACGT"), t.read(b"ACCT")
    t.record(x, y, b"ACCT", 0, 0, hp.cigar("2= 1X 1="), 0, copies=cr.CAP + 2)
    got, ref = same_as_restatement(ms, t.reads, t.ids, [t.add()], vc.SMALL, judged=[t.add(range(3))])
    assert got["counts"]["skipped_views"] == 4 and got["counts"]["accepted_views"] == 2 * cr.CAP
    for r in (x, y):                                                                  # (the session's counters equal these: same_as_restatement)
        assert ref.votes(r)[:, :4].sum(axis=1).tolist() == [cr.CAP] * 4 and ref.votes(r)[:, 5].tolist() == [cr.CAP] * 3 + [0]


IDS, LENS = [1, 2, 3, 4], [100, 200, 0, 300]
EQ = lambda n: (n << 4) | 7   # noqa: E731
GOOD_RUNS = ([0, 1, 2], [EQ(50), EQ(100)])


def four_reads():
    rng = np.random.default_rng(7)
    return [bytes(int(c) for c in rng.choice(list(vc.ACGT), n)) for n in LENS]


def says(call, text):
    with pytest.raises(api.MhapError) as e:
        call()
    assert str(e.value) == text


def test_refusals_each_leaving_the_session_usable(ms):
    import string_graph_ref as sg
    good = [sg.record(1, 2, 0, 49, 100, 10, 59, 200, 0), sg.record(2, 4, 0, 99, 200, 0, 99, 300, 1)]
    unknown = sg.record(1, 9, 0, 49, 100, 10, 59, 200, 0)
    wrong_length = sg.record(1, 2, 0, 49, 101, 10, 59, 200, 0)
    batch = lambda *r: np.concatenate(r)   # noqa: E731
    reads = four_reads()
    fa = fasta_of(reads, IDS)
    rule = "mhap_variant_begin: min_depth, min_minor and min_diff must be >= 1 and min_pct, max_del_pct and diff_pct 0 .. 100"
    for name, value in (("min_depth", 0), ("min_minor", 0), ("min_pct", 101), ("max_del_pct", -1), ("min_diff", 0), ("diff_pct", 101)):
        p = dict(vc.SMALL, **{name: value})
        says(lambda: api.VariantSession(fa, handle=ms, **p), f"{rule} ({', '.join(str(p[k]) for k in vr.PARAMETERS)}) (code -1)")
    ref = vr.Variants(reads, IDS, **vc.SMALL)
    with api.VariantSession(fa, handle=ms, **vc.SMALL) as vs:
        says(lambda: vs.apply(batch(*good), *GOOD_RUNS), "mhap_variant_apply: no mhap_variant_finish has completed (code -1)")
        says(vs.table, "mhap_variant_copy: no mhap_variant_finish has completed (code -1)")
        three = ([0, 1, 2, 3], [EQ(50), EQ(100), EQ(50)])
        says(lambda: vs.add(batch(*good, unknown), *three), "mhap_variant_add: record 2 names read 9, which is not among the reads (code -1)")
        says(lambda: vs.add(batch(*good, wrong_length), *three), "mhap_variant_add: record 2 gives read 1 the length 101, the reads say 100 (code -1)")
        says(lambda: vs.add(batch(*good, good[0]), [0, 1, 2, 3], [EQ(50), EQ(100), EQ(49)]),
             "mhap_variant_add: record 2 has runs that are not a path between its aligned ends (code -1)")
        says(lambda: vs.add(batch(*good), [0, 1, 2, 3], [EQ(50), EQ(100), EQ(50)]), "VariantSession.add: 2 records need 3 run offsets, not 4")
        vs.add(batch(*good), *GOOD_RUNS)                                         # the refused calls have cast no vote
        ref.add(batch(*good), *GOOD_RUNS)
        for r in range(4):
            assert vs.votes(r).astype(np.int64).tolist() == ref.votes(r).tolist()
        counts = vs.finish()
        assert [counts[k] for k in api.VARIANT_COUNTS] == ref.finish() and counts["accepted_views"] == 4
        says(lambda: vs.add(batch(*good), *GOOD_RUNS),
             "mhap_variant_add: mhap_variant_finish has completed, and its sites are those of the votes before it (code -1)")
        says(lambda: vs.apply(batch(*good, unknown), *three), "mhap_variant_apply: record 2 names read 9, which is not among the reads (code -1)")
        keep, tallies = vs.apply(batch(*good), *GOOD_RUNS)
        assert keep.tolist() == [1, 1] and tallies.tolist() == ref.apply(batch(*good), *GOOD_RUNS)[1].tolist()
        assert vs.finish() == counts                                              # a finish may be repeated
    with api.VariantSession(fasta_of([], []), handle=ms, **vc.SMALL) as vs:        # a session of no reads
        assert vs.finish()["reads"] == 0 and vs.table()[0].shape == (0, 2)
        assert vs.apply(np.zeros(0, api.RECORD_DTYPE), [0], [])[0].shape == (0,)


DIPLOID = dict(min_depth=4, min_minor=2, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # six reads deep at the most


def test_the_error_free_planted_diploid(ms):
    """The truth gate: 15 error-free reads of 4 kb per haplotype, a substitution every 400 bases, every pair that shares 1 kb realigned
    by the GPU aligner.  The session equals the restatement byte for byte, and the four statements hold exactly."""
    d = vc.planted_diploid()
    found = vc.layout_records(d)
    fa = fasta_of(d["reads"], d["ids"])
    out, _, op_offsets, ops = api.realign_records_paths(found, fa, handle=ms)
    assert len(kept_rows(out)) == len(found)                                      # every layout record has an alignment
    got, ref = same_as_restatement(ms, d["reads"], d["ids"], [(out, op_offsets, ops)], DIPLOID)
    keep, tallies = got["judged"][0]
    cross, aside = vc.check_truth(d, out, got["offsets"], got["sites"], keep, DIPLOID, vr.site_of)
    print(f"planted diploid: {len(out)} overlaps, {cross} cross-haplotype, {aside} set aside; {got['counts']}")
    assert got["counts"]["sites"] > 0 and 0 < aside <= cross
