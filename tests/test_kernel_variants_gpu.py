"""Every MinHash and index-build kernel variant behind an A/B switch against the oracle, with proof that the variant ran.

The switches (MHAP_MINHASH, MHAP_W1_TAIL_DIV, MHAP_W1_STAGGER at every MinHash launch; MHAP_INDEX_TILE, MHAP_INDEX_BINS_SHAPE at every index
build) are read per launch, so a test can set them inside one process.  With MHAP_HOST_PROF set the library prints one witness line per launch:
  [minhash] strands S weight-1 U weighted W nblocks B: weight-1 launch (none | classic | w1 n_whole A n_tail T rmax R stagger G); weighted launch (none | split | wave)
  [minhash] strands S weight-1 U weighted W nblocks B: perchain
  [index build] entries E tile_entries TE tiles T sub SUB bins_shape X grouped G lines L
Every case compares each strand's sketch, or the sorted records, with the oracle itself (a variant that only agrees with the default path
proves nothing) and asserts the witness lines of the launches it made.

Index shapes (search_kernels.hip): nb = 2^max(10, ceil(log2 entries)) buckets per slot, at most 2^20; sub = nb / 128 buckets per coarse bin; the bins
kernel <512, 64> / <2048, 256> / <8192, 256> (shape 0 / 1 / 2) is the smallest that holds sub, a pinned shape that does not fit falls back to the next
one that does.  Tiles of 1 024 entries up to 65 536 entries, 4 096 above.  Line table for 8 192 ... 2^18 entries, class-ordered (grouped) buckets above 2^18.
"""
import random
import re

import numpy as np
import pytest

import mhap_amd
import oracle_lib as O
import sketch_search_ref as R
from mhap_amd import FastaData, MhapParams, MinHashSearch
from test_small_grids_gpu import _expected_sketches, _rand_seq, _sketch_mismatches, _w1_reads

pytestmark = pytest.mark.gpu

MINHASH_SWITCHES = ("MHAP_MINHASH", "MHAP_NUM_CUS", "MHAP_MINHASH_WGS_PER_CU", "MHAP_W1_TAIL_DIV", "MHAP_W1_STAGGER", "MHAP_BATCH_BASES",
                    "MHAP_MINHASH_SPLIT")
INDEX_SWITCHES = ("MHAP_INDEX_TILE", "MHAP_INDEX_BINS_SHAPE")
MH_RE = re.compile(r"^\[minhash\] strands (\d+) weight-1 (-?\d+) weighted (-?\d+) nblocks (\d+): (.*)$")
W1_RE = re.compile(r"^weight-1 launch (none|classic|w1 n_whole (\d+) n_tail (\d+) rmax (\d+) stagger (\d+)); weighted launch (none|split|wave)$")
IX_RE = re.compile(r"^\[index build\] entries (\d+) tile_entries (\d+) tiles (\d+) sub (\d+) bins_shape (\d) grouped (\d) lines (\d)$")
CHECK_RE = re.compile(r"^\[index\] self-check: (\d+) of (\d+) postings missing$")
BINS_SUB = (512, 2048, 8192)   # largest sub of each bins shape


def _env(monkeypatch, names, env):
    for k in names:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _lines(capfd, regex):
    _, err = capfd.readouterr()
    return [m for m in (regex.match(x) for x in err.splitlines()) if m]


def _minhash_witness(capfd):
    """The launches' witness lines since the last read: dicts with the counts, `path` (w1 / classic / perchain / none) and `weighted`."""
    out = []
    for m in _lines(capfd, MH_RE):
        d = dict(strands=int(m[1]), unweighted=int(m[2]), weighted_n=int(m[3]), nblocks=int(m[4]))
        if m[5] == "perchain":
            d.update(path="perchain", weighted=None)
        else:
            w = W1_RE.match(m[5])
            assert w, m[0]
            d.update(path=w[1].split()[0], weighted=w[6])
            if d["path"] == "w1":
                d.update(n_whole=int(w[2]), n_tail=int(w[3]), rmax=int(w[4]), stagger=int(w[5]))
        out.append(d)
    return out


def _assert_path(wit, mode, split_ok=True):
    """Every launch ran `mode`'s kernels: the bit-sliced w1 kernel (default), the general kernel for the weight-1 strands too (classic), or
    the per-chain kernels for both lists (perchain); a weighted launch splits its strands over a workgroup's waves exactly when the
    rule of launch_minhash allows it."""
    assert wit, "no [minhash] witness line: MHAP_HOST_PROF not honoured?"
    for d in wit:
        assert 0 <= d["unweighted"] and 0 <= d["weighted_n"] and d["unweighted"] + d["weighted_n"] <= d["strands"], d
        if mode == "perchain":
            assert d["path"] == "perchain", d
            continue
        want = ("w1" if mode == "default" else "classic") if d["unweighted"] > 0 else "none"
        assert d["path"] == want, (mode, d)
        if d["weighted_n"] == 0:
            assert d["weighted"] == "none", d
        else:
            split = split_ok and 4 * d["weighted_n"] <= d["nblocks"]
            assert d["weighted"] == ("split" if split else "wave"), (mode, split_ok, d)
        if d["path"] == "w1":
            assert d["n_whole"] + d["n_tail"] == d["unweighted"], d


# ---- MinHash variants ----------------------------------------------------------------------------------------------------------
def _variant_corpus():
    """Weight-1 strands at the row edges (2 047 / 2 048 / 2 049 / 4 096 / 4 097 k-mers) and one of 30 kb, strands shorter than k, tandem
    repeats of multiplicity 2 to 40 (the weight classes), a read whose first 900 bases are one k-mer (the per-chain rows), raw-byte strands
    with N, and random weight-1 reads between."""
    rnd = random.Random(8118)
    seqs = _w1_reads(rnd, [nk + 15 for nk in (2047, 2048, 2049, 4096, 4097)] + [30000])
    seqs += [_rand_seq(rnd, n) for n in (1, 5, 15)]
    for reps in (2, 3, 5, 7, 12, 40):
        unit = _rand_seq(rnd, 40)
        seqs.append(_rand_seq(rnd, 1300) + unit * reps + _rand_seq(rnd, 1100))
    seqs.append("A" * 900 + _rand_seq(rnd, 2500))
    seqs += [_rand_seq(rnd, 3000, "ACGTN"), _rand_seq(rnd, 800, "ACGTN")]
    seqs += _w1_reads(rnd, [(300, 700, 1500, 2500, 3600)[i % 5] for i in range(40)])
    return FastaData.from_strings(seqs)


def _sketch(monkeypatch, capfd, fa, p, env, flt=None):
    _env(monkeypatch, MINHASH_SWITCHES, env)
    monkeypatch.setenv("MHAP_HOST_PROF", "1")
    capfd.readouterr()
    with MinHashSearch(p, kmer_filter=flt) as ms:
        sk = ms.sketch(fa)
    wit = _minhash_witness(capfd)
    _env(monkeypatch, MINHASH_SWITCHES + ("MHAP_HOST_PROF",), {})
    return sk, wit


MODES = {"default": {}, "perchain": {"MHAP_MINHASH": "perchain"}, "classic": {"MHAP_MINHASH": "classic"}}


@pytest.mark.parametrize("H", [16, 33, 512, 1024, 3000])
def test_minhash_variants_against_the_oracle(H, monkeypatch, capfd):
    """default / perchain / classic on the full grid and on two CUs: every strand's sketch equals the oracle's (J/sketch/MinHashSketch.java),
    and the witness shows the variant's kernels (H = 3 000 still has four waves per workgroup: the w1 kernel is the default)."""
    fa = _variant_corpus()
    p = MhapParams(num_hashes=H, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p)
    seen = set()
    for cap in (None, 2):
        for mode, env in MODES.items():
            sk, wit = _sketch(monkeypatch, capfd, fa, p, dict(env, **({"MHAP_NUM_CUS": cap} if cap else {})))
            bad = _sketch_mismatches(fa, p, sk, exp)
            assert not bad, f"H {H}, {mode}, cap {cap}: {len(bad)} strands differ from the oracle, first {bad[:8]}"
            _assert_path(wit, mode)
            assert len(wit) == 1, wit                                   # one launch group
            assert wit[0]["unweighted"] > 0 and wit[0]["weighted_n"] > 0, wit
            seen |= {(mode, d["weighted"]) for d in wit}
            if mode == "default":
                assert wit[0]["n_tail"] > 0 and wit[0]["rmax"] == (30000 - 15 + 2047) // 2048, wit
                assert (wit[0]["n_whole"] > 0) == (cap == 2), (cap, wit)   # two CUs: fewer resident waves than weight-1 strands
    assert {("default", "split"), ("default", "wave"), ("classic", "split"), ("classic", "wave")} <= seen, seen


def _tfidf_filter():
    """-f with --repeat-idf-scale 12 and no tf: every k-mer outside the (tiny) filter gets weight 12, every strand is weighted."""
    rnd = random.Random(11)
    kmers = [_rand_seq(rnd, 16) for _ in range(20)]
    hashes = np.array([int(O.kmer_hashes64(k, 16, True)[0]) for k in kmers], dtype=np.int64)
    fracs = np.linspace(2e-3, 1e-4, len(kmers))
    return mhap_amd.FrequencyCounts(hashes, fracs, 1e-5, 0.9, 12.0, True), O.Filter(hashes, fracs, 1e-5, 0.9, 12.0, True)


def _long_weighted_batch():
    """The launch's longest strand is weighted (30 kb with tandem repeats) and its weight-1 strands are short: rmax is large and most
    row items of the tail are empty."""
    rnd = random.Random(9229)
    unit = _rand_seq(rnd, 50)
    seqs = [_rand_seq(rnd, 14000) + unit * 9 + _rand_seq(rnd, 15550)]
    seqs += _w1_reads(rnd, [(200, 450, 900)[i % 3] for i in range(60)])
    return FastaData.from_strings(seqs)


@pytest.mark.parametrize("mode", list(MODES))
def test_minhash_variants_in_batches_unsplit_filtered_and_long_weighted(mode, monkeypatch, capfd):
    """Each variant (H = 512) with several launch groups (MHAP_BATCH_BASES), with MHAP_MINHASH_SPLIT=0, under a tf-idf -f filter
    (weight 12: every strand in the weighted launch) and on a batch whose longest strand is weighted while its weight-1 strands are short."""
    fa = _variant_corpus()
    p = MhapParams(num_hashes=512, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p)
    env = MODES[mode]

    sk, wit = _sketch(monkeypatch, capfd, fa, p, dict(env, MHAP_BATCH_BASES=20000))
    assert not _sketch_mismatches(fa, p, sk, exp), (mode, "batches")
    _assert_path(wit, mode)
    assert len(wit) >= 5 and sum(d["strands"] for d in wit) == 2 * len(fa), wit

    sk, wit = _sketch(monkeypatch, capfd, fa, p, dict(env, MHAP_MINHASH_SPLIT=0))
    assert not _sketch_mismatches(fa, p, sk, exp), (mode, "no split")
    _assert_path(wit, mode, split_ok=False)
    assert mode == "perchain" or wit[0]["weighted"] == "wave", wit

    flt, oflt = _tfidf_filter()
    exp_f = _expected_sketches(fa, p, oflt)
    sk, wit = _sketch(monkeypatch, capfd, fa, p, env, flt=flt)
    assert not _sketch_mismatches(fa, p, sk, exp_f), (mode, "-f")
    _assert_path(wit, mode)
    assert wit[0]["unweighted"] <= 6 and wit[0]["weighted_n"] >= 2 * len(fa) - 6, wit   # (the six strands shorter than k aside)

    fl = _long_weighted_batch()
    exp_l = _expected_sketches(fl, p)
    for cap in (None, 2):
        sk, wit = _sketch(monkeypatch, capfd, fl, p, dict(env, **({"MHAP_NUM_CUS": cap} if cap else {})))
        assert not _sketch_mismatches(fl, p, sk, exp_l), (mode, "long weighted", cap)
        _assert_path(wit, mode)
        assert wit[0]["weighted_n"] == 2, wit
        if mode == "default":
            assert wit[0]["rmax"] == (30000 - 15 + 2047) // 2048 and wit[0]["n_tail"] > 0, wit


# ---- the weight-1 tail split ---------------------------------------------------------------------------------------------------
def test_w1_tail_split_and_stagger(monkeypatch, capfd):
    """MHAP_W1_TAIL_DIV: the last min(n_unweighted, 4 nblocks / div) strands of the weight-1 list are cut into row items whose minima
    meet in the merge buffer (minhash_w1_finish_kernel); div 2^20 cuts none (no merge, no finish kernel).  On two and eight CUs at four
    workgroups per CU, and once with MHAP_W1_STAGGER=325; the sketches equal the oracle's every time."""
    rnd = random.Random(4554)
    fa = FastaData.from_strings(_w1_reads(rnd, [(300, 700, 1500, 2063, 2064, 3000, 4300, 6200, 9000)[i % 9] for i in range(180)]))
    p = MhapParams(num_hashes=128, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p)
    n_unweighted = 2 * len(fa)
    tails = set()
    for cap in (2, 8):
        nblocks = 4 * cap
        for div, stagger in ((1, None), (2, None), (5, None), (1 << 20, None)) + (((1, 325),) if cap == 8 else ()):
            env = {"MHAP_NUM_CUS": cap, "MHAP_MINHASH_WGS_PER_CU": 4, "MHAP_W1_TAIL_DIV": div}
            if stagger is not None:
                env["MHAP_W1_STAGGER"] = stagger
            sk, wit = _sketch(monkeypatch, capfd, fa, p, env)
            bad = _sketch_mismatches(fa, p, sk, exp)
            assert not bad, f"cap {cap}, div {div}, stagger {stagger}: {len(bad)} strands differ from the oracle, first {bad[:8]}"
            _assert_path(wit, "default")
            assert len(wit) == 1, wit
            d = wit[0]
            assert d["nblocks"] == nblocks and d["unweighted"] == n_unweighted, d
            assert d["n_tail"] == min(n_unweighted, 4 * nblocks // div), (cap, div, d)
            assert d["stagger"] == (stagger or 0) and d["rmax"] == (9000 - 15 + 2047) // 2048, d
            tails.add(d["n_tail"])
    assert 0 in tails and {32, 16, 6, 128, 64, 25} <= tails, tails


# ---- index build on reads ------------------------------------------------------------------------------------------------------
def _index_reads():
    """1 500 reads plus 300 that carry one 400-base repeat (long buckets), as test_gpu_parity's line-table test."""
    rnd = random.Random(77)
    fa1 = mhap_amd.synth_reads(1500, 3000, seed=77, error_rate=0.10)
    rep = _rand_seq(rnd, 400)
    extra = [_rand_seq(rnd, 900) + rep + _rand_seq(rnd, 700) for _ in range(300)]
    return FastaData.from_strings([fa1.sequence(i) for i in range(len(fa1))] + extra)


def _index_witness(capfd):
    _, err = capfd.readouterr()
    lines = err.splitlines()
    builds = [m for m in (IX_RE.match(x) for x in lines) if m]
    checks = [m for m in (CHECK_RE.match(x) for x in lines) if m]
    return [dict(entries=int(m[1]), te=int(m[2]), tiles=int(m[3]), sub=int(m[4]), shape=int(m[5]), grouped=int(m[6]), lines=int(m[7]))
            for m in builds], [(int(m[1]), int(m[2])) for m in checks]


def _fitting_shape(sub, pinned):
    return min(s for s in range(3) if s >= pinned and sub <= BINS_SUB[s])


def test_index_build_tiles_and_bins_shapes_on_reads(monkeypatch, capfd):
    """MHAP_INDEX_TILE 256 / 300 / 1 024 / 4 096 x MHAP_INDEX_BINS_SHAPE 0 / 1 / 2 on 3 600 entries (sub 32: every shape fits) with the
    self-check on: nothing missing, records equal the oracle's, and the same candidates and table elements in every build."""
    fa = _index_reads()
    H, S = 128, 500
    p = MhapParams(num_hashes=H, ordered_sketch_size=S)
    want = O.run_self(fa, H=H, S=S, nthreads=16, cap=1 << 22)
    want_lines = O.record_lines(want["records"])
    assert len(want_lines) > 3000
    ne = 2 * len(fa)
    seen = set()
    for te in (256, 300, 1024, 4096):
        for shape in (0, 1, 2):
            _env(monkeypatch, INDEX_SWITCHES, {"MHAP_INDEX_TILE": te, "MHAP_INDEX_BINS_SHAPE": shape})
            monkeypatch.setenv("MHAP_DEBUG_INDEX", "1")
            monkeypatch.setenv("MHAP_HOST_PROF", "1")
            capfd.readouterr()
            with MinHashSearch(p) as ms:
                ms.add_data(fa)
                got = sorted(mhap_amd.records_to_lines(ms.find_matches()))
                st = ms.stats()
            builds, checks = _index_witness(capfd)
            assert got == want_lines, (te, shape, len(got), len(want_lines))
            assert builds == [dict(entries=ne, te=te, tiles=-(-ne // te), sub=32, shape=shape, grouped=0, lines=0)], (te, shape, builds)
            assert checks == [(0, ne * H)], checks
            assert st["candidates_compared"] == want["compared"], (te, shape, st)
            seen.add((st["candidates_compared"], st["table_elements"], st["matches_found"]))
    assert len(seen) == 1, seen
    _env(monkeypatch, INDEX_SWITCHES + ("MHAP_DEBUG_INDEX", "MHAP_HOST_PROF"), {})


# ---- index build at the size edges, on crafted sketches ------------------------------------------------------------------------
SIZE_EDGES = [65536, 65537, 262144, 262145, (1 << 20) + 4097]
EDGE_H, EDGE_S = 16, 8
EDGE_KW = dict(H=EDGE_H, k2=12, num_min_matches=3, min_store_length=0, threshold=0.0, max_shift=0.2)


def _unique_values(rng, n, reserved):
    """n distinct int32 values, none of them in `reserved`, in random order."""
    x = rng.integers(R.INT32_MIN, R.INT32_MAX, size=n + n // 50 + 1024, endpoint=True, dtype=np.int64)
    x = x[~np.isin(x, reserved)]
    _, first = np.unique(x, return_index=True)
    x = x[np.sort(first)]
    assert len(x) >= n
    return x[:n]


def _edge_tables(ne, seed):
    """ne entries of H = 16: 150 crafted pairs with one shared MinHash row (exact copies; every fourth pair's stored entry a reverse strand),
    five groups of 40 entries that share 2 of their 16 slot values (below num_min_matches 3: long buckets, no candidates), and every other slot
    value unique in its column.  Returns the table, the candidate pairs (every ordered pair of a copy with a forward query) and the duplicates
    each column holds by construction."""
    c = R.Corpus(EDGE_S, H=EDGE_H, seed=seed)
    for i in range(150):
        c.pair(f"copy {i}", joined=int(c.rng.integers(1, 7)), seqlen_a=int(c.rng.integers(40, 400)), seqlen_b=int(c.rng.integers(40, 400)),
               shift=int(c.rng.integers(-5, 6)), rev_b=i % 4 == 3)
    crafted, _ = c.tables()
    groups = [(int(a), int(b)) for a, b in ((0, 1), (3, 9), (15, 14), (7, 8), (2, 12))]
    shared = [c.hs.take(2) for _ in groups]
    rng = np.random.default_rng(seed + 1)
    nc, ng = len(crafted["ids"]), 40 * len(groups)
    assert nc + ng < ne
    t = {"ids": np.arange(1, ne + 1, dtype=np.int64), "is_fwd": np.ones(ne, np.uint8), "seq_length": np.full(ne, 8 + 11, np.int32),
         "minhash": np.zeros((ne, EDGE_H), np.int32), "ordered": np.zeros((ne, EDGE_S, 2), np.int32),
         "ordered_size": np.full(ne, EDGE_S, np.int32), "ordered_seqlen": np.full(ne, EDGE_S, np.int32)}
    t["ordered"][:, :, 0] = np.sort(rng.integers(R.INT32_MIN, R.INT32_MAX, size=EDGE_S))     # one valid row for every filler entry
    t["ordered"][:, :, 1] = np.arange(EDGE_S)
    reserved = np.array(sorted(c.hs.used), dtype=np.int64)
    for s in range(EDGE_H):
        t["minhash"][:, s] = _unique_values(rng, ne, reserved)
    rows = rng.permutation(ne)                       # planted rows anywhere in the index (first and last tiles included)
    crow, grow = rows[:nc], rows[nc:nc + ng]
    for k in ("is_fwd", "seq_length", "minhash", "ordered", "ordered_size", "ordered_seqlen"):
        t[k][crow] = crafted[k]
    t["ids"][crow] = ne + crafted["ids"]             # (a pair keeps its id order: the larger id asks)
    for gi, ((s1, s2), (v1, v2)) in enumerate(zip(groups, shared)):
        g = grow[40 * gi:40 * (gi + 1)]
        t["minhash"][g, s1] = v1
        t["minhash"][g, s2] = v2
    dups = np.zeros(EDGE_H, np.int64)
    dups += 150                                      # a copy pair: one value twice in every column
    for s1, s2 in groups:
        dups[s1] += 39
        dups[s2] += 39
    pairs = []
    for a, b in c.notes.values():
        for q, m in ((a, b), (b, a)):
            if crafted["is_fwd"][q]:
                pairs.append((int(crow[q]), int(crow[m])))
    return t, pairs, dups


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("ne", SIZE_EDGES)
def test_index_build_at_the_size_edges(ne, monkeypatch, capfd):
    """The index build where its defaults switch over: 65 536 / 65 537 entries (bins shape 0 -> 1, tiles 1 024 -> 4 096), 262 144 / 262 145
    (shape 1 -> 2, line table and grouping), 2^20 + 4 097 (more entries than the 2^20 buckets).  Defaults, then every shape that fits at the
    default tile and at 256, and every pinned shape that does not fit (the witness shows the fallback): witness, self-check, records of the
    known pairs against sketch_search_ref, candidates by their closed form."""
    t, pairs, dups = _edge_tables(ne, seed=ne % 1000)
    for s in range(EDGE_H):
        assert len(np.unique(t["minhash"][:, s])) == ne - dups[s], s
    want, compared = R.expected_records(t, return_compared=True, pairs=pairs, **EDGE_KW)
    assert compared == 150 and len(want) == compared                    # each copy pair once (the larger id asks); threshold 0
    lg = max(10, min(20, (ne - 1).bit_length()))
    sub = (1 << lg) >> 7
    default_shape = _fitting_shape(sub, 0)
    default_te = 1024 if ne <= 65536 else 4096
    assert (default_shape, default_te) == {65536: (0, 1024), 65537: (1, 4096), 262144: (1, 4096), 262145: (2, 4096)}.get(ne, (2, 4096))
    # (a pinned shape too small for sub falls back to the next one that holds it: once, at the default tile)
    runs = [(None, None)] + [(shape, te) for shape in range(3) for te in ((None, 256) if sub <= BINS_SUB[shape] else (None,))]
    p = MhapParams(num_hashes=EDGE_H, ordered_kmer_size=12, ordered_sketch_size=EDGE_S, num_min_matches=3, min_store_length=0,
                   threshold=0.0, max_shift=0.2)
    for shape, te in runs:
        env = {}
        if shape is not None:
            env["MHAP_INDEX_BINS_SHAPE"] = shape
        if te is not None:
            env["MHAP_INDEX_TILE"] = te
        _env(monkeypatch, INDEX_SWITCHES, env)
        monkeypatch.setenv("MHAP_DEBUG_INDEX", "1")
        monkeypatch.setenv("MHAP_HOST_PROF", "1")
        capfd.readouterr()
        with MinHashSearch(p) as ms:
            ms.add_sketches(t)
            got = sorted(mhap_amd.records_to_lines(ms.find_matches()))
            st = ms.stats()
        builds, checks = _index_witness(capfd)
        tile = te or default_te
        assert builds == [dict(entries=ne, te=tile, tiles=-(-ne // tile), sub=sub, shape=_fitting_shape(sub, shape or 0),
                               grouped=int(ne > 1 << 18), lines=int(8192 <= ne <= 1 << 18))], (ne, shape, te, builds)
        assert checks == [(0, ne * EDGE_H)], checks
        assert st["candidates_compared"] == compared, (ne, shape, te, st)
        assert got == want, (ne, shape, te, len(got), len(want), sorted(set(want) - set(got))[:3], sorted(set(got) - set(want))[:3])
    _env(monkeypatch, INDEX_SWITCHES + ("MHAP_DEBUG_INDEX", "MHAP_HOST_PROF"), {})


# ---- switches that must not change results ------------------------------------------------------------------------------------
def test_length_order_eager_index_and_own_count_switches(monkeypatch):
    """MHAP_NO_LENGTH_ORDER (a batch of clearly different read lengths: min_len 5 < max_len 4, so the default hands reads out longest
    first), MHAP_NO_EAGER_INDEX (the index is built at search time instead of during the add) and MHAP_COUNT_OWN (a self search counts
    the query's own strand again): records equal the oracle's in every case."""
    fa0 = mhap_amd.synth_reads(500, 4000, seed=515, error_rate=0.08)
    rng = np.random.default_rng(515)
    seqs = []
    for i in range(len(fa0)):
        s = fa0.sequence(i)
        seqs.append(s[:int(rng.integers(900, 2500))] if i % 3 == 0 else s)
    fa = FastaData.from_strings(seqs)
    assert int(fa.lengths.min()) * 5 < int(fa.lengths.max()) * 4
    p = MhapParams(num_hashes=128, ordered_sketch_size=500)
    want = O.run_self(fa, H=128, S=500, nthreads=16)
    want_lines = O.record_lines(want["records"])
    assert len(want_lines) > 1000
    switches = ("MHAP_NO_LENGTH_ORDER", "MHAP_NO_EAGER_INDEX", "MHAP_COUNT_OWN")
    for env in ({}, {"MHAP_NO_LENGTH_ORDER": "1"}, {"MHAP_NO_EAGER_INDEX": "1"}, {"MHAP_COUNT_OWN": "1"}):
        _env(monkeypatch, switches, env)
        with MinHashSearch(p) as ms:
            ms.add_data(fa)
            got = sorted(mhap_amd.records_to_lines(ms.find_matches()))
            st = ms.stats()
        assert got == want_lines, (env, len(got), len(want_lines))
        assert st["candidates_compared"] == want["compared"], (env, st)
    _env(monkeypatch, switches, {})
