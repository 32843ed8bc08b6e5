"""Persistent kernels on small grids (MHAP_NUM_CUS): every persistent grid is sized from the handle's compute units, and with the count
capped at a few CUs every worker takes several items from its counter, so the resets between two items run.  On the full device almost every
test corpus is smaller than the grid.  Each case checks against the references the suite already trusts (the oracle, tests/align_ref.py,
tests/ksim_ref.py) and asserts, with the bound written out, that its work items outnumber the grid the cap allows.

Grid bounds at cap c (upper bounds, not mirrors of the occupancy rules):
  weight kernel        <= 2 c workgroups (one read, or one strand under -f, per item)
  MinHash launches     <= 8 c workgroups of 4 waves = 32 c waves (one strand, or one row of a strand, per item)
  aligner              <= 2 c four-wave and <= 8 c one-wave workgroups (one pair per item)
  k-mer statistics     <= 4 c LDS and <= 2 c HBM workgroups (one pair per item)
  join kernel          <= 32 c waves (a CU holds at most 32), at most 8 candidates per pull
"""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import align_ref
import ksim_ref as R
import mhap_amd
import oracle_lib as O
from mhap_amd import FastaData, MhapParams, MinHashSearch
from mhap_amd import kmer_sim as K

pytestmark = pytest.mark.gpu

CAPS = (1, 2, 3, 7, 32)
WGS_PER_CU = (1, 8)
WEIGHT_WG_PER_CU = 2
MINHASH_WAVES_PER_CU = 32
ALIGN_BIG_PER_CU, ALIGN_SMALL_PER_CU = 2, 8
KSIM_LDS_PER_CU, KSIM_HBM_PER_CU = 4, 2
JOIN_WAVES_PER_CU, JOIN_CHUNK = 32, 8
ALIGN_PASS_ROWS = 4 * 64 * 8     # s1 rows one pass of the four-wave aligner holds; longer s1 keeps rows in HBM between passes


def _rand_seq(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def _rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _no_repeated_kmer(s, k=16):
    """No k-mer occurs twice, in either orientation: both strands of the read are weight-1 strands."""
    fw = {s[i:i + k] for i in range(len(s) - k + 1)}
    if len(fw) < len(s) - k + 1:
        return False
    return not any(_rc(x) in fw for x in fw)


def _w1_reads(rnd, lengths):
    out = []
    for n in lengths:
        s = _rand_seq(rnd, n)
        while not _no_repeated_kmer(s):
            s = _rand_seq(rnd, n)
        out.append(s)
    return out


def _expected_sketches(fa, p, oflt=None):
    """The oracle's (minhash rc, row, ordered rc, rows) of every strand (J/sketch/MinHashSketch.java, OrderedNGramHashes)."""
    def one(i):
        seq = fa.sequence(i)
        out = []
        for s in (seq, O.rc(seq)):
            rc1, mh = O.minhash(s, p.kmer_size, p.num_hashes, p.repeat_weight, oflt)
            rc2, od, _ = O.ordered(s, p.ordered_kmer_size, p.ordered_sketch_size)
            out.append((rc1, mh.tolist(), rc2, od.tolist()))
        return out
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, range(len(fa))))


def _sketch_mismatches(fa, p, sk, exp):
    """Strands whose sketch differs from the oracle's (the rules of test_gpu_parity._assert_sketch_parity)."""
    bad = []
    for i in range(len(fa)):
        L = int(fa.lengths[i])
        for strand in (0, 1):
            e = 2 * i + strand
            rc1, mh, rc2, od = exp[i][strand]
            st = int(sk["status"][e])
            if L < p.min_olap_length:
                ok = st == 2
            elif strand == 1 and sk["status"][e - 1] != 0:
                ok = st != 0
            elif rc1 or rc2:
                ok = st == 1
            else:
                n = int(sk["ordered_size"][e])
                ok = st == 0 and sk["minhash"][e].tolist() == mh and n == len(od) and sk["ordered"][e, :n].tolist() == od
            if not ok:
                bad.append(e)
    return bad


def _sweep_sketches(monkeypatch, fa, p, exp, flt=None, check=None):
    """Sketches of fa at every cap and MinHash workgroups per CU against the oracle's; check(cap, wgs) asserts the case's bounds."""
    for cap in CAPS:
        for wgs in WGS_PER_CU:
            monkeypatch.setenv("MHAP_NUM_CUS", str(cap))
            monkeypatch.setenv("MHAP_MINHASH_WGS_PER_CU", str(wgs))
            if check:
                check(cap, wgs)
            with MinHashSearch(p, kmer_filter=flt) as ms:
                sk = ms.sketch(fa)
            bad = _sketch_mismatches(fa, p, sk, exp)
            assert not bad, f"cap {cap}, {wgs} MinHash workgroups per CU: {len(bad)} strands differ from the oracle, first {bad[:8]}"


def _w1_corpus():
    """Random reads without a repeated k-mer — every strand is a weight-1 strand — of mixed length: reads shorter than k, reads of more than
    2 048 k-mers (the w1 kernel's tail cuts them into several row items) and everything between."""
    rnd = random.Random(3113)
    lengths = [(10, 15, 16, 300, 900, 1500, 2063, 2064, 2100, 3000, 4200, 4300, 6200, 9000)[i % 14] for i in range(560)]
    return FastaData.from_strings(_w1_reads(rnd, lengths))


@pytest.mark.parametrize("H", [16, 512, 1024, 3000, 4000])
def test_weight1_sketches_on_small_grids(H, monkeypatch):
    """The weight kernel (a READ per item: a read without repeats settles both strands) and the MinHash launches on 1 120 weight-1 strands.
    H <= 3 000: the w1 kernel, whole strands first, then the tail's row items (n_whole > 0 and n_tail > 0 at every cap); H = 4 000: four
    waves' slot tables no longer fit a workgroup's LDS (from about 3 100 on), the general kernel takes the strands with fewer waves per
    workgroup and as many waves in all."""
    fa = _w1_corpus()
    p = MhapParams(num_hashes=H, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p)
    n_reads = len(fa)
    n_unweighted = 2 * n_reads      # (strands shorter than k are on the weight-1 list too)
    assert int(fa.lengths.max()) - 16 + 1 > 2 * 2048      # rmax >= 3: a tail strand has several row items

    def check(cap, wgs):
        assert n_reads > 4 * WEIGHT_WG_PER_CU * cap                # weight kernel: >= 4 reads per workgroup
        waves = MINHASH_WAVES_PER_CU * cap                        # MinHash: <= 8 c workgroups of 4 waves
        n_tail = min(n_unweighted, waves)                          # minhash_tail_strands: a strand's worth of rows per resident wave, at most
                                                                   # (the general kernel, H = 4 000: more strands than waves)
        n_whole = n_unweighted - n_tail
        assert n_unweighted > waves and n_whole > 0 and n_tail > 0, (cap, n_unweighted, waves)
    _sweep_sketches(monkeypatch, fa, p, exp, check=check)


@pytest.mark.parametrize("H", [16, 512])
def test_weighted_sketches_on_small_grids(H, monkeypatch):
    """30 reads with tandem repeats (60 weighted strands) among 520 weight-1 reads.  The weighted launch takes a WORKGROUP per strand where
    4 x 60 <= its workgroups (split: only at cap 32 with 8 per CU) and a wave per strand elsewhere; where 60 strands outnumber its
    4 x cap x per-CU waves, waves take several weighted strands."""
    rnd = random.Random(4224)
    seqs = []
    for i in range(30):
        unit = _rand_seq(rnd, 30 + i)
        body = _rand_seq(rnd, (900, 2100, 4300)[i % 3])
        seqs.append(body[:400] + unit * (2 + i % 7) + body[400:])
    seqs += _w1_reads(rnd, [(300, 1200, 2100, 2600)[i % 4] for i in range(520)])
    fa = FastaData.from_strings(seqs)
    p = MhapParams(num_hashes=H, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p)
    n_weighted, n_unweighted = 60, 2 * 520
    split_seen, reuse_seen = set(), set()

    def check(cap, wgs):
        assert len(fa) > 4 * WEIGHT_WG_PER_CU * cap
        assert n_unweighted > MINHASH_WAVES_PER_CU * cap          # weight-1 launch: n_whole > 0
        blocks = cap * wgs                                         # MHAP_MINHASH_WGS_PER_CU fixes the workgroups per CU
        if 4 * n_weighted <= blocks:
            split_seen.add((cap, wgs))
        elif n_weighted > 4 * blocks:
            reuse_seen.add((cap, wgs))
    _sweep_sketches(monkeypatch, fa, p, exp, check=check)
    assert split_seen == {(32, 8)}, split_seen
    assert {(1, 1), (2, 1), (3, 1), (7, 1), (1, 8)} <= reuse_seen, reuse_seen


def test_filtered_sketches_on_small_grids(monkeypatch):
    """A -f run (tf-idf weights): every strand is weighted and is an item of its own in the weight kernel; 1 040 strands in the weighted
    MinHash launch, more than its 32 x cap waves at every cap."""
    rnd = random.Random(5335)
    rep = _rand_seq(rnd, 300)
    seqs = []
    for i in range(520):
        s = _rand_seq(rnd, (700, 1300, 2200)[i % 3])
        seqs.append(s[:200] + rep + s[200:] if i % 3 == 0 else s)
    counts = {}
    for s in seqs:
        for i in range(len(s) - 15):
            counts[s[i:i + 16]] = counts.get(s[i:i + 16], 0) + 1
    total = sum(counts.values())
    top = sorted(counts.items(), key=lambda kv: -kv[1])[:300]
    fracs = np.array([c / total for _, c in top])
    hashes = np.array([int(O.kmer_hashes64(k, 16, True)[0]) for k, _ in top], dtype=np.int64)
    flt = mhap_amd.FrequencyCounts(hashes, fracs, 1e-5, 0.9, 3.0, False)
    oflt = O.Filter(hashes, fracs, 1e-5, 0.9, 3.0, False)
    fa = FastaData.from_strings(seqs)
    p = MhapParams(num_hashes=512, ordered_sketch_size=300, min_olap_length=0)
    exp = _expected_sketches(fa, p, oflt)
    n_strands = 2 * len(fa)

    def check(cap, wgs):
        assert n_strands > 4 * WEIGHT_WG_PER_CU * cap
        assert n_strands > MINHASH_WAVES_PER_CU * cap and 4 * n_strands > 8 * cap   # more strands than waves; no split
    _sweep_sketches(monkeypatch, fa, p, exp, flt=flt, check=check)


def _shared_repeat_corpus():
    """Reads of a genome with interspersed copies of one unit (test_gpu_parity.test_overlap_join_groups_and_lane_fallback's shape):
    duplicated ordered-k-mer hashes, identical reads and low-complexity reads send pairs to the slow (per-lane) kernel."""
    rnd = random.Random(6446)

    def mutate(s, rate):
        out = []
        for ch in s:
            r = rnd.random()
            if r < rate / 3:
                continue
            if r < 2 * rate / 3:
                out.append(rnd.choice("ACGT"))
                continue
            out.append(ch)
            if r < rate:
                out.append(rnd.choice("ACGT"))
        return "".join(out)
    unit = _rand_seq(rnd, 30)
    parts = []
    for _ in range(40):
        parts.append(mutate(unit, 0.01))
        parts.append(_rand_seq(rnd, rnd.randrange(400, 900)))
    genome = "".join(parts)
    seqs = []
    for _ in range(300):
        L = rnd.randrange(1500, 3500)
        o = rnd.randrange(0, len(genome) - L)
        s = mutate(genome[o:o + L], rnd.choice([0.03, 0.05, 0.07]))
        seqs.append(O.rc(s) if rnd.random() < 0.5 else s)
    seqs += [genome[1000:4000]] * 3
    seqs += [("ACGTTGCA" * 300)[i:i + 2200] for i in range(4)] + ["ACGGT" * 500, "A" * 1800, "A" * 2100]
    return FastaData.from_strings(seqs)


def _self_run(p, fa):
    with MinHashSearch(p) as ms:
        ms.add_data(fa)
        lines = sorted(mhap_amd.records_to_lines(ms.find_matches()))
        return lines, ms.stats()


@pytest.mark.parametrize("corpus", ["repeat", "err0.00", "err0.01"])
def test_self_records_on_small_grids(corpus, monkeypatch):
    """Whole self runs (sketch, index, join kernel, slow pairs) against the oracle's records (J/impl/MinHashSearch.java:150-251) at every
    cap.  The shared repeat sends pairs to the slow kernel; error-free and 1 % reads take the join kernel's wide passes."""
    if corpus == "repeat":
        fa = _shared_repeat_corpus()
        p = MhapParams(num_hashes=128, ordered_sketch_size=600)
        want = O.run_self(fa, H=128, S=600, nthreads=16)
    else:
        fa = mhap_amd.synth_reads(260, 5000, seed=911, error_rate=float(corpus[3:]))
        p = MhapParams()
        want = O.run_self(fa, nthreads=16)
    want_lines = O.record_lines(want["records"])
    assert len(want_lines) > 500
    monkeypatch.setenv("MHAP_MINHASH_WGS_PER_CU", "1")
    for cap in CAPS:
        monkeypatch.setenv("MHAP_NUM_CUS", str(cap))
        got, st = _self_run(p, fa)
        assert got == want_lines, (corpus, cap, len(got), len(want_lines))
        assert st["candidates_compared"] == want["compared"], (corpus, cap)
        if corpus == "repeat":
            assert st["slow_pairs"] > 0, (cap, st)
        if cap <= 3:
            # join kernel: more candidates than 32 c waves take in one pull of 8 each
            assert st["candidates_compared"] > JOIN_WAVES_PER_CU * JOIN_CHUNK * cap, (corpus, cap, st)
        assert len(fa) > 4 * WEIGHT_WG_PER_CU * cap                # weight kernel: >= 4 reads per workgroup


def _query_expectation(index, queries, H, S):
    """-s index -q queries (toSelf = false), brute force from the oracle's primitives (as test_gpu_parity.test_index_vs_stream_mode)."""
    def sketches(fa, both):
        out = []
        for i in range(len(fa)):
            s = fa.sequence(i)
            for fwd, t in (((1, s), (0, O.rc(s))) if both else ((1, s),)):
                _, od, olen = O.ordered(t, 12, S)
                out.append((int(fa.ids[i]), fwd, len(s), O.minhash(t, 16, H)[1], od, olen))
        return out
    ent, qs = sketches(index, True), sketches(queries, False)
    want = []
    for qid, _, qlen, qmh, qo, qolen in qs:
        for mid, fwd, L, mh, mo, molen in ent:
            if int((qmh == mh).sum()) < 3:
                continue
            r = O.overlap(qo, qolen, mo, molen)
            if r["score"] >= 0.78:
                b1, b2 = (r["b1"], r["b2"]) if fwd else (L - r["b2"] - 1, L - r["b1"] - 1)
                want.append(O.format_record({"from_id": qid, "to_id": mid, "score": r["score"], "raw": r["raw"], "a1": r["a1"], "a2": r["a2"],
                                             "alen": qlen, "b1": b1, "b2": b2, "blen": L, "to_rc": 0 if fwd else 1}))
    return sorted(want)


def test_query_records_on_small_grids(monkeypatch):
    """-q mode (find_matches_stream) on the shared-repeat reads: 200 indexed reads, 113 queries, against the oracle's brute force."""
    fa = _shared_repeat_corpus()
    index = fa.subset(np.arange(0, 200))
    index.ids[:] = np.arange(1, 201)
    queries = fa.subset(np.arange(200, len(fa)))
    queries.ids[:] = np.arange(201, 201 + len(queries))
    H, S = 128, 600
    want = _query_expectation(index, queries, H, S)
    assert len(want) > 200
    p = MhapParams(num_hashes=H, ordered_sketch_size=S)
    for cap in (1, 3, 32):
        monkeypatch.setenv("MHAP_NUM_CUS", str(cap))
        with MinHashSearch(p) as ms:
            ms.add_data(index)
            got = sorted(mhap_amd.records_to_lines(ms.find_matches_stream(queries)))
            st = ms.stats()
        assert got == want, (cap, len(got), len(want))
        assert len(index) > 4 * WEIGHT_WG_PER_CU * cap or cap == 32
        if cap <= 3:
            assert st["candidates_compared"] > JOIN_WAVES_PER_CU * cap, (cap, st)   # more candidates than resident join waves


# ---- aligner ----------------------------------------------------------------------------------------------------------------
def _mutate_bytes(rng, s, div):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < div / 3:
            continue
        if u < 2 * div / 3:
            out.append(c)
            out.append(int(rng.choice(list(b"ACGT"))))
            continue
        out.append(int(rng.choice(list(b"ACGT"))) if u < div else c)
    return bytes(out)


def _align_segments():
    """test_align_gpu's random divergent pairs and strip / pass boundary pairs, plus short pairs for the one-wave kernel, in one batch."""
    segs = []
    rng = np.random.default_rng(1)
    for k in range(14):
        n = int(rng.integers(0, 3001)) if k > 1 else k * 5
        s = bytes(rng.choice(list(b"ACGT"), n).tolist())
        t = _mutate_bytes(rng, s[int(rng.integers(0, max(1, n // 4))):], rng.uniform(0, 0.2))
        rc = int(rng.integers(0, 2))
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc))
    R8, ONE_WAVE, PASS = 8, 64 * 8, ALIGN_PASS_ROWS
    for m in (R8 - 1, R8, R8 + 1, ONE_WAVE - 1, ONE_WAVE, ONE_WAVE + 1, PASS - 1, PASS, PASS + 1, 2 * PASS - 1, 2 * PASS, 2 * PASS + 1, 3 * PASS + 5):
        rng = np.random.default_rng(m)
        g = bytes(rng.choice(list(b"ACGT"), m + 400).tolist())
        s1 = g[:m]
        s2 = _mutate_bytes(rng, g[max(0, m - 250):m + 150], 0.1)
        s3 = _mutate_bytes(rng, g[:300], 0.1)
        segs += [(s1, s2, 0), (s1, s3, 0), (s2, s1, 0)]
    rng = np.random.default_rng(99)
    for _ in range(30):
        m = int(rng.integers(20, 500))
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        segs.append((s, _mutate_bytes(rng, s, 0.1), int(rng.integers(0, 2))))
    return segs


def test_aligner_on_small_grids(monkeypatch):
    segs = _align_segments()
    bases, rows, off = bytearray(), [], 0
    for s1, s2, rc in segs:
        bases += s1 + s2
        rows.append((off, len(s1), off + len(s1), len(s2), rc))
        off += len(s1) + len(s2)
    bases = np.frombuffer(bytes(bases), np.uint8)
    pairs = np.array(rows, np.int64)
    want = align_ref.align_pairs(bases, pairs)
    m = pairs[:, 1]
    n_big = int(((m + 7) // 8 > 64).sum())                  # s1 beyond one wave's lanes: the four-wave kernel
    n_small = len(pairs) - n_big
    n_hbm = int((m > ALIGN_PASS_ROWS).sum())                # several passes: rows in HBM between them
    assert n_hbm >= 5
    for cap in (1, 3):
        assert n_big > ALIGN_BIG_PER_CU * cap and n_small > ALIGN_SMALL_PER_CU * cap, (cap, n_big, n_small)
        assert len(pairs) > 8 * cap
        monkeypatch.setenv("MHAP_NUM_CUS", str(cap))
        got = mhap_amd.align_pairs(bases, pairs)
        bad = [q for q in range(len(pairs)) if got[q].tolist() != want[q].tolist()]
        assert not bad, (cap, [(q, pairs[q].tolist(), got[q].tolist(), want[q].tolist()) for q in bad[:4]])


# ---- k-mer statistics ---------------------------------------------------------------------------------------------------------
def _ksim_pairs(k, rng):
    """test_ksim_gpu's crafted pairs plus short related pairs (LDS path) and long ones beyond the LDS scratch (HBM path)."""
    from test_ksim_gpu import _crafted, _mutate, _rand
    pairs = _crafted(k, rng)
    for _ in range(10):
        a = _rand(rng, rng.randrange(k, 900))
        pairs.append((a, _mutate(rng, a, 0.07)))
    for n in (14000, 15000, 17000, 20000, 14500, 16000, 18000, 21000):
        a = _rand(rng, n)
        pairs.append((a, _mutate(rng, a, 0.08)))
    return pairs


@pytest.mark.parametrize("k", [12, 16, 33])
def test_pair_kmer_stats_on_small_grids(k, monkeypatch):
    rng = random.Random(700 + k)
    pairs = _ksim_pairs(k, rng)
    want = [R.pair_stats(a, b, k) for a, b in pairs]
    bases, rows, off = [], [], 0
    for a, b in pairs:
        bases += [a, b]
        rows.append((off, len(a), off + len(a), len(b)))
        off += len(a) + len(b)
    buf = np.frombuffer("".join(bases).encode("latin-1"), dtype=np.uint8)
    rows = np.array(rows, dtype=np.int64)
    for cap in (1, 3):
        monkeypatch.setenv("MHAP_NUM_CUS", str(cap))
        got, taken = mhap_amd.pair_kmer_stats(buf, rows, k, paths=True)
        n_lds, n_hbm = int((taken == 1).sum()), int((taken == 2).sum())
        assert n_lds > KSIM_LDS_PER_CU * cap and n_hbm > KSIM_HBM_PER_CU * cap, (k, cap, n_lds, n_hbm)
        bad = [q for q in range(len(pairs)) if tuple(got[q]) != want[q]]
        assert not bad, (k, cap, [(q, len(pairs[q][0]), len(pairs[q][1]), tuple(got[q]), want[q]) for q in bad[:4]])


def test_device_trials_chunk_invariance_at_one_cu(monkeypatch):
    """--rng device at cap 1: 37 trials = 74 pairs on at most 4 LDS workgroups; chunks of 1 and 7 and the full grid give the same output."""
    rng = random.Random(1)
    recs = ["".join(rng.choice("ACGT") for _ in range(9000)), "".join(random.Random(2).choice("ACGT") for _ in range(2500))]
    args = (37, 16, 500, 150, 0.1, 0.03, 0.02)
    kw = dict(reference=recs, rng="device", seed=5, return_reads=True)
    full = K.simulate_pairs(*args, **kw)
    monkeypatch.setenv("MHAP_NUM_CUS", "1")
    assert 2 * args[0] > KSIM_LDS_PER_CU * 1
    for chunk in (None, 1, 7):
        got = K.simulate_pairs(*args, chunk=chunk, **kw)
        for a, b in zip(full, got):
            assert np.array_equal(a, b, equal_nan=True), chunk
