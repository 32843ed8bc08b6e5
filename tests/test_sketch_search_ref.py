"""The expected-records helper of the crafted second-stage tests (tests/sketch_search_ref.py) against the oracle's whole self search
(orc_run_self): what makes its expectations trustworthy.  CPU only."""
import numpy as np
import pytest

import oracle_lib as O
import sketch_search_ref as R
from mhap_amd import FastaData

K, K2 = 16, 12


def _reads(n=200, seed=7):
    """Reads of a 30 kb genome, both strands, 0-12 % substitutions; short ones (some below min_olap_length 116, some shorter
    than a k-mer) and ones with runs of N."""
    rng = np.random.default_rng(seed)
    genome = rng.choice(list("ACGT"), size=30000)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    seqs = []
    for i in range(n):
        L = int(rng.choice([8, 60, 130, 400, 1500, 2500, 4000])) if i % 10 == 0 else int(rng.integers(800, 4500))
        s = int(rng.integers(0, len(genome) - L))
        r = genome[s:s + L].copy()
        err = [0.0, 0.01, 0.03, 0.12][i % 4]
        flip = rng.random(L) < err
        r[flip] = rng.choice(list("ACGT"), size=int(flip.sum()))
        if i % 7 == 3 and L > 200:
            a = int(rng.integers(0, L - 50)); r[a:a + int(rng.integers(1, 40))] = "N"
        seq = "".join(r)
        if i % 2:
            seq = "".join(comp.get(c, c) for c in reversed(seq))
        seqs.append(seq)
    return FastaData.from_strings(seqs)


def _tables(fa, H, S):
    """Both strands sketched by the oracle, as orc_run_self keeps them (a read whose forward strand fails is dropped; a failing
    reverse strand alone is dropped too)."""
    b = R.TableBuilder(S, H, K2)
    for i in range(len(fa)):
        seq = fa.sequence(i)
        if len(seq) < 116:
            continue
        for fwd, s in ((True, seq), (False, O.rc(seq))):
            rc1, mh = O.minhash(s, K, H)
            rc2, od, seqlen = O.ordered(s, K2, S)
            if rc1 or rc2:
                break
            b.add(int(fa.ids[i]), od[:, 0], od[:, 1], seqlen, mh, fwd=fwd)
            assert b.rows[-1][2] == len(s)   # seq_length = ordered_seqlen + k2 - 1 = the read length
    return b.table()


@pytest.mark.parametrize("H,S,threshold,min_store_length,num_min_matches", [
    (64, 128, 0.78, 0, 3),
    (128, 512, 0.0, 2000, 1),
    (32, 1536, 0.0, 0, 3),
    (256, 300, 0.78, 2000, 1),
    (16, 64, 0.0, 0, 1),
])
def test_expected_records_match_the_oracle_self_search(H, S, threshold, min_store_length, num_min_matches):
    fa = _reads()
    kw = dict(k2=K2, num_min_matches=num_min_matches, min_store_length=min_store_length, threshold=threshold, max_shift=0.2)
    want = O.run_self(fa, k=K, H=H, S=S, nthreads=8, **kw)
    t = _tables(fa, H, S)
    assert len(t["ids"]) == want["strands"]
    got, compared = R.expected_records(t, H=H, return_compared=True, **kw)
    assert compared == want["compared"] and compared > 50
    assert got == O.record_lines(want["records"]) and len(got) > 20, (len(got), len(want["records"]))


def test_expected_records_query_mode():
    """-q mode: toSelf false, so a read also meets itself and larger ids; only "never short to short" applies.  The forward rows
    as queries give exactly the self search's pairs plus these."""
    fa = _reads(120, seed=11)
    H, S = 64, 256
    kw = dict(k2=K2, num_min_matches=3, min_store_length=2000, threshold=0.0, max_shift=0.2)
    t = _tables(fa, H, S)
    fw = np.nonzero(t["is_fwd"])[0]
    q = {k: v[fw] for k, v in t.items()}
    pairs = R.expected_pairs(t, q, num_min_matches=3, min_store_length=2000)
    self_pairs = R.expected_pairs(t, num_min_matches=3, min_store_length=2000)
    qset = {(int(fw[a]), b) for a, b in pairs}
    assert set(self_pairs) < qset
    assert any(t["ids"][a] == t["ids"][b] for a, b in qset)   # the read against its own strands
    for a, b in qset:
        assert t["seq_length"][a] >= 2000 or t["seq_length"][b] >= 2000
    lines = R.expected_records(t, q, H=H, **kw)
    assert len(lines) == len(pairs)                # threshold 0: every compared pair is a record


def test_known_candidate_pairs_give_the_scan_s_records():
    """expected_records(pairs=...): the candidate pairs given by a caller who built the tables (every ordered pair of rows that share
    num_min_matches slots, self pairs and both directions included) pass the same filters and give the same records and count as the
    all-pairs scan, in self mode and in -q mode."""
    fa = _reads(120, seed=13)
    H, S = 64, 256
    kw = dict(H=H, k2=K2, num_min_matches=3, min_store_length=2000, threshold=0.0, max_shift=0.2)
    t = _tables(fa, H, S)
    mh = t["minhash"]
    shared = (mh[:, None, :] == mh[None, :, :]).sum(axis=2) >= 3
    fw = np.nonzero(t["is_fwd"])[0]
    self_cand = [(int(a), int(b)) for a, b in zip(*np.nonzero(shared)) if t["is_fwd"][a]]
    want, compared = R.expected_records(t, return_compared=True, **kw)
    got, got_compared = R.expected_records(t, return_compared=True, pairs=self_cand, **kw)
    assert got == want and got_compared == compared and compared > 50
    q = {k: v[fw] for k, v in t.items()}
    q_cand = [(int(a), int(b)) for a, b in zip(*np.nonzero(shared[fw]))]
    assert R.expected_records(t, q, pairs=q_cand, **kw) == R.expected_records(t, q, **kw)
    with pytest.raises(AssertionError):
        R.expected_records(t, pairs=[(int(np.nonzero(t["is_fwd"] == 0)[0][0]), 0)], **kw)


def test_row_builder_refuses_rows_a_dat_cannot_hold():
    b = R.TableBuilder(S=8, H=4)
    mh = [1, 2, 3, 4]
    b.add(1, [5, -3, 9], [0, 2, 1], 3, mh)                                # sorted on the way in
    with pytest.raises(AssertionError, match="duplicated position"):
        b.add(2, [5, -3, 9], [0, 0, 1], 3, mh)
    with pytest.raises(AssertionError, match="outside"):
        b.add(3, [5, -3, 9], [0, 1, 3], 3, mh)
    with pytest.raises(AssertionError, match="ordered size"):
        b.add(4, [5, -3], [0, 1], 3, mh)                                  # size must be min(S, seqlen)
    with pytest.raises(AssertionError, match="ordered size"):
        b.add(5, list(range(9)), list(range(9)), 20, mh)                  # more than S
    with pytest.raises(AssertionError, match="outside int32"):
        b.add(6, [1 << 31, 0], [0, 1], 2, mh)
    with pytest.raises(AssertionError, match="not sorted"):
        R.check_row([[3, 0], [1, 1]], 2, 8)
    with pytest.raises(AssertionError, match="not sorted"):
        R.check_row([[1, 1], [1, 0]], 2, 8)                               # equal hashes: by position
    R.check_row([[R.INT32_MIN, 1], [-1, 0], [0, 2], [R.INT32_MAX, 3]], 4, 8)
    t = b.table()
    assert t["seq_length"].tolist() == [3 + 12 - 1] and t["ordered"][0, :3].tolist() == [[-3, 2], [5, 0], [9, 1]]
