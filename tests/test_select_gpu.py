"""Overlap selection on the GPU (select_kernels.hip) against tests/select_ref.py, byte for byte: rows, counts and view bytes — at
every segment size round best_n, at best_n round the wave and workgroup sizes, with ties of every kind at the last place, with
segments whose keys differ in one byte only for each of the four passes of the radix select, at and past the LDS budget, past the
1 024-entry step of the prefix sum, under any order and split of the records — then the call sequence and the refusals.

Reads are given by lengths only, so long reads cost nothing: with score 1.0 a view's key is 1 + span, and any key up to 2^31 - 8
can be made.  A crafted record sits with a span of `key - 1` on its target read and with a span of 1 on the partner read, which
min_span = 2 keeps from being a view: the target's segment is exactly the keys asked for."""
import numpy as np
import pytest

import mhap_amd
from mhap_amd import api

import select_ref as ref
import trim_cases as tc

pytestmark = pytest.mark.gpu
PARTNER, PARTNER_LEN = 9_000_001, 10
BIG = 2 ** 31 - 9     # the longest read a table takes


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def views_on(read_id, read_len, keys):
    """Records that give read `read_id` one view of each of `keys` (>= 3) and the partner read none (under min_span = 2)."""
    keys = np.asarray(keys, np.int64)
    assert len(keys) == 0 or (keys.min() >= 3 and keys.max() - 1 <= read_len)
    r = np.zeros(len(keys), api.RECORD_DTYPE)
    r["from_id"], r["to_id"], r["score"], r["raw"] = read_id, PARTNER, 1.0, 50.0
    r["a1"], r["a2"], r["alen"] = 0, keys - 2, read_len
    r["b1"], r["b2"], r["blen"] = 0, 0, PARTNER_LEN
    return r


def table(lengths):
    """ids 1 .. n for the given lengths, and the partner read behind them."""
    ids = np.concatenate([np.arange(1, len(lengths) + 1, dtype=np.int64), [PARTNER]])
    return ids, np.concatenate([np.asarray(lengths, np.int32), [PARTNER_LEN]]).astype(np.int32)


def same(ss, m):
    assert ss.rows.dtype == np.int32 and ss.rows.tobytes() == m["rows"].tobytes(), (ss.rows[:8], m["rows"][:8])
    assert ss.counts == m["counts"]


def check(ms, ids, lengths, records, P, apply_to=None):
    m = ref.select(ids, lengths, records, P)
    with api.SelectSession(ids, lengths, handle=ms, **P) as ss:
        ss.add(records)
        ss.finish()
        same(ss, m)
        for recs in (records, apply_to):
            if recs is not None:
                views = ss.apply(recs)
                assert views.dtype == np.uint8 and views.tobytes() == ref.apply(ids, m["thr"], recs, P).tobytes()
    return m


def crafted(ms, segments, best_n, lengths=None):
    """One read per list of keys in `segments`; returns the restatement's result."""
    lengths = [max(1000, max(k, default=0)) for k in segments] if lengths is None else lengths
    ids, lens = table(lengths)
    records = np.concatenate([views_on(int(ids[r]), int(lens[r]), k) for r, k in enumerate(segments)] + [np.zeros(0, api.RECORD_DTYPE)])
    return check(ms, ids, lens, records, ref.params(best_n=best_n, min_span=2))


@pytest.mark.parametrize("best_n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_segment_sizes_round_best_n(ms, best_n):
    """0, 1, best_n - 1, best_n and best_n + 1 entries, distinct keys and keys with duplicates, and some larger segments."""
    rng = np.random.default_rng(best_n)
    sizes = sorted({0, 1, max(best_n - 1, 0), best_n, best_n + 1, best_n + 2, 2 * best_n + 1, 3 * best_n + 7, 1000})
    segments = [rng.permutation(np.arange(3, 3 + 4 * e, 4))[:e] for e in sizes]       # distinct
    segments += [rng.integers(3, 3 + max(e // 3, 1), e) for e in sizes]               # many duplicates
    m = crafted(ms, segments, best_n)
    assert m["rows"][:len(sizes), 0].tolist() == sizes
    for r, e in enumerate(sizes):     # distinct keys: exactly best_n kept when there are more
        assert m["rows"][r, 1] == min(e, best_n) and m["rows"][r, 2] == (1 if e <= best_n else 3 + 4 * (e - best_n))
    assert m["counts"]["reads_over"] == 2 * sum(e > best_n for e in sizes)


def test_best_n_above_every_segment(ms):
    m = crafted(ms, [[5, 9, 9, 700], [3] * 50, []], 10_000)
    assert m["rows"].tolist() == [[4, 4, 1, 700], [50, 50, 1, 3], [0, 0, 1, 0], [0, 0, 1, 0]] and m["counts"]["reads_over"] == 0


def test_ties_at_the_last_place(ms):
    n = 7
    segments = [[500] * 40,                                        # all equal: all kept
                [900, 800, 700, 600, 500, 400] + [300] * 9 + [200, 100],   # the tie group straddles the 7th place: 6 + 9 kept
                [900, 800, 700, 600, 500, 400, 300, 299, 298],     # the 7th and the 8th differ by 1
                [300] * 7 + [299] * 7,                             # the group ends exactly at the 7th place
                [2 ** 24 + 5] * 3 + [2 ** 24 + 4] * 30]            # equal down to the last byte
    m = crafted(ms, segments, n, lengths=[2 ** 25] * 5)
    assert m["rows"][:, :3].tolist() == [[40, 40, 500], [17, 15, 300], [9, 7, 300], [14, 7, 300], [33, 33, 2 ** 24 + 4], [0, 0, 1]]


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_keys_that_differ_in_one_byte_only(ms, byte):
    """The pass of that byte alone decides; byte 3 needs reads of about 2^30 and of 2^31 - 9 bases."""
    rng = np.random.default_rng(byte)
    top = 0x7E if byte == 3 else 0xFF
    base = 0x00_34_56_78 if byte == 3 else 0x12_34_56_78
    base &= ~(0xFF << (8 * byte))
    distinct = base | (rng.permutation(np.arange(1, top + 1)).astype(np.int64)[:100] << (8 * byte))
    dup = base | (rng.integers(1, top + 1, 400).astype(np.int64) << (8 * byte))
    lengths = [BIG, BIG, 2 ** 30 + 11]
    small = dup[dup < 2 ** 30][:150] if byte == 3 else dup[:150]
    m = crafted(ms, [distinct, dup, small], 37, lengths=lengths)
    assert m["rows"][0, 1] == 37 and m["rows"][1, 1] >= 37 and m["counts"]["reads_over"] == 3
    assert m["rows"][0, 2] == np.sort(distinct)[-37]


def test_greatest_keys_and_the_last_pass(ms):
    """Keys up to 2^31 - 8, and a segment whose deciding bin is reached only in the last pass: two of every key, so no pass but the
    last sees a bin with one key."""
    last = np.repeat(0x12_34_56_00 + np.arange(100, dtype=np.int64), 2)
    hi = np.array([BIG + 1, BIG, BIG - 1, BIG + 1, 2 ** 30, 3, 2 ** 24, BIG - 255, BIG - 256], np.int64)
    rng = np.random.default_rng(5)
    wide = rng.integers(3, BIG + 1, 3000)          # distinct in the first bytes: the search ends early
    m = crafted(ms, [last, hi, wide], 37, lengths=[BIG] * 3)
    assert m["rows"][0].tolist() == [200, 38, 0x12_34_56_00 + 81, 0x12_34_56_00 + 99]
    assert m["rows"][1, 3] == BIG + 1 == 2 ** 31 - 8
    m = crafted(ms, [hi], 2, lengths=[BIG])
    assert m["rows"][0].tolist() == [9, 2, BIG + 1, BIG + 1]


@pytest.mark.parametrize("entries", [api.SELECT_LDS_KEYS - 1, api.SELECT_LDS_KEYS, api.SELECT_LDS_KEYS + 1, 70_000])
def test_segments_against_the_lds_budget(ms, entries):
    """At the budget the segment stays in LDS, one past it every pass streams it; heavy duplicates and distinct keys."""
    rng = np.random.default_rng(entries)
    heavy = np.concatenate([rng.choice([0x01_00_00_07, 0x01_00_01_07, 0x01_02_00_07, 0x03_00_00_07, 77, 78, 0x00_01_00_00], entries - 2000),
                            rng.integers(3, 2 ** 26, 2000)])
    distinct = rng.permutation(np.arange(3, 3 + entries, dtype=np.int64) * 3)
    for best_n in (40, 5000):
        m = crafted(ms, [heavy, distinct, [5, 6]], best_n, lengths=[2 ** 27, 2 ** 27, 100])
        assert m["rows"][1].tolist() == [entries, best_n, 3 * (3 + entries - best_n), 3 * (2 + entries)]
        assert m["rows"][0, 1] >= best_n and m["counts"]["reads_over"] == 2


def test_many_reads_past_the_tile_of_the_prefix_sum(ms):
    """1 100 reads with entries among 2 100; reads over best_n on both sides of read 1 024 and of read 2 048."""
    rng = np.random.default_rng(21)
    n, best_n = 2100, 4
    over = [0, 1022, 1023, 1024, 1025, 2046, 2047, 2048, 2049, 2099]
    rest = rng.choice(np.setdiff1d(np.arange(n), over), 1100 - len(over), replace=False)
    segments = [[] for _ in range(n)]
    for r in over:
        segments[r] = rng.integers(3, 4000, best_n + 1 + int(rng.integers(0, 30)))
    for r in rest.tolist():
        segments[r] = rng.integers(3, 4000, int(rng.integers(1, best_n + 1)))
    m = crafted(ms, segments, best_n, lengths=[5000] * n)
    assert m["counts"]["reads_with_entry"] == 1100 and m["counts"]["reads_over"] == len(over)
    assert (m["rows"][over, 0] > best_n).all()


def general_case(seed=9, n_reads=30, n=4000):
    """Records with both views, random spans and the realignment's scores (1 - errors / columns), some ineligible."""
    rng = np.random.default_rng(seed)
    lengths = np.random.default_rng(1234).integers(600, 20000, n_reads).astype(np.int32)     # one table whatever the seed
    ids = np.arange(101, 101 + n_reads, dtype=np.int64)
    out = []
    for _ in range(n):
        x, y = rng.integers(0, n_reads, 2).tolist()       # (x == y now and then: a self overlap)
        la, lb = int(lengths[x]), int(lengths[y])
        sa, sb = int(rng.integers(1, la + 1)), int(rng.integers(1, lb + 1))
        a1, b1 = int(rng.integers(0, la - sa + 1)), int(rng.integers(0, lb - sb + 1))
        cols = max(sa, sb) + int(rng.integers(0, 40))
        score = float(rng.choice([0.0, float("nan"), 1.0, 1.5])) if rng.random() < 0.1 else 1.0 - int(rng.integers(0, cols // 2 + 1)) / cols
        out.append(tc.rec(int(ids[x]), int(ids[y]), a1, a1 + sa - 1, la, b1, b1 + sb - 1, lb, int(rng.integers(0, 2)), score))
    return ids, lengths, tc.recs(out)


def test_general_records_and_parameters(ms):
    ids, lengths, records = general_case()
    for kw in (dict(best_n=5), dict(best_n=40, min_span=0), dict(best_n=64, min_span=3000, min_identity=0.7), dict()):
        m = check(ms, ids, lengths, records, ref.params(**kw))
        assert 0 < m["counts"]["eligible_records"] < len(records) and m["counts"]["reads_over"] > 0


def test_order_split_and_call_sequence(ms):
    ids, lengths, records = general_case(seed=10)
    others = general_case(seed=11)[2]
    P = ref.params(best_n=6, min_span=200)
    m = ref.select(ids, lengths, records, P)
    half = len(records) // 2
    m_half = ref.select(ids, lengths, records[:half], P)
    want = ref.apply(ids, m["thr"], records, P).tobytes()
    with api.SelectSession(ids, lengths, handle=ms, **P) as ss:
        with pytest.raises(api.MhapError, match=r"no mhap_select_finish has completed.*code -4"):     # MHAP_E_STATE
            ss.apply(records[:3])
        ss.add(records[:half])
        ss.add(records[:0])                                     # an add of nothing
        ss.finish()
        same(ss, m_half)
        ss.finish()                                             # a repeated finish
        same(ss, m_half)
        assert ss.apply(records).tobytes() == ref.apply(ids, m_half["thr"], records, P).tobytes()     # half of them never added
        ss.add(records[half:])                                  # adds after a finish, then a finish
        ss.finish()
        same(ss, m)
        assert ss.apply(records).tobytes() == want
        assert ss.apply(others).tobytes() == ref.apply(ids, m["thr"], others, P).tobytes()            # records never added
        assert ss.apply(records[:0]).tobytes() == b""
    for order in ("seven adds", "reversed"):
        with api.SelectSession(ids, lengths, handle=ms, **P) as ss:
            if order == "reversed":
                ss.add(records[::-1])
            else:
                for part in np.array_split(np.arange(len(records)), 7):
                    ss.add(records[part])
            ss.finish()
            same(ss, m)
            assert ss.apply(records).tobytes() == want


def test_empty_tables_and_sessions(ms):
    none = np.zeros(0, api.RECORD_DTYPE)
    with api.SelectSession([], [], handle=ms) as ss:
        rows, counts = ss.finish()
        assert rows.shape == (0, 4) and counts == dict(zip(api.SELECT_COUNTS, [0] * 6))
    ids, lengths = table([100, 200])
    m = check(ms, ids, lengths, none, ref.params(), apply_to=views_on(1, 100, [50]))
    assert m["rows"].tolist() == [[0, 0, 1, 0]] * 3


def test_bad_parameters_and_tables_are_refused(ms):
    for kw in (dict(best_n=0), dict(min_span=-1)):
        with pytest.raises(api.MhapError, match="best_n must be >= 1 and min_span >= 0"):
            api.SelectSession([1], [10], handle=ms, **kw)
    with pytest.raises(api.MhapError, match="read 1 has a negative length"):
        api.SelectSession([1, 2], [10, -1], handle=ms)


def test_refused_adds_name_the_record_and_add_nothing(ms):
    ids, lengths, records = general_case(seed=12, n=300)
    P = ref.params(best_n=3)
    m = ref.select(ids, lengths, records, P)
    good = records[:5].copy()
    la = int(lengths[0])
    bad = {"names read 77, which is not among the reads": tc.rec(77, int(ids[1]), 0, 9, 50, 0, 9, int(lengths[1])),
           "the length": tc.rec(int(ids[0]), int(ids[1]), 0, 9, la + 1, 0, 9, int(lengths[1])),
           f"of read {int(ids[0])}, which has {la} bases": tc.rec(int(ids[0]), int(ids[1]), 5, la, la, 0, 9, int(lengths[1]))}
    with api.SelectSession(ids, lengths, handle=ms, **P) as ss:
        ss.add(records)
        ss.finish()
        same(ss, m)
        for word, rec in bad.items():
            batch = np.concatenate([good[:2], tc.recs([rec]), good[2:]])
            with pytest.raises(api.MhapError, match="mhap_select_add: record 2 .*" + word):
                ss.add(batch)
            with pytest.raises(api.MhapError, match="mhap_select_apply: record 2 "):
                ss.apply(batch)
            ss.finish()
            same(ss, m)                                         # counts and rows unchanged
