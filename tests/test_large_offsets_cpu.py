"""What tests/test_large_offsets_gpu.py stands on, without a GPU: the placement helper puts the index marks where it says, the
shift argument of the longest read holds against the restatements on whole reads, and a filler's expected result is what the
restatements give a read without records."""
import numpy as np
import pytest

import consensus_ref as cref
import large_offsets as lo
import repeat_ref
import trim_cases as tc
import trim_ref


# ---- the placement helper -----------------------------------------------------------------------------------------------------------------

def _naive_starts(lengths, element):
    """The documented layouts once more, written apart from the helper: Python integers only."""
    starts, at = [], 0
    for n in lengths:
        starts.append(at)
        if element == "slot":
            at += n + 1
            at += (-at) % 4
        elif element == "word":
            at += 12 * n
        else:
            at += n
    return starts, at


SIZES = {"slot": (lo.pile_slots, lo.pile_used), "word": (lo.vote_words, lo.vote_words), "byte": (lo.base_bytes, lo.base_bytes)}


@pytest.mark.parametrize("element", list(SIZES))
def test_placement_puts_every_mark_inside_its_test_read(element):
    size_of, used_of = SIZES[element]
    rng = np.random.default_rng(5)
    for _ in range(60):
        n = int(rng.integers(3, 12))
        test_lengths = rng.integers(600, 9000, n).tolist()
        which = sorted(rng.choice(n, 3, replace=False).tolist())
        filler_max = int(rng.choice([1 << 22, 1 << 26, (1 << 28) - 3, 1 << 28]))
        fraction = float(rng.choice([0.5, 0.3, 0.8]))
        lay = lo.place(test_lengths, dict(zip(lo.MARKS, which)), size_of, filler_max, fraction)
        starts, total = _naive_starts(lay.lengths, element)
        assert starts == lay.starts and total == lay.total and total > lo.M32
        assert all(isinstance(s, int) for s in starts)                      # no 64-bit numpy integer decides a place
        assert [lay.lengths[i] for i in lay.test] == test_lengths            # the test reads, in order, each once
        assert all(1 <= lay.lengths[i] <= filler_max for i in lay.fillers) and len(lay.fillers) >= 3
        assert not lay.filler[0] or which[0] == 0
        found = lay.marks_inside_test_reads(lo.MARKS, used_of, 100)
        for mark, k in zip(lo.MARKS, which):
            i = lay.test[k]
            assert found[mark][0] == k
            assert starts[i] + 100 <= mark < starts[i] + used_of(lay.lengths[i]) - 100
            assert abs((mark - starts[i]) - fraction * size_of(lay.lengths[i])) <= 16
        if element == "word":                                                 # the plane a mark falls into, as the GPU case counts it
            for mark in lo.MARKS:
                k, o = found[mark]
                assert 0 <= o // test_lengths[k] < 12 and 12 * test_lengths[k] > o


def test_placement_refuses_a_mark_that_no_test_read_holds():
    lay = lo.place([5000, 5000, 5000], {lo.M30: 0, lo.M31: 1, lo.M32: 2}, lo.pile_slots, 1 << 28)
    lay.marks_inside_test_reads(lo.MARKS, lo.pile_used, 100)
    with pytest.raises(AssertionError):
        lay.marks_inside_test_reads([lo.M31 + 40000], lo.pile_used, 100)      # inside a filler
    with pytest.raises(AssertionError):
        lay.marks_inside_test_reads([lay.starts[lay.test[1]] + 50], lo.pile_used, 100)   # too near the read's first slot
    short = lo.place([5000, 5000], {lo.M30: 0, lo.M31: 1}, lo.pile_slots, 1 << 28)
    with pytest.raises(AssertionError):
        short.marks_inside_test_reads([lo.M32], lo.pile_used, 100)             # behind the table's end


# ---- the shift argument of the longest read ---------------------------------------------------------------------------------------------------

W = 3000
TRIM_PS = (trim_ref.params(min_cov=2, end_clip=3, min_span=10, min_identity=0.5), trim_ref.params(min_cov=3, end_clip=0, min_span=1))
REPEAT_PS = (repeat_ref.params(max_cov=1, min_run=20, min_unique=10, min_identity=0.5), repeat_ref.params(factor_pct=150, min_run=5, min_unique=0))


def _draw(rng, kind):
    """Runs [(window, begin, end, depth)] of one draw."""
    runs = []
    for wid in (lo.A_ID, lo.B_ID):
        for _ in range(int(rng.integers(0, 4))):
            n = int(rng.integers(20, 900))
            s = int(rng.integers(0, W - n + 1))
            runs.append((wid, s, s + n, int(rng.integers(1, 5))))
    if kind == "equal runs":          # the same length in both windows: the first wins
        n = int(rng.integers(100, 1000))
        sa, sb = (int(x) for x in rng.integers(0, W - n + 1, 2))
        runs = [(lo.A_ID, sa, sa + n, 3), (lo.B_ID, sb, sb + n, 3)]
    elif kind == "edges":             # runs that touch the ends of the windows that face the empty middle, and the read's own ends
        runs += [(lo.A_ID, W - int(rng.integers(30, 500)), W, 3), (lo.B_ID, 0, int(rng.integers(30, 500)), 3)]
        if rng.integers(0, 2):
            runs += [(lo.A_ID, 0, 50, 3), (lo.B_ID, W - 50, W, 3)]
    elif kind == "one window":
        runs = [r for r in runs if r[0] == lo.B_ID]
    return runs


def _cases():
    rng = np.random.default_rng(23)
    for k in range(320):
        kind = ("random", "equal runs", "edges", "one window")[k % 4]
        long_len = int(rng.integers(2 * W + 1, 60000))
        partner_len = int(rng.integers(50, 2000))
        folded = tc.recs(lo.window_records(rng, W, partner_len, _draw(rng, kind), tc.rec, noise=int(rng.integers(0, 6))))
        yield kind, long_len, partner_len, folded


def test_two_windows_put_together_equal_the_whole_read():
    seen = dict(ties=0, edge_runs=0, deleted=0, gapped=0, intervals=0, edge_intervals=0, b_first=0)
    for kind, long_len, partner_len, folded in _cases():
        real = lo.unfold(folded, long_len, W)
        assert ((real["from_id"] != lo.B_ID) & (real["to_id"] != lo.B_ID)).all()
        ids, lengths = [lo.A_ID, lo.P_ID], [long_len, partner_len]
        for P in TRIM_PS:
            rows, flags, counts, cov = trim_ref.trim(ids, lengths, real, P)
            assert not cov[0][W:long_len - W].any()                            # the premise: nothing between the windows
            erows, eflags, ecounts = lo.trim_unfolded(folded, long_len, W, partner_len, P)
            assert rows.tolist() == erows.tolist() and flags.tolist() == eflags.tolist() and counts == ecounts, (kind, rows, erows)
            runs = trim_ref.runs_of(cov[0], P["min_cov"])
            best = max((e - s for s, e in runs), default=0)
            seen["ties"] += sum(1 for s, e in runs if e - s == best) > 1
            seen["edge_runs"] += any(e == W or s == long_len - W for s, e in runs)
            seen["deleted"] += bool(flags[0] & trim_ref.DELETED)
            seen["gapped"] += bool(flags[0] & trim_ref.GAPPED)
            seen["b_first"] += bool(runs) and rows[0, 0] >= long_len - W - P["end_clip"]
        for P in REPEAT_PS:
            m = repeat_ref.mark(ids, lengths, real, P)
            e = lo.repeat_unfolded(folded, long_len, W, partner_len, P)
            for key in ("rows", "flags", "offsets", "intervals", "hist"):
                assert m[key].tolist() == e[key].tolist(), (kind, key)
            assert m["counts"] == e["counts"]
            seen["intervals"] += len(m["intervals"]) > 0
            seen["edge_intervals"] += any(b == W or a == long_len - W for a, b in m["intervals"][:m["offsets"][1]].tolist())
    assert min(seen.values()) >= 10, seen


# ---- a filler's expected result ------------------------------------------------------------------------------------------------------------------

def test_a_read_without_records_is_what_the_filler_expectations_say():
    ids, lengths = [7, 8, 9], [40, 300, 25]
    records = tc.recs([tc.rec(7, 9, 5, 30, 40, 0, 20, 25), tc.rec(9, 7, 2, 22, 25, 10, 35, 40)])     # none names read 8
    P = trim_ref.params(min_cov=1, end_clip=0, min_span=1)
    rows, flags, counts, _ = trim_ref.trim(ids, lengths, records, P)
    lay = lo.Layout(lengths, [False, True, False], lo.pile_slots)
    small = trim_ref.trim([7, 9], [40, 25], records, P)
    erows, eflags, ecounts = lo.trim_with_fillers(lay, *small[:3])
    assert rows[1].tolist() == [0, 0, 0, 0] and flags[1] == trim_ref.DELETED
    assert rows.tolist() == erows.tolist() and flags.tolist() == eflags.tolist() and counts == ecounts

    RP = repeat_ref.params(max_cov=1, min_run=3, min_unique=1)
    m = repeat_ref.mark(ids, lengths, np.concatenate([records, records]), RP)
    e = lo.repeat_with_fillers(lay, repeat_ref.mark([7, 9], [40, 25], np.concatenate([records, records]), RP))
    assert m["rows"][1].tolist() == [0, 0, 0, -1] and m["flags"][1] == 0 and m["offsets"][1] == m["offsets"][2]
    assert m["counts"]["intervals"] > 0
    for key in ("rows", "flags", "offsets", "intervals", "hist"):
        assert m[key].tolist() == e[key].tolist(), key
    assert m["counts"] == e["counts"]

    reads = [b"ACGTACGTAC", b"GATTACANNACGT", b"ACGTACGTAC"]
    c = cref.Consensus(reads, [1, 2, 3])
    rec = cref.records_from_results([1], [3], [10], [10], [0], [[20, 0, 9, 0, 9, 10, 0]])
    c.add(rec, [0, 1], np.array([10 << 4 | 7], np.uint32))
    for min_cov in (1, 4):
        seqs, stats = c.call(min_cov)
        want_seq, want_stats = lo.correct_filler(reads[1])
        assert seqs[1] == want_seq and stats[1].tolist() == want_stats
    assert not c.votes[1].any() and c.votes[0].any()
