"""mhap_correct_add_views on the GPU against the CPU restatement (tests/consensus_ref.py) given only the selected views: the raw
counters of every read, the corrected bytes, the six counts and skipped_views, exactly — for no view bytes at all, every view, view
A only, view B only, none and a random mix, on the seventy-overlap pile and the quality workload; a cleared view takes no place under
the 65 535-view cap; then `mhap-hip --realign --correct --best-overlaps` end to end against the run without the flag and against
`python -m mhap_amd.correct --best-overlaps`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import consensus_ref as cref  # noqa: E402
from align_ref import rc_bytes  # noqa: E402
from test_correct_gpu import CLI, GOLD, OP_EQ, _align, _fasta, _mutate, _rand  # noqa: E402

pytestmark = pytest.mark.gpu


class SelectedConsensus(cref.Consensus):
    """The restatement with one byte per record that says which of its views vote: a view whose bit is clear is not added at all, so
    it takes no place under the cap and is not a skipped view.  views None: both."""

    def add_selected(self, records, op_offsets, ops, views, memo):
        for q in range(len(records)):
            rec = records[q]
            runs = tuple(int(x) for x in ops[int(op_offsets[q]):int(op_offsets[q + 1])])
            fid, tid = int(rec["from_id"]), int(rec["to_id"])
            if not runs or fid == tid:
                continue
            ia, ib = self.row[fid], self.row[tid]
            to_rc = int(rec["to_rc"]) != 0
            blen = len(self.reads[ib])
            i0 = int(rec["a1"])
            j0 = blen - int(rec["b2"]) - 1 if to_rc else int(rec["b1"])
            key = (ia, ib, i0, j0, to_rc, runs)
            if key not in memo:
                memo[key] = cref.views_of(self.reads[ia], rc_bytes(self.reads[ib]) if to_rc else self.reads[ib], i0, j0, runs, to_rc, blen)
            va, vb = memo[key]
            bits = 3 if views is None else int(views[q])
            if bits & 1:
                self.add_view(ia, va)      # arrival order: view A, then view B
            if bits & 2:
                self.add_view(ib, vb)


def _check_views(reads, recs, off, ops, views, memo, min_cov=4, splits=1):
    """The session given `views` (in `splits` adds) against the wrapper: (seqs, stats, skipped, votes)."""
    ref = SelectedConsensus(reads, range(1, len(reads) + 1))
    ref.add_selected(recs, off, ops, views, memo)
    from mhap_amd.correct import select_paths
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        for rows in np.array_split(np.arange(len(recs)), splits):
            po, pops = (off, ops) if splits == 1 else select_paths(off, ops, rows)
            cs.add(recs[rows], po, pops, views=None if views is None else views[rows])
        votes = [cs.votes(r) for r in range(len(reads))]
        seqs, stats, skipped = cs.finish(min_cov)
    wseqs, wstats = ref.call(min_cov)
    for r in range(len(reads)):
        bad = np.argwhere(votes[r].astype(np.int64) != ref.votes[r])
        assert len(bad) == 0, (r, bad[:5].tolist())
        assert seqs[r] == wseqs[r], r
    assert stats.tolist() == wstats.tolist() and skipped == ref.skipped_views
    return seqs, stats, skipped, votes


def _plain_add(reads, recs, off, ops):
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        cs.add(recs, off, ops)
        votes = [cs.votes(r) for r in range(len(reads))]
        return cs.finish(4) + (votes,)


def _modes(reads, recs, off, ops, seed):
    n = len(recs)
    memo = {}
    plain = _plain_add(reads, recs, off, ops)
    for views in (None, np.full(n, 3, np.uint8)):      # also what mhap_correct_add gives
        got = _check_views(reads, recs, off, ops, views, memo)
        assert got[0] == plain[0] and got[1].tolist() == plain[1].tolist() and got[2] == plain[2]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[3], plain[3]))
    froms, tos = set(recs["from_id"].tolist()), set(recs["to_id"].tolist())
    only_a = _check_views(reads, recs, off, ops, np.full(n, 1, np.uint8), memo)
    only_b = _check_views(reads, recs, off, ops, np.full(n, 2, np.uint8), memo, splits=3)
    for r in range(len(reads)):                        # a read that is only ever `to` gets nothing from view A, and the reverse
        if r + 1 not in froms:
            assert only_a[3][r].sum() == 0
        if r + 1 not in tos:
            assert only_b[3][r].sum() == 0
    assert sum(int(v.sum()) for v in only_a[3]) > 0 and sum(int(v.sum()) for v in only_b[3]) > 0
    for r in range(len(reads)):                        # votes are sums: A only plus B only is both
        assert (only_a[3][r].astype(np.int64) + only_b[3][r]).tolist() == plain[3][r].astype(np.int64).tolist()
    none = _check_views(reads, recs, off, ops, np.zeros(n, np.uint8), memo)
    assert none[0] == [bytes(r) for r in reads] and all(v.sum() == 0 for v in none[3])
    mix = np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)
    assert len(set(mix.tolist())) == 4
    _check_views(reads, recs, off, ops, mix, memo, splits=2)


def test_views_on_the_seventy_overlap_pile():
    rng = np.random.default_rng(13)
    target = _rand(rng, 300)
    reads, pairs = [target], []
    for k in range(70):      # the pile of test_correct_gpu's fixture
        rc = k % 2
        e = _mutate(rng, target[k % 7 * 5:300 - k % 5 * 9], 0.12)
        reads.append(rc_bytes(e) if rc else e)
        pairs.append((0, k + 1, rc, -(k % 7 * 5), 40) if k % 3 else (k + 1, 0, rc, k % 7 * 5, 40))
    pairs = [(x, y, rc, (len(reads[y]) - len(reads[x])) - d if (rc and y == 0) else d, b) for x, y, rc, d, b in pairs]
    recs, off, ops = _align(reads, pairs)
    assert (recs["score"] > 0.7).sum() >= 60
    _modes(reads, recs, off, ops, 1)


def test_views_on_the_quality_workload():
    reads, truths, bases, pairs, meta = cref.quality_workload(7)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    _modes(reads, recs, offsets, ops, 2)


def test_wrong_number_of_view_bytes_is_refused():
    reads = [b"ACGTACGTAC", b"ACGTACGTAC"]
    recs, off, ops = _align(reads, [(0, 1, 0, 0, 3)])
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        with pytest.raises(mhap_amd.MhapError, match="view bytes"):
            cs.add(recs, off, ops, views=np.zeros(2, np.uint8))
        none = np.zeros(0, mhap_amd.api.RECORD_DTYPE)
        cs.add(none, np.zeros(1, np.int64), np.zeros(0, np.uint32), views=np.zeros(0, np.uint8))     # an empty add with views
        assert cs.votes(0).sum() == 0


def test_a_cleared_view_takes_no_place_under_the_cap():
    """The 65 537 copies of test_the_cap_of_65535_views with view B cleared on every one: read 0 stops at 65 535 views and two are
    skipped; read 1 was never voted on, and nothing of it counts as skipped."""
    read = _rand(np.random.default_rng(14), 40)
    reads = [read, read, b"ACGT" * 10]
    rec, off, ops = _align(reads, [(0, 1, 0, 0, 5)])
    assert ops.tolist() == [40 << 4 | OP_EQ]
    n = 65537
    seqs, stats, skipped, votes = _check_views(reads, np.repeat(rec, n), np.arange(n + 1, dtype=np.int64), np.repeat(ops, n),
                                               np.full(n, 1, np.uint8), {})
    assert skipped == 2
    want = np.zeros((40, 24), np.int64)
    for t, c in enumerate(read):
        want[t, b"ACGT".index(c)] = 65535
    want[:39, 5] = 65535
    assert votes[0].astype(np.int64).tolist() == want.tolist()
    assert votes[1].sum() == 0 and votes[2].sum() == 0 and seqs == reads and stats[1].tolist() == [40, 40, 0, 0, 0, 40]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


def _counts(stderr):
    lines = [l for l in stderr.decode().split("\n") if l.startswith("Best overlaps: ")]
    assert len(lines) == 1, stderr[-2000:]
    m = re.fullmatch(r"Best overlaps: (\d+) reads, (\d+) with a view, (\d+) cut; (\d+) of (\d+) views kept; (\d+) eligible overlaps", lines[0])
    assert m, lines[0]
    return lines[0], [int(x) for x in m.groups()]


def test_driver_and_tool_with_best_overlaps(tmp_path):
    fasta = os.path.join(GOLD, "small_reads.fasta")
    fa = mhap_amd.FastaData.from_file(fasta)
    plain = _cli(["-s", fasta])
    out0, out1, out2, table = (tmp_path / n for n in ("all.fasta", "wide.fasta", "cut.fasta", "best.tsv"))
    base = _cli(["-s", fasta, "--realign", "--correct", str(out0)])
    assert plain.returncode == 0 and base.returncode == 0, base.stderr[-2000:]
    assert b"Best overlaps" not in base.stderr and b"--best" not in base.stderr
    # a best_n that no read exceeds and no minimum span: every view votes, and the corrected reads are those of the run without the flag
    wide = _cli(["-s", fasta, "--realign", "--correct", str(out1), "--best-overlaps", "1000000", "--best-min-span", "0"])
    assert wide.returncode == 0, wide.stderr[-2000:]
    _, c = _counts(wide.stderr)
    assert c[0] == len(fa) and c[2] == 0 and c[3] == c[4] == 2 * c[5] > 0
    assert out1.read_bytes() == out0.read_bytes()
    # a small best_n: reads are cut, and the driver's FASTA is the tool's on the driver's plain output
    cut = _cli(["-s", fasta, "--realign", "--correct", str(out2), "--best-overlaps", "2", "--best-min-span", "100", "--best-table", str(table)])
    assert cut.returncode == 0, cut.stderr[-2000:]
    line, c = _counts(cut.stderr)
    assert c[2] >= 1 and c[3] < c[4], line                                  # at least one read cut
    assert b"--best-overlaps = 2" in cut.stderr and b"--best-min-span = 100" in cut.stderr
    assert sorted(cut.stdout.split(b"\n")) == sorted(base.stdout.split(b"\n")) and len(cut.stdout) == len(base.stdout) > 1000
    rows = [l.split(" ") for l in table.read_text().split("\n") if l]
    assert [r[0] for r in rows] == [str(i) for i in fa.ids.tolist()] and all(len(r) == 4 for r in rows)
    assert [sum(int(r[k]) for r in rows) for k in (1, 2)] == [c[4], c[3]] and sum(int(r[1]) > 2 for r in rows) == c[2]
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tool_out = tmp_path / "tool.fasta"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.correct", str(tmp_path / "ovl.txt"), fasta, "--best-overlaps", "2", "--best-min-span", "100",
                        "-o", str(tool_out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert line in p.stderr
    assert tool_out.read_bytes() == out2.read_bytes()
    assert out2.read_bytes() != out0.read_bytes(), "the selection changes at least one corrected read of the fixture"
    # the selection tool on the same overlaps: the same counts and table, and only records with a kept view
    kept, ttable = tmp_path / "kept.txt", tmp_path / "tool.tsv"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.best_overlaps", str(tmp_path / "ovl.txt"), fasta, "-n", "2", "--min-span", "100",
                        "--table", str(ttable), "-o", str(kept)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert line in p.stderr and ttable.read_text() == table.read_text()
    assert 0 < len(kept.read_text().split("\n")) - 1 <= c[3]
    # without --correct the flag still selects: the counts line and the table
    table.unlink()
    alone = _cli(["-s", fasta, "--realign", "--best-overlaps", "2", "--best-min-span", "100", "--best-table", str(table)])
    assert alone.returncode == 0 and _counts(alone.stderr)[0] == line and table.read_text() == ttable.read_text()
