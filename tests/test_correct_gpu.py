"""Read correction on the GPU (mhap_correct_*, correct_kernels.hip) against its CPU restatement (tests/consensus_ref.py): the raw
counters of every read and the finished bytes, offsets and six counts, exactly; then `mhap-hip --realign --correct` against
`python -m mhap_amd.correct` end to end."""
import os
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

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8


def _fasta(reads):
    """A FastaData of the given byte strings (an empty one included), ids 1 .. n."""
    lengths = np.array([len(r) for r in reads], np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64) if len(reads) else np.zeros(0, np.int64)
    bases = np.frombuffer(b"".join(reads) or b"\0", np.uint8)[:int(lengths.sum())]
    return mhap_amd.FastaData(bases, offsets, lengths, np.arange(1, len(reads) + 1))


def _align(reads, pairs):
    """Realigned records and runs of (x, y, to_rc, diag, band) pairs of reads, aligned on the GPU."""
    fa = _fasta(reads)
    p7 = np.array([(fa.offsets[x], len(reads[x]), fa.offsets[y], len(reads[y]), rc, diag, band) for x, y, rc, diag, band in pairs],
                  np.int64).reshape(-1, 7)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(fa.bases if len(fa.bases) else np.zeros(1, np.uint8), p7)
    recs = cref.records_from_results([x + 1 for x, *_ in pairs], [y + 1 for _, y, *_ in pairs], [len(reads[x]) for x, *_ in pairs],
                                     [len(reads[y]) for _, y, *_ in pairs], [p[2] for p in pairs], results)
    return recs, offsets, ops


def _check(reads, adds, min_cov=4):
    """The shared check: `adds` is a list of (records, op_offsets, ops), one per add.  Every counter of every read, the corrected bytes,
    the offsets, the six counts and skipped_views equal the restatement's.  Returns (seqs, stats, skipped, the session's votes)."""
    ref = cref.Consensus(reads, range(1, len(reads) + 1))
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        for recs, off, ops in adds:
            cs.add(recs, off, ops)
            ref.add(recs, off, ops)
        votes = [cs.votes(r) for r in range(len(reads))]
        seqs, stats, skipped = cs.finish(min_cov)
        out_offsets, flat = cs.offsets.copy(), cs.bytes.copy()
    wseqs, wstats = ref.call(min_cov)
    for r in range(len(reads)):
        assert votes[r].dtype == np.uint16 and votes[r].shape == (len(reads[r]), 24)
        bad = np.argwhere(votes[r].astype(np.int64) != ref.votes[r])
        assert len(bad) == 0, (r, bad[:5].tolist(), votes[r][bad[0][0]].tolist(), ref.votes[r][bad[0][0]].tolist())
    for r in range(len(reads)):
        assert seqs[r] == wseqs[r], (r, stats[r].tolist(), wstats[r].tolist())
    assert stats.tolist() == wstats.tolist() and skipped == ref.skipped_views
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in wseqs])]).tolist() if reads else out_offsets.tolist() == [0]
    assert flat.tobytes() == b"".join(wseqs)
    return seqs, stats, skipped, votes


def _rand(rng, n):
    return bytes(rng.choice(list(b"ACGT"), n).tolist())


def _mutate(rng, s, div):
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


def test_hand_made_piles():
    """The hand-made cases of test_correct_cpu through the aligner: each pile is a target F1 + mid + F2 and evidence reads with another
    middle between the same flanks (40 random bases that end in A and begin with C, so that the aligner has one place for a gap)."""
    rng = np.random.default_rng(11)
    reads, pairs, expect = [], [], {}

    def pile(mid, evidence, want):
        f1, f2 = _rand(rng, 39) + b"A", b"C" + _rand(rng, 39)
        t = len(reads)
        reads.append(f1 + mid + f2)
        for e in evidence:
            reads.append(f1 + e + f2)
            pairs.append((len(reads) - 1, t, 0, 0, 20) if len(reads) % 2 else (t, len(reads) - 1, 0, 0, 20))   # the target as read A and as read B
        expect[t] = f1 + want + f2

    pile(b"G", [b"T"] * 3 + [b"G"], b"T")                       # outvoted 3 : 1 plus own
    pile(b"G", [b"T"] * 2 + [b"G"] * 2, b"G")
    pile(b"G", [b""] * 3 + [b"G"] * 2, b"G")                    # 2 del > total: 6 > 6, 8 > 6, 6 > 7, 8 > 7
    pile(b"G", [b""] * 4 + [b"G"], b"")
    pile(b"G", [b""] * 3 + [b"G"] * 3, b"G")
    pile(b"G", [b""] * 4 + [b"G"] * 2, b"")
    pile(b"G", [b"GT"] * 2 + [b"G"] * 2, b"G")                  # 2 m > span + 1: 4 > 5, 6 > 5, 6 > 6, 8 > 6
    pile(b"G", [b"GT"] * 3 + [b"G"], b"GT")
    pile(b"G", [b"GT"] * 3 + [b"G"] * 2, b"G")
    pile(b"G", [b"GT"] * 4 + [b"G"], b"GT")
    pile(b"G", [b"T"] * 3, b"G")                                # d = min_cov - 1, d = min_cov
    pile(b"G", [b"T"] * 4, b"T")
    pile(b"G", [b"T"] * 2 + [b"A"] * 2 + [b"G"], b"G")          # ties: own among them; the first of A, C, G, T
    pile(b"G", [b"T"] * 2 + [b"A"] * 2, b"A")
    pile(b"G", [b"GT"] * 4, b"GT")                              # insertions of 1, 4 and 6
    pile(b"G", [b"GTATA"] * 4, b"GTATA")
    pile(b"G", [b"GTATATA"] * 4, b"GTATA")
    pile(b"N", [b"G"] * 4, b"G")                                # N in the target, in an M column, inside an insertion
    pile(b"G", [b"N"] * 2 + [b"T"] * 3, b"G")
    pile(b"G", [b"GTNA"] * 4, b"GT")
    recs, off, ops = _align(reads, pairs)
    assert (recs["score"] > 0).all()
    seqs, stats, skipped, _ = _check(reads, [(recs, off, ops)])
    assert skipped == 0
    for t, want in expect.items():
        assert seqs[t] == want, (t, seqs[t], want)
    # the same piles at another minimum coverage
    _check(reads, [(recs, off, ops)], min_cov=3)
    _check(reads, [(recs, off, ops)], min_cov=1)


def _edit_every(rng, s, step, kinds):
    """s with one edit every `step` bases, taken in turn from `kinds` ("X", "I", "D")."""
    out, k = bytearray(), 0
    for pos, c in enumerate(s):
        if pos % step == step - 1 and 10 < pos < len(s) - 10:
            kind = kinds[k % len(kinds)]
            k += 1
            if kind == "X":
                out.append(cref.complement(c))
            elif kind == "I":
                out.append(c)
                out.append(cref.complement(c))
            continue
        out.append(c)
    return bytes(out)


def test_wave_boundaries():
    """Paths with more than 64 and more than 128 runs (a chunk of runs is 64), '=' runs of 65 and of 200 columns (a deal of columns is
    64), an alignment that begins and ends inside both reads, to_rc records; every one four times, so that calls change as well."""
    rng = np.random.default_rng(12)
    reads, pairs = [], []

    def pair(s1, s2, rc, diag=0, band=60):
        reads.append(s1)
        reads.append(rc_bytes(s2) if rc else s2)
        pairs.extend([(len(reads) - 2, len(reads) - 1, rc, diag, band)] * 4)

    a = _rand(rng, 330)
    pair(a, _edit_every(rng, a, 8, "X"), 0)                      # 38 substitutions: 77 runs
    b = _rand(rng, 700)
    pair(b, _edit_every(rng, b, 5, "XID"), 0)                    # about 135 edits of all three kinds
    pair(b, _edit_every(rng, b, 6, "DXI"), 1)                    # ... and on the other strand
    c = _rand(rng, 400)
    c2 = bytearray(c)
    for pos in (30, 96, 297):                                     # '=' runs of 65 (31 .. 95) and 200 (97 .. 296)
        c2[pos] = cref.complement(c2[pos])
    pair(c, bytes(c2), 0)
    pair(c, bytes(c2), 1)
    core = _rand(rng, 250)
    # (random flanks would not end it: at +2 / -2 and gaps of 2 + (L - 1) a local alignment runs on through unrelated bases)
    pair(b"A" * 37 + core + b"A" * 55, b"C" * 90 + _mutate(rng, core, 0.1) + b"C" * 21, 0, diag=53, band=40)
    pair(b"A" * 37 + core + b"A" * 55, b"C" * 90 + _mutate(rng, core, 0.1) + b"C" * 21, 1, diag=53, band=40)
    recs, off, ops = _align(reads, pairs)
    n_runs = np.diff(off)[::4]
    assert 64 < n_runs[0] <= 128 and n_runs[1] > 128 and n_runs[2] > 128, n_runs.tolist()
    for q in (12, 16):
        lens = [(int(r) >> 4, int(r) & 15) for r in ops[off[q]:off[q + 1]]]
        assert (65, OP_EQ) in lens and (200, OP_EQ) in lens, lens
    for q in (20, 24):
        assert recs[q]["a1"] > 20 and recs[q]["a2"] < recs[q]["alen"] - 20 and recs[q]["b1"] > 10 and recs[q]["b2"] < recs[q]["blen"] - 10, recs[q]
    codes = {int(r) & 15 for r in ops[off[4]:off[5]]}
    assert codes == {OP_I, OP_D, OP_EQ, OP_X}
    seqs, stats, _, _ = _check(reads, [(recs, off, ops)])
    assert seqs[0] == reads[1] and seqs[1] == reads[0]           # four views against own: each read becomes the other
    assert stats[:, 2:5].sum() > 300


@pytest.fixture(scope="module")
def seventy():
    rng = np.random.default_rng(13)
    target = _rand(rng, 300)
    reads, pairs = [target], []
    for k in range(70):
        rc = k % 2
        e = _mutate(rng, target[k % 7 * 5:300 - k % 5 * 9], 0.12)
        reads.append(rc_bytes(e) if rc else e)
        pairs.append((0, k + 1, rc, -(k % 7 * 5), 40) if k % 3 else (k + 1, 0, rc, k % 7 * 5, 40))
    # with to_rc and the target as read B the diagonal is that of the target's reverse complement
    pairs = [(x, y, rc, (len(reads[y]) - len(reads[x])) - d if (rc and y == 0) else d, b) for x, y, rc, d, b in pairs]
    return reads, _align(reads, pairs)


def test_seventy_overlaps_in_one_add_and_in_three(seventy):
    reads, (recs, off, ops) = seventy
    assert (recs["score"] > 0.7).sum() >= 60
    from mhap_amd.correct import select_paths
    one = _check(reads, [(recs, off, ops)])
    parts = [np.arange(0, 23), np.arange(0, 0), np.arange(23, 70)]
    three = _check(reads, [(recs[rows],) + select_paths(off, ops, rows) for rows in parts])
    assert one[0] == three[0] and one[1].tolist() == three[1].tolist()
    for a, b in zip(one[3], three[3]):
        assert a.tobytes() == b.tobytes()
    assert one[3][0][:, :5].sum(axis=1).max() > 60 and one[1][0, 5] == 0 and one[1][0, 2:5].sum() == 0     # 70 noisy views agree on the target


def test_the_cap_of_65535_views():
    """65 537 copies of one record of two identical 40-base reads: both targets stop at 65 535 views, the last two records' four views
    are skipped, and no counter has carried into the other half of its word."""
    read = _rand(np.random.default_rng(14), 40)
    reads = [read, read, b"ACGT" * 10]
    rec, off, ops = _align(reads, [(0, 1, 0, 0, 5)])
    assert ops.tolist() == [40 << 4 | OP_EQ]
    n = 65537
    recs = np.repeat(rec, n)
    seqs, stats, skipped, votes = _check(reads, [(recs, np.arange(n + 1, dtype=np.int64), np.repeat(ops, n))])
    assert skipped == 4
    for r in (0, 1):
        want = np.zeros((40, 24), np.int64)
        for t, c in enumerate(read):
            want[t, b"ACGT".index(c)] = 65535
        want[:39, 5] = 65535
        assert votes[r].astype(np.int64).tolist() == want.tolist()
    assert votes[2].sum() == 0 and seqs == reads and stats[2].tolist() == [40, 40, 0, 0, 0, 40]


def test_quality_workload_equals_the_restatement():
    """The workload of test_correct_cpu's quality condition with the realignment on the GPU: the session's output is the restatement's
    on the GPU's own records and paths, and it meets the same condition."""
    reads, truths, bases, pairs, meta = cref.quality_workload(7)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    recs = cref.quality_records(reads, meta, results)
    seqs, stats, skipped, _ = _check(reads, [(recs, offsets, ops)])
    raw = sum(cref.levenshtein(r, t) for r, t in zip(reads, truths))
    cor = sum(cref.levenshtein(s, t) for s, t in zip(seqs, truths))
    print(f"raw {raw}, corrected {cor}, ratio {cor / raw:.3f}")
    assert cor < 0.5 * raw and skipped == 0


def test_reads_nobody_voted_on_empty_adds_and_an_empty_read(seventy):
    reads = [b"ACGTNACGT", b"", b"TTTTGGGG", b"A"]
    none = (np.zeros(0, mhap_amd.api.RECORD_DTYPE), np.zeros(1, np.int64), np.zeros(0, np.uint32))
    seqs, stats, skipped, _ = _check(reads, [none, none])
    assert seqs == reads and stats.tolist() == [[9, 9, 0, 0, 0, 9], [0, 0, 0, 0, 0, 0], [8, 8, 0, 0, 0, 8], [1, 1, 0, 0, 0, 1]] and skipped == 0
    seqs, _, _, _ = _check(reads, [])
    assert seqs == reads
    _check([], [none])
    # records without an alignment and records of a read with itself vote nothing, between records that do
    r70, (recs, off, ops) = seventy
    extra = r70 + [b"", b"GGGGGGGGGGGG"]
    mixed = np.concatenate([recs[:3], recs[:2]])
    mixed[3]["to_id"] = mixed[3]["from_id"]
    mixed[3]["blen"] = mixed[3]["alen"]
    from mhap_amd.correct import select_paths
    moff, mops = select_paths(off, ops, [0, 1, 2, 0, 1])
    cut = moff.copy()
    cut[5:] = cut[4]                                              # the last record: no runs
    _check(extra, [(mixed, cut, mops[:cut[-1]])])
    # convenience entry point
    seqs, stats, skipped = mhap_amd.correct_reads(recs, _fasta(r70), off, ops)
    assert seqs == _check(r70, [(recs, off, ops)])[0]


def test_invalid_records_are_refused_with_their_index(seventy):
    reads, (recs, off, ops) = seventy
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        bad = recs[:3].copy()
        bad[2]["to_id"] = 999
        with pytest.raises(mhap_amd.MhapError, match="record 2 names read 999"):
            cs.add(bad, off[:4], ops[:off[3]])
        bad = recs[:3].copy()
        bad[1]["alen"] += 1
        with pytest.raises(mhap_amd.MhapError, match="record 1 gives read"):
            cs.add(bad, off[:4], ops[:off[3]])
        bad = recs[:3].copy()
        bad[0]["a2"] -= 1
        with pytest.raises(mhap_amd.MhapError, match="record 0 has runs"):
            cs.add(bad, off[:4], ops[:off[3]])
        assert all(cs.votes(r).sum() == 0 for r in range(4))      # a refused call has cast no vote
        with pytest.raises(mhap_amd.MhapError, match="min_cov"):
            cs.finish(0)
        cs.add(recs[:3], off[:4], ops[:off[3]])
        assert cs.votes(0).sum() > 0


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


def test_driver_and_tool_write_the_same_fasta(tmp_path):
    fasta = os.path.join(GOLD, "small_reads.fasta")
    plain = _cli(["-s", fasta])
    base = _cli(["-s", fasta, "--realign"])
    out = tmp_path / "corrected.fasta"
    cor = _cli(["-s", fasta, "--realign", "--correct", str(out)])
    assert plain.returncode == 0 and base.returncode == 0 and cor.returncode == 0, cor.stderr[-2000:]
    # stdout is what it is without --correct: the same bytes line for line.  The driver prints records in the order the search's
    # kernels append them, which differs between two runs of the same command, so the lines are compared sorted, as every test of
    # the driver's output does.
    assert sorted(cor.stdout.split(b"\n")) == sorted(base.stdout.split(b"\n")) and len(cor.stdout) == len(base.stdout) > 1000
    assert b"correct" not in base.stderr and b"--correct-min-coverage = 4" in cor.stderr
    text = out.read_text()
    lines = text.split("\n")
    fa = mhap_amd.FastaData.from_file(fasta)
    assert len(lines) == 2 * len(fa) + 1 and lines[0].startswith(">1 len=") and lines[-1] == ""
    totals = [l for l in cor.stderr.decode().split("\n") if l.startswith("Corrected ")]
    assert len(totals) == 1 and totals[0].startswith(f"Corrected {len(fa)} reads: {int(fa.lengths.sum())} bases in, ") and "skipped_views = 0" in totals[0]
    assert any(" sub=0 del=0 ins=0 " not in l for l in lines[0::2] if l), "the fixture's overlaps change at least one read"
    # the stand-alone tool on the driver's own plain output
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tool_out = tmp_path / "tool.fasta"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.correct", str(tmp_path / "ovl.txt"), fasta, "-o", str(tool_out)], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tool_out.read_text() == text
    assert totals[0] in p.stderr
    # --store-full-id: the stored name in the header; another minimum coverage and an identity floor through both
    cor2 = _cli(["-s", fasta, "--realign", "--correct", str(out), "--store-full-id", "--correct-min-coverage", "2", "--realign-min-identity", "0.8"])
    assert cor2.returncode == 0, cor2.stderr[-2000:]
    names = [l[1:].split()[0] for l in open(fasta) if l.startswith(">")]
    got = out.read_text().split("\n")
    assert [l[1:].split()[0] for l in got[0::2] if l] == names
    p = subprocess.run([sys.executable, "-m", "mhap_amd.correct", str(tmp_path / "ovl.txt"), fasta, "--min-coverage", "2", "--min-identity", "0.8"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split("\n")[1::2] == got[1::2]
