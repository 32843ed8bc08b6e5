"""Sequence assessment on the GPU (kmer_set_kernel, kmer_eval_kernel, kmer_eval_intervals_kernel, kmer_set_compare_kernel) against
the restatement of its contract (tests/kmer_qv_ref.py): rows, intervals, the table and the BED text, set membership and the set
comparison, equal and not merely close.  The reads are error-free and tile a small random genome, so the set is exactly the genome's
k-mers; the sequences are the genome with planted edits at the edges of the kernel's lanes (64 positions) and tiles (4 032)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import kmer_qv_ref as R
import mhap_amd
from mhap_amd import FastaScan, MhapError
from test_kmer_count import KMERS_CLI, ROOT
from test_kmer_count_edges_gpu import _fasta, _handle
from test_kmer_qv_cpu import LANE, TILE, _edited

GENOME = 20_000


def _genome(seed):
    rnd = random.Random(seed)
    return "".join(rnd.choice("ACGT") for _ in range(GENOME)), rnd


def _tiling_reads(genome, length=1000, step=500):
    return [genome[i:i + length] for i in range(0, len(genome) - length + step, step)]


def _set_of(ms, reads, k, canonical, min_count):
    ms.kmer_count_begin(k, canonical)
    ms.kmer_count_add(_fasta(reads))
    return ms.kmer_count_finish_set(min_count)


def _check_eval(ev, seqs, kset, k, canonical, tmp_path, what):
    rows, ivs = R.evaluate_all(seqs, kset, k, canonical)
    assert ev.rows.tolist() == rows, what
    assert [tuple(i) for i in ev.intervals.tolist()] == ivs, what
    assert ev.totals.tolist() == [sum(r[f] for r in rows) for f in range(5)], what
    ev.write_table(tmp_path / "t.tsv")
    ev.write_bed(tmp_path / "b.bed")
    assert (tmp_path / "t.tsv").read_text() == R.table(rows, k), what
    assert (tmp_path / "b.bed").read_text() == R.bed(ivs, len(seqs)), what
    return rows, ivs


def _cases(genome, rnd, k):
    """Lengths around k, the lane and the tile; edits that begin, end and straddle runs and unsupported stretches at their edges."""
    cases = [genome[:n] for n in (0, k - 1, k, k + 1, LANE + k - 2, LANE + k - 1, LANE + k, TILE + k - 2, TILE + k - 1, TILE + k)]   # Q-1, Q, Q+1, T-1, T, T+1 windows
    cases += [genome[:n] for n in (LANE - 1, LANE, LANE + 1, TILE - 1, TILE, TILE + 1)]                                             # ... and positions
    n = 2 * TILE + k                                                                                                                # 2T + 1 windows
    cases.append(genome[:n])
    for at in (0, n - 1, LANE - 1, LANE, LANE + k - 1, TILE - k, TILE - 1, TILE, TILE + k - 1, 2 * TILE - 1, 2 * TILE):
        cases.append(_edited(genome, rnd, n, {at: "x"}))
        cases.append(_edited(genome, rnd, n, {at: "x", at + k - 1: "x"}))                   # fewer than k apart: one run, a longer stretch
        cases.append(_edited(genome, rnd, n, {at: "N"}))
    for at in (LANE - 3, TILE - 5):
        cases.append(_edited(genome, rnd, n, {at + j: "N" for j in range(k + 3)}))          # a run of N longer than k over the edge
        cases.append(_edited(genome, rnd, n, {at: "R", at + 2 * k: "a", at + 4 * k: "x"}))  # raw bytes: an IUPAC code, a lower-case base
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 9, 12, 16])
def test_rows_intervals_and_files_match_the_restatement(tmp_path, k):
    genome, rnd = _genome(50 + k)
    if k % 2 == 0:   # a palindromic k-mer (its own reverse complement) at 300, in the reads and in every longer sequence
        half = genome[300:300 + k // 2]
        genome = genome[:300] + half + half.translate(str.maketrans("ACGT", "TGCA"))[::-1] + genome[300 + k:]
        assert R.window_key(genome, 300, k, False) == R.window_key(genome, 300, k, True)
    reads = _tiling_reads(genome)
    cases = _cases(genome, rnd, k)
    for canonical in (True, False):
        cnt = R.count(reads, k, canonical)
        # k <= 2: every k-mer occurs, so a threshold that leaves some out; else every k-mer of the reads
        min_count = sorted(cnt.values())[len(cnt) // 2] if k <= 2 else 1
        kset, _ = R.solid(cnt, min_count)
        with _handle() as ms, _set_of(ms, reads, k, canonical, min_count) as gs:
            assert (gs.k, gs.canonical, gs.min_count) == (k, canonical, min_count)
            assert (gs.total, gs.distinct, gs.members) == (sum(cnt.values()), len(cnt), len(kset))
            ev = ms.kmer_set_eval(gs, _fasta(cases))
            rows, _ = _check_eval(ev, cases, kset, k, canonical, tmp_path, (k, canonical))
            if k > 2:
                assert sum(r[2] for r in rows) > 0 and sum(r[4] for r in rows) > 0
            # the same sequences without their raw bytes: the 2-bit path alone
            pure = [s for s in cases if set(s) <= set("ACGT")]
            _check_eval(ms.kmer_set_eval(gs, _fasta(pure)), pure, kset, k, canonical, tmp_path, (k, canonical, "pure"))


@pytest.mark.gpu
def test_more_sequences_than_one_block_of_the_work_item_prefix(tmp_path):
    k = 12
    genome, rnd = _genome(7)
    reads = _tiling_reads(genome)
    seqs = []
    for i in range(1100):
        a, n = rnd.randrange(GENOME - 400), rnd.choice((0, 5, 11, 12, 13, 40, 64, 75, 76, 200, 333))
        seqs.append(_edited(genome[a:], rnd, n, {rnd.randrange(max(n, 1)): rnd.choice("xxN")} if i % 3 else {}))
    seqs[500] = _edited(genome, rnd, TILE + 700, {TILE - 1: "x", 2000: "x"})   # one sequence of two tiles among them
    kset = set(R.count(reads, k, True))
    with _handle() as ms, _set_of(ms, reads, k, True, 1) as gs:
        _check_eval(ms.kmer_set_eval(gs, _fasta(seqs)), seqs, kset, k, True, tmp_path, "1100")


@pytest.mark.gpu
def test_scan_in_several_groups_equals_one_call(tmp_path, monkeypatch):
    k = 16
    genome, rnd = _genome(11)
    reads = _tiling_reads(genome)
    g = np.frombuffer(genome.encode(), dtype=np.uint8)
    seqs, rs = [], np.random.default_rng(5)
    for i in range(140):                           # 1.4 Mbase: the ingest's first group takes 2^20 bases, the others 120 000 each
        a = int(rs.integers(0, GENOME - 10_000))
        s = g[a:a + 10_000].copy()
        at = rs.integers(0, 10_000, size=6)
        s[at] = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rs.integers(0, 10, size=6)]
        seqs.append(s.tobytes().decode())
    path = tmp_path / "seqs.fasta"
    path.write_text("".join(f">contig_{i} note\n{s[:7000]}\n{s[7000:]}\n" for i, s in enumerate(seqs)))
    monkeypatch.setenv("MHAP_INGEST_GROUP_BASES", "120000")
    with _handle() as ms, _set_of(ms, reads, k, True, 1) as gs:
        with FastaScan(str(path)) as scan:
            ev = ms.kmer_set_eval(gs, scan)
        one = ms.kmer_set_eval(gs, _fasta([s.upper() for s in seqs]))   # (the ingest upper-cases a scanned file)
        assert ev.names == [f"contig_{i}" for i in range(140)]
        assert ev.rows.tolist() == one.rows.tolist() and ev.intervals.tolist() == one.intervals.tolist()
        assert ev.totals[2] > 0 and len(ev.intervals) > 100 and ev.intervals[-1][0] > 130
        rows, ivs = R.evaluate_all([s.upper() for s in seqs[:3]], set(R.count(reads, k, True)), k, True)
        assert ev.rows[:3].tolist() == rows and [tuple(i) for i in ev.intervals.tolist() if i[0] < 3] == ivs
        ev.write_bed(tmp_path / "b.bed")
        assert (tmp_path / "b.bed").read_text() == R.bed([tuple(i) for i in ev.intervals.tolist()], 140, ev.names)


def _all_values(k):
    return np.arange(4 ** k, dtype=np.uint64)


def _members(kset):
    return sorted(R.key_value(key) for key in kset)


def _check_set(monkeypatch, calls, cnt, k, canonical, flush, min_count):
    if flush:
        monkeypatch.setenv("MHAP_KMER_STAGE_WINDOWS", "1")   # (read at begin: every add after the first flushes the staged ones)
    what = (k, canonical, flush, min_count)
    kset, used = R.solid(cnt, min_count)
    with _handle() as ms:
        ms.kmer_count_begin(k, canonical)
        monkeypatch.delenv("MHAP_KMER_STAGE_WINDOWS", raising=False)
        for c in calls:
            ms.kmer_count_add(_fasta(c))
        with ms.kmer_count_finish_set(min_count) as gs:
            assert (gs.min_count, gs.total, gs.distinct, gs.members) == (used, sum(cnt.values()), len(cnt), len(kset)), what
            assert np.flatnonzero(ms.kmer_set_contains(gs, _all_values(k))).tolist() == _members(kset), what
            assert ms.kmer_set_contains(gs, np.array([4 ** k, 2 ** 63], dtype=np.uint64)).tolist() == [0, 0]
            if not kset:   # the empty set: every window is missing, every covered base unsupported
                seq = calls[0][0][:700] + "N" + calls[0][0][700:900]
                ev = ms.kmer_set_eval(gs, _fasta([seq]))
                rows, ivs = R.evaluate_all([seq], set(), k, canonical)
                assert rows[0][2] == rows[0][1] > 0 and ev.rows.tolist() == rows and [tuple(i) for i in ev.intervals.tolist()] == ivs
        with pytest.raises(MhapError):   # the count ended with the set
            ms.kmer_count_finish()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 9])
def test_set_building_and_contains_over_the_whole_space(monkeypatch, k):
    rnd = random.Random(90 + k)
    unit = "".join(rnd.choice("ACGT") for _ in range(3000))
    calls = [[unit[:2000], unit[500:2500]], [unit[1000:3000] + "N" + unit[:300]], ["".join(rnd.choice("ACGT") for _ in range(1500))]]
    for canonical in (True, False):
        cnt = R.count([s for c in calls for s in c], k, canonical)
        some, top = sorted(cnt.values())[len(cnt) // 3], max(cnt.values())   # a k-mer's count, and the largest
        for min_count in (1, 2, some, some + 1, top, top + 1, 0):
            _check_set(monkeypatch, calls, cnt, k, canonical, False, min_count)
        for min_count in (1, some, 0):                                        # the counts made across flushes
            _check_set(monkeypatch, calls, cnt, k, canonical, True, min_count)


@pytest.mark.gpu
def test_the_valley_separates_error_kmers_from_the_genome(tmp_path):
    """Reads with errors: every read k-mer is in the min_count 1 set, so a sequence that copies a read's error passes; at the valley it does not."""
    k = 12
    genome, rnd = _genome(23)
    reads = []
    for i in range(0, GENOME - 1000 + 250, 250):   # coverage 4
        r = list(genome[i:i + 1000])
        for _ in range(10):
            p = rnd.randrange(1000)
            r[p] = "ACGT"[("ACGT".index(r[p]) + 1 + rnd.randrange(3)) % 4]
        reads.append("".join(r))
    cnt = R.count(reads, k, True)
    kset, used = R.solid(cnt, 0)
    assert used == R.valley(R.histogram(cnt)) and 1 < used <= 4
    seqs = [genome[:5000], reads[7], reads[30][:400]]
    with _handle() as ms, _set_of(ms, reads, k, True, 0) as gs:
        assert (gs.min_count, gs.members) == (used, len(kset))
        rows, _ = _check_eval(ms.kmer_set_eval(gs, _fasta(seqs)), seqs, kset, k, True, tmp_path, "valley")
        assert rows[1][2] > 0
    with _handle() as ms, _set_of(ms, reads, k, True, 1) as gs:
        rows, _ = _check_eval(ms.kmer_set_eval(gs, _fasta(seqs)), seqs, set(cnt), k, True, tmp_path, "min_count 1")
        assert rows[1][2] == 0


@pytest.mark.gpu
def test_compare(tmp_path):
    genome, rnd = _genome(31)
    for k, canonical in ((16, True), (12, False), (9, True), (2, False)):
        whole, half, other = [genome], [genome[:GENOME // 2]], ["A" * 300 + "C" * 300 if not canonical else "AC" * 300]
        with _handle() as ms:
            sets = {name: _set_of(ms, seqs, k, canonical, 1) for name, seqs in (("whole", whole), ("half", half), ("other", other))}
            ref = {name: set(R.count(seqs, k, canonical)) for name, seqs in (("whole", whole), ("half", half), ("other", other))}
            for a in sets:
                for b in sets:
                    assert ms.kmer_set_compare(sets[a], sets[b]) == R.compare(ref[a], ref[b]), (k, canonical, a, b)
            assert ms.kmer_set_compare(sets["whole"], sets["whole"]) == (len(ref["whole"]),) * 3
            assert ms.kmer_set_compare(sets["whole"], sets["half"])[2] == len(ref["half"])   # a subset
            if k >= 12:
                assert ms.kmer_set_compare(sets["whole"], sets["other"])[2] == 0             # disjoint sets
            for wrong in (_set_of(ms, whole, k - 1, canonical, 1), _set_of(ms, whole, k, not canonical, 1)):
                with pytest.raises(MhapError, match="differ in k or in canonical"):
                    ms.kmer_set_compare(sets["whole"], wrong)
                wrong.close()
            for s in sets.values():
                s.close()


@pytest.mark.gpu
def test_both_tools_end_to_end(tmp_path):
    """k = 16, 12 substitutions at least 2k apart and away from the ends: each makes 16 missing windows in one run and leaves one base that
    no present window covers.  (Checked with the restatement for this seed: no edited window collides with a k-mer of the genome.)"""
    k = 16
    genome, rnd = _genome(2026)
    reads = _tiling_reads(genome)
    at = [1000 + 1500 * i for i in range(12)]
    asm = _edited(genome, rnd, GENOME, {p: "x" for p in at})
    kset = set(R.count(reads, k, True))
    rows, ivs = R.evaluate_all([asm, genome[:3000]], kset, k, True)
    assert rows[0][1:] == [GENOME - k + 1, 12 * 16, 12, 12] and ivs == [(0, p, p + 1) for p in at] and rows[1][2:] == [0, 0, 0]
    rf, sf = tmp_path / "reads.fasta", tmp_path / "asm.fasta"
    rf.write_text("".join(f">r{i}\n{r}\n" for i, r in enumerate(reads)))
    sf.write_text(f">utg1 len={GENOME}\n{asm}\n>utg2\n{genome[:3000]}\n")
    names = ["utg1", "utg2"]
    out = {t: (tmp_path / f"{t}.tsv", tmp_path / f"{t}.bed") for t in ("cli", "py")}
    r = subprocess.run([KMERS_CLI, "--assess", str(sf), "--assess-min-count", "1", "--assess-table", str(out["cli"][0]), "--assess-bed", str(out["cli"][1]),
                        "-o", str(tmp_path / "f.txt"), str(rf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "mhap_amd.kmer_qv", str(rf), str(sf), "--min-count", "1", "--table", str(out["py"][0]), "--bed", str(out["py"][1])],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    assert out["cli"][0].read_text() == out["py"][0].read_text() == R.table(rows, k, names)
    assert out["cli"][1].read_text() == out["py"][1].read_text() == R.bed(ivs, 2, names)
    cli_lines = [l for l in r.stderr.split("\n") if l]
    py_lines = [l for l in p.stderr.split("\n") if l]   # (a runtime library may write a line of its own ahead of the tool's)
    assert len(cli_lines) == 2 and cli_lines[0].startswith("Counted ") and cli_lines[1] == py_lines[-1]
    own = set(R.count([asm, genome[:3000]], k, True))
    line = cli_lines[1]
    assert f"Assessed 2 sequences, {GENOME + 3000} bases against {len(kset)} solid 16-mers (count >= 1)" in line
    assert f"{GENOME + 3000 - 2 * (k - 1)} windows, 192 missing in 12 runs, 12 unsupported bases, QV {R.qv(GENOME + 3000 - 2 * (k - 1), 192, k)[1]:.2f}" in line
    assert f"completeness {len(kset & own) / len(kset):.6f} ({len(kset & own)} of the solid 16-mers are among the sequences' {len(own)})" in line
    # the -f file is the one the tool writes without --assess, and the valley default runs
    plain = subprocess.run([KMERS_CLI, "-o", str(tmp_path / "g.txt"), str(rf)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and (tmp_path / "f.txt").read_bytes() == (tmp_path / "g.txt").read_bytes()
    res = mhap_amd.assess(str(rf), str(sf), k=k)
    assert res.min_count == R.solid(R.count(reads, k, True), 0)[1]
    assert (res.solid, res.own, res.both) == R.compare(R.solid(R.count(reads, k, True), 0)[0], own)
    assert res.names == names and res.line.startswith("Assessed 2 sequences")
