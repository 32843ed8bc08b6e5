"""Graph cleaning on the GPU (mhap_graph_clean / _copy_dropped / _copy_removed, unitig_kernels.hip) against its CPU restatement
(tests/graph_clean_ref.py over unitig_ref.py and string_graph_ref.py), exactly: the dropped and removed bytes, the counts, every table
of the cleaned unitigs, their spelled sequences and both GFA texts; then `mhap-hip --realign --gfa --gfa-unitigs --gfa-clean` against
`python -m mhap_amd.graph --clean` and against the genome its reads were drawn from.  The shapes are those of test_graph_clean_cpu.py,
where their expected answers are written out."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import graph_clean_ref as cr  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import unitig_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
SENTINEL = 0x01       # a byte no read holds and the complement table leaves alone
TABLES = ("unitig_start", "unitig_len", "circular", "vertex", "offset", "span", "links")


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _same_tables(got, exp):
    for k in TABLES:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (k, got[k].shape, exp[k].shape)
        if not np.array_equal(got[k], exp[k]):
            bad = np.flatnonzero((got[k] != exp[k]).reshape(len(exp[k]), -1).any(axis=1))
            assert False, (k, bad[:5], got[k][bad[0]], exp[k][bad[0]])
    assert got["counts"] == exp["counts"]


def _compare(gs, ref, bases, offsets, **clean):
    """Clean the session (its finish has run) and the finished restatement `ref` alike and compare everything; returns (the
    restatement's Cleaned, what the session gave)."""
    want = cr.Cleaned(ref, **clean)
    counts = gs.clean(**clean)
    assert counts == want.counts, (counts, want.counts)
    dropped, removed = gs.dropped(), gs.removed()
    assert dropped.dtype == np.uint8 and dropped.tolist() == want.dropped
    assert removed.dtype == np.uint8 and removed.tolist() == want.removed
    got, exp = gs.cleaned_unitigs(), want.unitigs.tables()
    _same_tables(got, exp)
    u = want.unitigs
    assert gs.unitigs_info() == (len(u.unitig_len), len(u.vertex), len(u.links), sum(u.unitig_len))
    out = np.full(sum(u.unitig_len), SENTINEL, np.uint8)
    gs.spell_into(bases, offsets, out)
    assert not (out == SENTINEL).any()
    want_seqs = u.sequences(bases, offsets, ref.lengths)
    assert out.tobytes() == b"".join(want_seqs)
    fasta = mhap_amd.FastaData(bases, offsets, ref.lengths, ref.ids)
    seqs = gs.unitig_sequences(fasta)
    assert seqs == want_seqs
    utext = gs.unitig_gfa(fasta)
    assert utext == u.gfa(ref.ids, want_seqs)
    text = gs.gfa(cleaned=True)
    assert text == want.gfa() and gs.gfa() == ref.gfa()
    return want, (counts, dropped.tolist(), removed.tolist(), got, seqs, utext, text)


def _same(a, b):
    assert a[:3] == b[:3] and a[4:] == b[4:] and a[3]["counts"] == b[3]["counts"] and all((a[3][k] == b[3][k]).all() for k in TABLES)


def _check(ms, ids, lengths, adds, bases=None, offsets=None, params=None, **clean):
    """One session and one restatement given the same adds, finished once, cleaned and compared; bases are drawn when none come."""
    if bases is None:
        bases, offsets = ur.random_bases(lengths, len(ids) + 7, pad=1)
    ref = sg.Graph(ids, lengths, sg.Params(**(params or {})))
    with mhap_amd.GraphSession(ids, lengths, handle=ms, **(params or {})) as gs:
        for recs in adds:
            gs.add(recs)
            ref.add(recs)
        gs.finish()
        ref.finish()
        return _compare(gs, ref, bases, offsets, **clean)


def _shape(ms, shape, **clean):
    ids, lengths, recs = shape
    return _check(ms, ids, lengths, [recs], **clean)


def _members(u):
    return np.diff(u["unitig_start"]).tolist()


@pytest.mark.parametrize("mode", ["out", "in", "rc"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_tip_length_boundary(ms, k, mode):
    want, got = _shape(ms, cr.tip_on_backbone(k, mode))
    assert got[0]["tip_reads"] == (k if k <= 4 else 0) and (_members(got[3]) == [12]) == (k <= 4)


@pytest.mark.parametrize("arms", [(2, 3, 2500, 2500), (2, 2, 2500, 2600), (2, 2, 2700, 2500), (2, 2, 2500, 2500)])
def test_terminal_fork(ms, arms):
    """Decided by members, by bases either way, and by the unitig's number; with the isolated chain, the lone reads and the cycle."""
    want, got = _shape(ms, cr.terminal_fork(*arms, extras=True))
    assert got[0]["tip_unitigs"] == 1 and got[0]["tip_reads"] == 2 and sorted(_members(got[3])) == [1, 1, 3, 5, 8 + arms[1]]
    assert got[3]["counts"]["circular"] == 1


@pytest.mark.parametrize("at", [1, 6])
def test_star_of_70_tips(ms, at):
    """More in-links on one unitig end than a wave has lanes: at the backbone's first read 69 tips go and the best-ranked one joins
    the backbone; at read 6 the backbone holds the junction itself and all 70 go."""
    want, got = _shape(ms, cr.star(70, at))
    assert got[0]["tip_unitigs"] == (69 if at == 1 else 70) and got[0]["rounds"] == 2 and _members(got[3]) == [13 if at == 1 else 12]


def test_simple_bubbles(ms):
    want, got = _shape(ms, cr.bubble((2, 3)))
    assert got[0]["bubble_reads"] == 2 and _members(got[3]) == [15]
    want, got = _shape(ms, cr.bubble((2, 3, 4)))
    assert got[0]["bubble_unitigs"] == 2 and got[0]["bubble_reads"] == 5 and _members(got[3]) == [16]
    long2 = cr.bubble((2, 3), inner=(9000, 2500))                                       # the lesser branch is 29 000 bases long
    assert _shape(ms, long2, bubble_bases=29000)[1][0]["bubble_unitigs"] == 1
    assert _shape(ms, long2, bubble_bases=28999)[1][0] == dict(zip(cr.COUNT_NAMES, (1, 0, 0, 0, 0, 0)))
    want, got = _shape(ms, cr.bubble((2, 3), second_in=True), tip_reads=0)              # a second in-link: no branch, nothing popped
    assert got[0] == dict(zip(cr.COUNT_NAMES, (1, 0, 0, 0, 0, 0))) and got[6] == want.g.gfa()


def test_cascade(ms):
    want, got = _shape(ms, cr.bubble((2, 3), second_in=True))
    assert got[0] == dict(zip(cr.COUNT_NAMES, (3, 1, 1, 1, 2, 8))) and _members(got[3]) == [15]
    want, got = _shape(ms, cr.bubble((2, 3), second_in=True), max_rounds=1)
    assert got[0] == dict(zip(cr.COUNT_NAMES, (1, 1, 1, 0, 0, 2))) and sorted(_members(got[3])) == [2, 3, 6, 6]


def test_thinned_layout_of_1100_reads_in_one_add_three_adds_and_shuffled(ms):
    ids, lengths, reads, recs = cr.thinned_layout()
    _, bases, offsets = ur.plant(reads, 2, 880000)
    want, one = _check(ms, ids, lengths, [recs], bases, offsets)
    print(one[0], want.unitigs.counts)
    assert want.unitigs.counts["unitigs"] < ur.of_graph(want.g).counts["unitigs"] and one[3]["counts"]["unitigs"] == want.unitigs.counts["unitigs"]
    assert want.counts["tip_unitigs"] > 0 and want.counts["bubble_unitigs"] > 0 and 2 * len(ids) > 2048
    third = len(recs) // 3
    _same(one, _check(ms, ids, lengths, [recs[:third], recs[third:third + 1], recs[third + 1:]], bases, offsets)[1])
    _same(one, _check(ms, ids, lengths, [recs[np.random.default_rng(1).permutation(len(recs))]], bases, offsets)[1])


def test_removed_unitigs_and_dropped_reads_in_every_scan_tile(ms):
    want, got = _shape(ms, cr.tiles())
    assert got[0] == dict(zip(cr.COUNT_NAMES, (2, 3, 6, 3, 6, 30)))
    gone = np.flatnonzero(got[1])
    for lo, hi in ((0, 512), (512, 1024), (1024, 1100)):                                # reads: their vertices lie in the three tiles
        assert ((gone >= lo) & (gone < hi)).sum() == 4


def test_calls_out_of_order_are_refused_and_the_uncleaned_unitigs_stay_what_they_were(ms):
    ids, lengths, recs = cr.bubble((2, 3), second_in=True)
    bases, offsets = ur.random_bases(lengths, 3, pad=1)
    ref = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_clean: no mhap_graph_finish has completed"):
            gs.clean()
        half = len(recs) // 2
        gs.add(recs[:half])
        ref.add(recs[:half])
        gs.finish()
        ref.finish()
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_dropped: no mhap_graph_clean has completed"):
            gs.dropped()
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_copy_removed: no mhap_graph_clean has completed"):
            gs.removed()
        for bad in (dict(tip_reads=-1), dict(bubble_bases=-1), dict(max_rounds=0)):
            with pytest.raises(mhap_amd.MhapError, match="must be >= 0 and max_rounds >= 1"):
                gs.clean(**bad)
        _compare(gs, ref, bases, offsets)
        gs.add(recs[half:])
        ref.add(recs[half:])
        with pytest.raises(mhap_amd.MhapError, match="mhap_graph_clean: records were added after the last mhap_graph_finish"):
            gs.clean()
        gs.finish()                                                                     # forgets the clean state, invalidates the unitigs
        ref.finish()
        assert gs.unitigs_info()[0] == -1
        with pytest.raises(mhap_amd.MhapError, match="no mhap_graph_clean has completed"):
            gs.dropped()
        with pytest.raises(mhap_amd.MhapError, match="no clean"):
            gs.cleaned_unitigs()
        plain = gs.unitigs()
        _same_tables(plain, ur.of_graph(ref).tables())
        want, first = _compare(gs, ref, bases, offsets)
        assert first[0]["rounds"] == 3
        again = gs.unitigs()                                                            # the uncleaned ones, as before the clean
        _same_tables(again, plain)
        assert gs.dropped().tolist() == first[1] and gs.removed().tolist() == first[2]  # ... and the bytes are not disturbed
        assert gs.unitig_gfa(mhap_amd.FastaData(bases, offsets, lengths, ids)) == ur.of_graph(ref).gfa(ids, ur.of_graph(ref).sequences(bases, offsets, lengths))
        _same_tables(gs.cleaned_unitigs(), first[3])                                    # read at the clean, nothing is rebuilt
        _same(first, _compare(gs, ref, bases, offsets)[1])                              # twice: each clean starts from the uncleaned graph
        _same(_compare(gs, ref, bases, offsets, max_rounds=1)[1], _check(ms, ids, lengths, [recs], bases, offsets, max_rounds=1)[1])


def test_no_reads_and_no_records(ms):
    want, got = _check(ms, [], [], [], np.zeros(0, np.uint8), np.zeros(0, np.int64))
    assert got[0] == dict(zip(cr.COUNT_NAMES, (1, 0, 0, 0, 0, 0))) and got[5] == "H\tVN:Z:1.0\n" and got[6] == "H\tVN:Z:1.0\n"
    want, got = _check(ms, [1000, 1001], [5000, 0], [])
    assert got[0]["rounds"] == 1 and got[3]["counts"]["unitigs"] == 2 and got[1] == [0, 0] and got[2] == []


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

SCALED = ["--gfa-max-hang", "300", "--gfa-min-overlap", "1000", "--gfa-fuzz", "300"]


def _cli(args, timeout=600):
    return subprocess.run([CLI] + args, capture_output=True, timeout=timeout)


def _write_fasta(path, fa):
    with open(path, "w") as fh:
        for i in range(len(fa)):
            fh.write(f">read{i}\n{fa.sequence(i)}\n")


def _s_lines(text):
    return [l.split("\t") for l in text.split("\n") if l.startswith("S\t")]


def _lines(stderr, head):
    return [l for l in stderr.split("\n") if l.startswith(head)]


def test_driver_and_tool_write_the_same_cleaned_graphs(tmp_path):
    """The 40 reads at 10 % error of the string graph's driver test."""
    fa = mhap_amd.synth_reads(40, 3000, seed=77, coverage=8.0, error_rate=0.10)
    fasta = str(tmp_path / "reads.fasta")
    _write_fasta(fasta, fa)
    g0, u0, g1, u1, g2, u2 = (tmp_path / n for n in ("zero.gfa", "zero.utg.gfa", "one.gfa", "one.utg.gfa", "two.gfa", "two.utg.gfa"))
    plain = _cli(["-s", fasta])
    r0 = _cli(["-s", fasta, "--realign", "--gfa", str(g0), "--gfa-unitigs", str(u0)] + SCALED)
    r1 = _cli(["-s", fasta, "--realign", "--gfa", str(g1), "--gfa-unitigs", str(u1), "--gfa-clean"] + SCALED)
    r2 = _cli(["-s", fasta, "--realign", "--gfa", str(g2), "--gfa-unitigs", str(u2), "--gfa-tip-reads", "9", "--gfa-bubble-bases", "1", "--gfa-clean-rounds", "1"] + SCALED)
    assert plain.returncode == 0 and r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r1.stderr[-2000:]
    assert b"Cleaned" not in r0.stderr and b"Cleaned" not in r2.stderr and b"--gfa-clean" not in r0.stderr and b"--gfa-tip-reads" not in r0.stderr
    assert g2.read_bytes() == g0.read_bytes() and u2.read_bytes() == u0.read_bytes()    # the values alone change nothing
    e1 = r1.stderr.decode()
    cleaned, totals = _lines(e1, "Cleaned in "), _lines(e1, "Unitigs: ")
    assert len(cleaned) == 1 and len(totals) == 1 and e1.index("String graph of") < e1.index("Cleaned in ") < e1.index("Unitigs: ")
    assert sorted(r1.stdout.split(b"\n")) == sorted(r0.stdout.split(b"\n"))
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tool = [sys.executable, "-m", "mhap_amd.graph", str(tmp_path / "ovl.txt"), fasta, "--max-hang", "300", "--min-overlap", "1000", "--fuzz", "300"]
    tg, tu = tmp_path / "tool.gfa", tmp_path / "tool.utg.gfa"
    p = subprocess.run(tool + ["-o", str(tg), "--unitigs", str(tu), "--clean"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tg.read_bytes() == g1.read_bytes() and tu.read_bytes() == u1.read_bytes()
    assert _lines(p.stderr, "Cleaned in ") == cleaned and _lines(p.stderr, "Unitigs: ") == totals
    print(cleaned[0], "|", totals[0], "|", _lines(r0.stderr.decode(), "Unitigs: ")[0])
    # the cleaned read graph is the uncleaned one less some lines, and what is gone is what the line counts
    before, after = g0.read_text().split("\n"), g1.read_text().split("\n")
    assert set(after) <= set(before)
    counts = [int(x) for x in cleaned[0].replace("(", "").split() if x.isdigit()]
    assert len(before) - len(after) == counts[2] + counts[4] + counts[5]
    alone = tmp_path / "alone.gfa"
    r3 = _cli(["-s", fasta, "--realign", "--gfa", str(alone), "--gfa-clean"] + SCALED)                  # --gfa-clean without --gfa-unitigs
    assert r3.returncode == 0 and alone.read_bytes() == g1.read_bytes() and _lines(r3.stderr.decode(), "Cleaned in ") == cleaned
    assert b"Unitigs: " not in r3.stderr


def test_error_free_reads_still_spell_their_genome_when_cleaned(tmp_path):
    """The 60 error-free reads of the unitig test's genome: cleaned, every unitig still reads as a piece of the genome, tripled, or
    of its reverse complement, and there are no more unitigs than without the flag."""
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    genome = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 60).astype(np.int32), seed=9, error_rate=0.0)
    fasta = str(tmp_path / "reads.fasta")
    _write_fasta(fasta, fa)
    texts = []
    for extra in ([], ["--gfa-clean"]):
        out, utg = tmp_path / f"g{len(extra)}.gfa", tmp_path / f"u{len(extra)}.gfa"
        p = _cli(["-s", fasta, "--realign", "--gfa", str(out), "--gfa-unitigs", str(utg)] + SCALED + extra)
        assert p.returncode == 0, p.stderr[-2000:]
        texts.append(utg.read_text())
    s_lines = _s_lines(texts[1])
    print(f"{len(_s_lines(texts[0]))} unitigs, cleaned {len(s_lines)}, members {[l[4] for l in s_lines]}")
    assert 0 < len(s_lines) <= len(_s_lines(texts[0]))
    fwd, rev = genome * 3, ur.revcomp(genome * 3)
    for l in s_lines:
        seq = l[2].encode()
        assert l[3] == f"LN:i:{len(seq)}" and len(seq) <= len(fwd)
        assert seq in fwd or seq in rev, l[1]


def test_driver_refuses_cleaning_without_gfa(tmp_path):
    fasta = os.path.join(ROOT, "tests", "golden", "small_reads.fasta")
    p = _cli(["-s", fasta, "--realign", "--gfa-clean"], timeout=60)
    assert p.returncode == 1 and p.stdout.count(b"\n") == 1 and b"--gfa-clean" in p.stdout and b"--gfa too" in p.stdout
