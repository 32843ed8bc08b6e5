"""The unitigs on the GPU (mhap_graph_unitigs / _copy_* / _spell, unitig_kernels.hip) against their CPU restatement
(tests/unitig_ref.py over tests/string_graph_ref.py): every array, the counts, the link rows, the sequences and the GFA text, exactly;
then `mhap-hip --realign --gfa --gfa-unitigs` against the genome its reads were drawn from and against `python -m mhap_amd.graph
--unitigs`.  The graphs are fabricated from reads placed on a line and from hand-made dovetails."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import string_graph_ref as sg  # noqa: E402
import unitig_ref as ur  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
CHUNK = 4096          # MHAP_SPELL_CHUNK of include/mhap_hip.h
SENTINEL = 0x01       # a byte no read holds and the complement table leaves alone


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def test_the_chunk_is_the_headers():
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        assert f"#define MHAP_SPELL_CHUNK {CHUNK}\n" in fh.read()


def _fasta(ids, lengths, bases, offsets):
    return mhap_amd.FastaData(bases, offsets, lengths, ids)


def _compare(gs, ref, bases, offsets):
    """The session's unitigs (its finish has run) against those of the finished restatement `ref`, spelled over `bases`: returns
    (tables, sequences, gfa text)."""
    want = ur.of_graph(ref)
    got, exp = gs.unitigs(), want.tables()
    for k in ("unitig_start", "unitig_len", "circular", "vertex", "offset", "span", "links"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (k, got[k].shape, exp[k].shape)
        if not np.array_equal(got[k], exp[k]):
            bad = np.flatnonzero((got[k] != exp[k]).reshape(len(exp[k]), -1).any(axis=1))
            assert False, (k, bad[:5], got[k][bad[0]], exp[k][bad[0]])
    assert got["counts"] == exp["counts"]
    assert gs.unitigs_info() == (len(want.unitig_len), len(want.vertex), len(want.links), sum(want.unitig_len))
    out = np.full(sum(want.unitig_len), SENTINEL, np.uint8)
    gs.spell_into(bases, offsets, out)
    assert not (out == SENTINEL).any()
    want_seqs = want.sequences(bases, offsets, ref.lengths)
    assert out.tobytes() == b"".join(want_seqs)
    fasta = _fasta(ref.ids, ref.lengths, bases, offsets)
    seqs = gs.unitig_sequences(fasta)
    assert seqs == want_seqs
    text = gs.unitig_gfa(fasta)
    assert text == want.gfa(ref.ids, want_seqs)
    return got, seqs, text


def _same(a, b):
    assert all((a[0][k] == b[0][k]).all() for k in a[0] if k != "counts") and a[0]["counts"] == b[0]["counts"] and a[1] == b[1] and a[2] == b[2]


def _check(ms, ids, lengths, adds, bases=None, offsets=None, **p):
    """One session and one restatement given the same adds, finished once, compacted and compared; bases are drawn when none come."""
    if bases is None:
        bases, offsets = ur.random_bases(lengths, len(ids) + 7, pad=1)
    ref = sg.Graph(ids, lengths, sg.Params(**p))
    with mhap_amd.GraphSession(ids, lengths, handle=ms, **p) as gs:
        for recs in adds:
            gs.add(recs)
            ref.add(recs)
        gs.finish()
        ref.finish()
        return _compare(gs, ref, bases, offsets)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025])
def test_chain_of_n_reads(ms, n):
    """Every boundary of the doubling rounds, the wave and the scan tile; the reads carry the bases of a drawn line, so the one unitig
    is that line or its reverse complement."""
    ids, lengths, reads, recs = ur.chain(n, 100 + n)
    genome, bases, offsets = ur.plant(reads, n)
    got, seqs, _ = _check(ms, ids, lengths, [recs], bases, offsets)
    assert got["counts"]["unitigs"] == 1 and got["counts"]["members"] == n and got["counts"]["joined_arcs"] == 2 * (n - 1)
    assert seqs[0] in (genome, ur.revcomp(genome))


@pytest.mark.parametrize("n", [2, 3, 64, 65, 1025])
def test_cycle_of_n_reads_with_its_smallest_vertex_anywhere(ms, n):
    """The table of reads is permuted, so the cycle's smallest vertex lies at another place of the cycle each time, and the cycle is
    walked in both directions of the table."""
    rng = np.random.default_rng(n)
    order = list(range(1, n + 1))
    for trial in range(3):
        ids = [int(x) for x in rng.permutation(order)] if trial else order
        walk = order if trial < 2 else order[::-1]
        got, _, _ = _check(ms, ids, [20000] * n, [ur.cycle(walk, n + trial)])
        assert got["counts"]["circular"] == 1 and got["counts"]["unitigs"] == 1 and got["counts"]["members"] == n and got["vertex"][0] == 0
        assert got["counts"]["joined_arcs"] == 2 * n and not len(got["links"])


def test_cycles_and_chains_in_one_graph(ms):
    """Two cycles, three chains and two lone reads, their reads interleaved in the table."""
    rng = np.random.default_rng(8)
    ids = [int(x) for x in rng.permutation(np.arange(1, 231))]
    groups = [ids[0:65], ids[65:68], ids[68:133], ids[133:198], ids[198:228]]
    recs = [ur.cycle(groups[0], 1), ur.cycle(groups[1], 2)]
    recs += [np.concatenate([sg.dove(g[i], g[i + 1], 2000 + 10 * i) for i in range(len(g) - 1)]) for g in groups[2:]]
    recs = np.concatenate(recs)
    got, _, _ = _check(ms, sorted(ids), [20000] * 230, [recs[rng.permutation(len(recs))]])
    assert got["counts"]["circular"] == 2 and got["counts"]["unitigs"] == 7 and got["counts"]["members"] == 230


def test_forks_and_in_degree_two(ms):
    ids, lengths, recs = ur.forks()
    got, _, text = _check(ms, ids, lengths, [recs])
    assert got["links"].tolist() == [[0, 1, 1, 0, 17000, 0], [0, 1, 2, 0, 15000, 1], [1, 1, 0, 0, 17000, 4], [2, 1, 0, 0, 15000, 6]]
    assert got["vertex"].tolist() == [1, 11, 2, 6, 4, 9] and text.endswith("L\tutg000003l\t-\tutg000001l\t+\t15000M\n")
    recs = np.concatenate([sg.dove(1, 3, 3000), sg.dove(2, 3, 4000), sg.dove(3, 4, 2000)])
    got, _, _ = _check(ms, [1, 2, 3, 4], [20000] * 4, [recs])
    assert got["links"].tolist() == [[0, 0, 2, 0, 17000, 0], [1, 0, 2, 0, 16000, 1], [2, 1, 0, 1, 17000, 3], [2, 1, 1, 1, 16000, 4]]


def test_lone_empty_and_contained_reads(ms):
    ids = [22, 10, 11, 12, 20, 21, 30, 31, 40, 41]
    lengths = [20000, 20000, 20000, 20000, 20000, 20000, 5000, 0, 20000, 9000]
    recs = np.concatenate([sg.dove(10, 11, 4000), sg.dove(12, 11, 6000, rc=1), sg.dove(20, 21, 1000), sg.dove(21, 22, 2000), sg.dove(22, 20, 3000),
                           sg.record(41, 40, 0, 8999, 9000, 500, 9499, 20000, 0)])
    got, seqs, text = _check(ms, ids, lengths, [recs])
    assert got["vertex"].tolist() == [0, 8, 10, 2, 4, 7, 12, 14, 16] and got["circular"].tolist() == [1, 0, 0, 0, 0]
    assert 18 not in got["vertex"] and 19 not in got["vertex"] and seqs[3] == b"" and "\t41:" not in text
    got, _, _ = _check(ms, [1000, 1001], [5000, 0], [])                              # reads only, no record at all
    assert got["counts"] == dict(unitigs=2, circular=0, members=2, joined_arcs=0, links=0, longest_bases=5000, total_bases=5000)
    got, _, _ = _check(ms, [1001], [0], [])                                          # nothing to spell
    assert got["counts"]["total_bases"] == 0 and got["counts"]["unitigs"] == 1


def test_no_reads_at_all(ms):
    got, seqs, text = _check(ms, [], [], [], np.zeros(0, np.uint8), np.zeros(0, np.int64))
    assert not any(got["counts"].values()) and seqs == [] and text == "H\tVN:Z:1.0\n" and got["unitig_start"].tolist() == [0]


def test_calls_out_of_order_are_refused_and_unitigs_follow_the_last_finish(ms):
    """unitigs before any finish; copy and spell before unitigs and after a later finish; records after the finish; then
    finish -> unitigs -> add more -> finish -> unitigs, each compared."""
    ids, lengths, reads, recs = ur.chain(40, 3)
    _, bases, offsets = ur.plant(reads, 3)
    ref = sg.Graph(ids, lengths)
    with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
        with pytest.raises(mhap_amd.MhapError, match="no mhap_graph_finish has completed"):
            gs.unitigs()
        assert gs.unitigs_info()[0] == -1
        gs.add(recs[:20])
        ref.add(recs[:20])
        gs.finish()
        ref.finish()
        with pytest.raises(mhap_amd.MhapError, match="no mhap_graph_unitigs has completed"):
            gs.spell_into(bases, offsets, np.zeros(10, np.uint8))
        first = _compare(gs, ref, bases, offsets)
        assert first[0]["counts"]["unitigs"] == 20                                   # a chain of 21 and 19 lone reads
        gs.add(recs[20:])
        ref.add(recs[20:])
        with pytest.raises(mhap_amd.MhapError, match="records were added after the last mhap_graph_finish"):
            gs.unitigs()
        gs.finish()
        ref.finish()
        assert gs.unitigs_info()[0] == -1
        with pytest.raises(mhap_amd.MhapError, match="no mhap_graph_unitigs has completed"):
            gs._ms._chk(gs._lib.mhap_graph_copy_links(gs._s, None))
        second = _compare(gs, ref, bases, offsets)
        assert second[0]["counts"]["unitigs"] == 1 and second[0]["counts"]["members"] == 40
        again = _compare(gs, ref, bases, offsets)                                    # the sequence twice in one session: the same bytes
        _same(second, again)
        short = bases[:-1]
        with pytest.raises(mhap_amd.MhapError, match=r"read 39 is \[\d+, \d+\) of \d+ bases"):
            gs.spell_into(short, offsets, np.zeros(second[0]["counts"]["total_bases"], np.uint8))


@pytest.fixture(scope="module", params=[2, 3, 5])
def layout(request):
    ids, lengths, reads, recs = sg.layout(request.param, jitter=300)
    _, bases, offsets = ur.plant(reads, request.param, 120000)
    return ids, lengths, recs, bases, offsets


@pytest.mark.parametrize("thinned", [False, True])
def test_layout_in_one_add_three_adds_and_shuffled(ms, layout, thinned):
    """The whole layout compacts to one or two unitigs without links; with four in ten of its overlaps missing, transitive arcs stay,
    and it falls into dozens of unitigs with forks and more than a hundred links."""
    ids, lengths, recs, bases, offsets = layout
    if thinned:
        recs = recs[np.random.default_rng(len(recs)).random(len(recs)) < 0.6]
    one = _check(ms, ids, lengths, [recs], bases, offsets)
    print(one[0]["counts"])
    assert one[0]["counts"]["joined_arcs"] > 0 and (one[0]["counts"]["links"] > 100) == thinned
    third = len(recs) // 3
    _same(one, _check(ms, ids, lengths, [recs[:third], recs[third:third + 1], recs[third + 1:]], bases, offsets))
    _same(one, _check(ms, ids, lengths, [recs[np.random.default_rng(1).permutation(len(recs))]], bases, offsets))


def test_layout_of_1100_reads_in_one_add_and_shuffled_over_three(ms):
    """2 200 vertices and a few unitigs of hundreds of reads whose members lie in all three tiles of the scans."""
    ids, lengths, reads, recs = sg.layout(2, n_reads=1100, genome=880000, jitter=300)
    _, bases, offsets = ur.plant(reads, 2, 880000)
    one = _check(ms, ids, lengths, [recs], bases, offsets)
    print(one[0]["counts"])
    assert 2 * len(ids) > 2048 and (one[0]["vertex"] >= 2048).any() and (np.diff(one[0]["unitig_start"]) > 128).any()
    perm = np.random.default_rng(12).permutation(len(recs))
    parts = [perm[:len(perm) // 3], perm[len(perm) // 3:len(perm) // 3 + 1], perm[len(perm) // 3 + 1:]]
    _same(one, _check(ms, ids, lengths, [recs[part] for part in parts], bases, offsets))


def test_unitigs_and_links_that_begin_in_every_scan_tile(ms):
    """1 100 reads, most of them lone, so that unitigs begin in all three tiles of the three numbering scans and the carries are not
    0; chains and a fork low, in the middle and high in the table, so that link rows come from arcs of every tile too."""
    ids, recs = list(range(1, 1101)), []
    for lo in (5, 600, 1050):
        recs += [sg.dove(i, i + 1, 2000 + i) for i in range(lo, lo + 12)]
        recs += [sg.dove(lo + 20, lo + 21, 3000), sg.dove(lo + 20, lo + 22, 5000)]
    got, _, _ = _check(ms, ids, [20000] * 1100, [np.concatenate(recs)])
    heads = got["vertex"][got["unitig_start"][:-1]]
    for lo, hi in ((0, 1024), (1024, 2048), (2048, 2200)):
        assert ((heads >= lo) & (heads < hi)).sum() > 10
    assert got["counts"]["links"] == 12 and got["counts"]["unitigs"] == 1100 - 3 * 12


SIZES = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1]


def test_spelling_at_every_size_and_strand(ms):
    """For every size and either strand a chain a, b, c placed on a line: a's span is the size, and c is a whole read of that size (not
    for size 1: such a read has no arc); then a lone read of every size.  The bases hold N, lower case, other IUPAC letters and bytes
    that are no letters; they begin at an odd offset and the reads' lengths are odd and even, so that sources of every alignment
    meet destinations of every alignment; some 16-byte groups lie in one member and some across two or three."""
    reads, pairs = [], []
    for size in SIZES:
        for f in (0, 1):
            at, k = 10000 * len(reads), len(reads)
            ov = min(size - 1, 10)
            reads += [(at, at + 6000, f), (at + size, at + size + 6000, f)]
            pairs.append((k, k + 1))
            if size > 1:
                reads.append((at + size + 6000 - ov, at + size + 6000 - ov + size, f))
                pairs.append((k + 2, k + 1))
    chained = len(reads)
    reads += [(0, size, 0) for size in SIZES]
    ids = list(range(1, len(reads) + 1))
    lengths = [e - s for s, e, _ in reads]
    recs = np.concatenate([sg.placed(ids[x], ids[y], reads[x], reads[y]) for x, y in pairs])
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"ACGTACGTACGTNnacgtRYKMSWBDHVxX-*", np.uint8)
    bases = alphabet[rng.integers(0, len(alphabet), 1 + sum(lengths))]
    offsets = (1 + np.concatenate([[0], np.cumsum(lengths)])[:len(lengths)]).astype(np.int64)
    got, _, _ = _check(ms, ids, lengths, [recs], bases, offsets, min_ovlp=1, max_hang=0, fuzz=0)
    assert got["counts"]["unitigs"] == 2 * len(SIZES) + len(SIZES) and got["counts"]["members"] == len(reads) and not len(got["links"])
    spans, odd = got["span"].tolist(), (got["vertex"] & 1).tolist()
    for size in SIZES:
        for f in (0, 1):
            assert (size, f) in zip(spans, odd), (size, f)
    assert set(np.asarray(lengths)[got["vertex"][np.flatnonzero(got["vertex"] >= 2 * chained)] >> 1].tolist()) == set(SIZES)


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


def test_error_free_reads_spell_their_genome(tmp_path):
    """60 error-free reads of 2 500 - 3 500 bases from a drawn circular genome of 20 kb: whatever the layout, every unitig must read as
    a piece of the genome (which may be walked round more than once) or of its reverse complement."""
    rng = np.random.default_rng(41)
    codes = rng.integers(0, 4, 20000).astype(np.uint8)
    genome = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
    fa = mhap_amd.synth_reads_from_genome(codes, rng.integers(2500, 3501, 60).astype(np.int32), seed=9, error_rate=0.0)
    fasta = str(tmp_path / "reads.fasta")
    _write_fasta(fasta, fa)
    out, utg = tmp_path / "g.gfa", tmp_path / "u.gfa"
    p = _cli(["-s", fasta, "--realign", "--gfa", str(out), "--gfa-unitigs", str(utg)] + SCALED)
    assert p.returncode == 0, p.stderr[-2000:]
    text = utg.read_text()
    lines = text.split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == "" and all(l[:2] in ("H\t", "S\t", "a\t", "L\t") for l in lines[:-1])
    s_lines = _s_lines(text)
    print(f"{len(s_lines)} unitigs, members {[l[4] for l in s_lines]}")
    assert s_lines and any(int(l[4].split(":")[2]) > 1 for l in s_lines)
    fwd, rev = genome * 3, ur.revcomp(genome * 3)
    for l in s_lines:
        seq = l[2].encode()
        assert l[3] == f"LN:i:{len(seq)}" and len(seq) <= len(fwd)
        assert seq in fwd or seq in rev, l[1]
    totals = [l for l in p.stderr.decode().split("\n") if l.startswith("Unitigs: ")]
    assert len(totals) == 1 and totals[0].startswith(f"Unitigs: {len(s_lines)} unitigs (")


def test_driver_and_tool_write_the_same_unitigs(tmp_path):
    """The 40 reads at 10 % error of the string graph's driver test."""
    fa = mhap_amd.synth_reads(40, 3000, seed=77, coverage=8.0, error_rate=0.10)
    fasta = str(tmp_path / "reads.fasta")
    _write_fasta(fasta, fa)
    plain = _cli(["-s", fasta])
    g0, g1, g2, u1, u2 = (tmp_path / n for n in ("zero.gfa", "one.gfa", "two.gfa", "one.utg.gfa", "two.utg.gfa"))
    r0 = _cli(["-s", fasta, "--realign", "--gfa", str(g0)] + SCALED)
    r1 = _cli(["-s", fasta, "--realign", "--gfa", str(g1), "--gfa-unitigs", str(u1)] + SCALED)
    r2 = _cli(["-s", fasta, "--realign", "--gfa", str(g2), "--gfa-unitigs", str(u2)] + SCALED)
    assert plain.returncode == 0 and r0.returncode == 0 and r1.returncode == 0 and r2.returncode == 0, r1.stderr[-2000:]
    assert g1.read_bytes() == g0.read_bytes() and g2.read_bytes() == g0.read_bytes()            # --gfa's file does not know of --gfa-unitigs
    assert sorted(r1.stdout.split(b"\n")) == sorted(r0.stdout.split(b"\n")) and len(r1.stdout) == len(r0.stdout) > 1000
    assert b"Unitigs: " not in r0.stderr
    text = u1.read_text()
    assert u2.read_text() == text and len(_s_lines(text)) > 0
    totals = [l for l in r1.stderr.decode().split("\n") if l.startswith("Unitigs: ")]
    assert len(totals) == 1
    (tmp_path / "ovl.txt").write_bytes(plain.stdout)
    tool_g, tool_u = tmp_path / "tool.gfa", tmp_path / "tool.utg.gfa"
    p = subprocess.run([sys.executable, "-m", "mhap_amd.graph", str(tmp_path / "ovl.txt"), fasta, "--max-hang", "300", "--min-overlap", "1000",
                        "--fuzz", "300", "-o", str(tool_g), "--unitigs", str(tool_u)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert tool_g.read_bytes() == g0.read_bytes() and tool_u.read_text() == text
    assert totals[0] in p.stderr
