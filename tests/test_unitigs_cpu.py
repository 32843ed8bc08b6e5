"""The unitig contract on the CPU (tests/unitig_ref.py, written from the "unitigs" part of the string-graph section of
include/mhap_hip.h): the spelled unitigs of planted layouts against the genome, the twin symmetry of next, the link ends, hand-made
graphs with their expected tables written out, the complement table, the GFA text and mhap_format_gfa_unitig_link, and the driver's
refusal.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import string_graph_ref as sg  # noqa: E402
import unitig_ref as ur  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("seed", [2, 3, 5])
def test_planted_layout_spells_the_genome(seed):
    """Error-free reads whose alignments are their whole shared intervals: every unitig is the genome between its leftmost start and
    its rightmost end, or the reverse complement of that."""
    ids, lengths, reads, recs = sg.layout(seed, jitter=0)
    genome, bases, offsets = ur.plant(reads, seed, 120000)
    g = ur.graph_of(ids, lengths, recs)
    u = ur.of_graph(g)
    seqs = u.sequences(bases, offsets, lengths)
    assert 1 <= u.counts["unitigs"] <= 2 and 65 <= u.counts["members"] <= 68 and 128 <= g.counts["final"] <= 134
    assert max(u.unitig_start[k + 1] - u.unitig_start[k] for k in range(len(seqs))) >= 65
    for k, s in enumerate(seqs):
        members = [u.vertex[m] >> 1 for m in range(u.unitig_start[k], u.unitig_start[k + 1])]
        lo, hi = min(reads[r][0] for r in members), max(reads[r][1] for r in members)
        assert s in (genome[lo:hi], ur.revcomp(genome[lo:hi])), k
    assert set(u.vertex).isdisjoint({v ^ 1 for v in u.vertex})
    assert sorted(v >> 1 for v in u.vertex) == [r for r in range(len(ids)) if not g.contained[r]]


@pytest.mark.parametrize("seed", [2, 3, 5])
def test_next_is_twin_symmetric_and_links_join_ends(seed):
    """With four in ten overlaps missing the layouts keep forks: next(v) = w <=> next(w ^ 1) = v ^ 1, prev inverts next, and every link
    leaves a tail and enters a head (the restatement asserts the last while it builds the rows)."""
    ids, lengths, _, recs = sg.layout(seed, jitter=300)
    g = ur.graph_of(ids, lengths, recs[np.random.default_rng(len(recs)).random(len(recs)) < 0.6])
    u = ur.of_graph(g)
    assert u.next and len(u.links) > 100
    for v, w in u.next.items():
        assert u.next[w ^ 1] == v ^ 1 and u.prev[w] == v
    heads = {u.vertex[u.unitig_start[k]] for k in range(len(u.unitig_len))}
    tails = {u.vertex[u.unitig_start[k + 1] - 1] for k in range(len(u.unitig_len))}
    for fu, fo, tu, to, ol, arc in u.links:
        a, b = g.rows[arc][0], g.rows[arc][1]
        assert g.rows[arc][6] and ol == g.rows[arc][3]
        assert (a in tails) if not fo else (a ^ 1 in heads)
        assert (b in heads) if not to else (b ^ 1 in tails)
    assert u.counts["joined_arcs"] + u.counts["links"] == g.counts["final"]
    assert u.counts["joined_arcs"] == 2 * (u.counts["members"] - u.counts["unitigs"] + u.counts["circular"])


def _tables(u):
    return (u.unitig_start, u.unitig_len, u.circular, u.vertex, u.offset, u.span, u.links)


def test_forks_by_hand():
    """1 -> 2 and 1 -> 3 fork, 2 -> 4, 3 -> 5 (reverse) and 6 -> 1: the chain 6, 1 is kept as its twin (vertices 1, 11), and both
    orientations stand on the link ends."""
    ids, lengths, recs = ur.forks()
    u = ur.of_graph(ur.graph_of(ids, lengths, recs))
    assert _tables(u) == ([0, 2, 4, 6], [22500, 22000, 22000], [0, 0, 0], [1, 11, 2, 6, 4, 9], [0, 2500, 0, 2000, 0, 2000],
                          [2500, 20000, 2000, 20000, 2000, 20000],
                          [[0, 1, 1, 0, 17000, 0], [0, 1, 2, 0, 15000, 1], [1, 1, 0, 0, 17000, 4], [2, 1, 0, 0, 15000, 6]])
    assert u.counts == dict(unitigs=3, circular=0, members=6, joined_arcs=6, links=4, longest_bases=22500, total_bases=66500)
    seqs = [b"AC", b"", b"G"]
    assert u.gfa(ids, seqs) == ("H\tVN:Z:1.0\n"
                                "S\tutg000001l\tAC\tLN:i:22500\tnr:i:2\n" "a\tutg000001l\t0\t1:1-2500\t-\t2500\n" "a\tutg000001l\t2500\t6:1-20000\t-\t20000\n"
                                "S\tutg000002l\t\tLN:i:22000\tnr:i:2\n" "a\tutg000002l\t0\t2:1-2000\t+\t2000\n" "a\tutg000002l\t2000\t4:1-20000\t+\t20000\n"
                                "S\tutg000003l\tG\tLN:i:22000\tnr:i:2\n" "a\tutg000003l\t0\t3:1-2000\t+\t2000\n" "a\tutg000003l\t2000\t5:1-20000\t-\t20000\n"
                                "L\tutg000001l\t-\tutg000002l\t+\t17000M\n" "L\tutg000001l\t-\tutg000003l\t+\t15000M\n"
                                "L\tutg000002l\t-\tutg000001l\t+\t17000M\n" "L\tutg000003l\t-\tutg000001l\t+\t15000M\n")


def test_in_degree_two_by_hand():
    """1 -> 3 and 2 -> 3, then 3 -> 4: reads 1 and 2 are unitigs of their own, 3 and 4 chain, and the twin of that chain links back."""
    recs = np.concatenate([sg.dove(1, 3, 3000), sg.dove(2, 3, 4000), sg.dove(3, 4, 2000)])
    u = ur.of_graph(ur.graph_of([1, 2, 3, 4], [20000] * 4, recs))
    assert _tables(u) == ([0, 1, 2, 4], [20000, 20000, 22000], [0, 0, 0], [0, 2, 4, 6], [0, 0, 0, 2000], [20000, 20000, 2000, 20000],
                          [[0, 0, 2, 0, 17000, 0], [1, 0, 2, 0, 16000, 1], [2, 1, 0, 1, 17000, 3], [2, 1, 1, 1, 16000, 4]])
    assert u.counts == dict(unitigs=3, circular=0, members=4, joined_arcs=2, links=4, longest_bases=22000, total_bases=62000)


def test_chain_cycle_lone_empty_and_contained_reads_by_hand():
    """One table of reads: 10 -> 11 -> 12 chain; 20 -> 21 -> 22 -> 20 is a cycle whose smallest vertex belongs to 22, the first of the
    three in the table; 30 is named by no record, 31 is empty; 41 is contained in 40 and is in no unitig."""
    ids = [22, 10, 11, 12, 20, 21, 30, 31, 40, 41]
    lengths = [20000, 20000, 20000, 20000, 20000, 20000, 5000, 0, 20000, 9000]
    recs = np.concatenate([sg.dove(10, 11, 4000), sg.dove(12, 11, 6000, rc=1), sg.dove(20, 21, 1000), sg.dove(21, 22, 2000), sg.dove(22, 20, 3000),
                           sg.record(41, 40, 0, 8999, 9000, 500, 9499, 20000, 0)])
    g = ur.graph_of(ids, lengths, recs)
    assert g.contained == [0] * 9 + [1]
    u = ur.of_graph(g)
    # the cycle starts at vertex 0 (read 22) and goes on to 20 (vertex 8) and 21 (vertex 10); the chain 10 + 11 + 12 - has the head 2 < 7 ^ 1
    assert _tables(u) == ([0, 3, 6, 7, 8, 9], [6000, 30000, 5000, 0, 20000], [1, 0, 0, 0, 0], [0, 8, 10, 2, 4, 7, 12, 14, 16],
                          [0, 3000, 4000, 0, 4000, 10000, 0, 0, 0], [3000, 1000, 2000, 4000, 6000, 20000, 5000, 0, 20000], [])
    assert u.counts == dict(unitigs=5, circular=1, members=9, joined_arcs=10, links=0, longest_bases=30000, total_bases=61000)
    bases, offsets = ur.random_bases(lengths, 4, pad=1)
    seqs = u.sequences(bases, offsets, lengths)
    read = lambda r: bytes(bases[offsets[r]:offsets[r] + lengths[r]])
    assert seqs[0] == read(0)[:3000] + read(4)[:1000] + read(5)[:2000]
    assert seqs[1] == read(1)[:4000] + read(2)[:6000] + ur.revcomp(read(3)) and seqs[2] == read(6) and seqs[3] == b""
    text = u.gfa(ids, seqs)
    assert text.count("\n") == 1 + 5 + 9 and "S\tutg000001c\t" in text and "a\tutg000002l\t10000\t12:1-20000\t-\t20000\n" in text
    assert "S\tutg000004l\t\tLN:i:0\tnr:i:1\na\tutg000004l\t0\t31:1-0\t+\t0\n" in text and "\t41:" not in text


@pytest.mark.parametrize("first", [0, 1, 2])
def test_cycle_starts_at_its_smallest_vertex(first):
    ids = [1, 2, 3]
    order = ids[first:] + ids[:first]
    u = ur.of_graph(ur.graph_of(ids, [20000] * 3, ur.cycle(order, 9)))
    assert u.vertex == [0, 2, 4] and u.circular == [1] and u.links == [] and u.counts["joined_arcs"] == 6
    back = ur.of_graph(ur.graph_of(ids, [20000] * 3, ur.cycle(order[::-1], 9)))
    assert back.vertex == [0, 4, 2] and sum(back.span) == back.unitig_len[0]


def test_no_reads_and_chain_fabricator():
    u = ur.of_graph(ur.graph_of([], [], np.zeros(0, sg.RECORD_DTYPE)))
    assert _tables(u) == ([0], [], [], [], [], [], []) and u.gfa([], []) == "H\tVN:Z:1.0\n" and not any(u.counts.values())
    for n in (1, 2, 5, 64):
        ids, lengths, reads, recs = ur.chain(n, n)
        genome, bases, offsets = ur.plant(reads, n)
        u = ur.of_graph(ur.graph_of(ids, lengths, recs))
        assert u.counts["unitigs"] == 1 and u.counts["members"] == n and u.counts["links"] == 0
        assert u.sequences(bases, offsets, lengths)[0] in (genome, ur.revcomp(genome))
    ids, lengths, _, _ = ur.chain(3, 1)
    rc_chain = np.concatenate([sg.dove(1, 2, 3000, rc=1), sg.dove(2, 3, 3000, rc=1)])     # the arcs enter the reverse vertex: no chain of three
    assert ur.of_graph(ur.graph_of(ids, [20000] * 3, rc_chain)).counts["unitigs"] == 3


def test_complement_table():
    assert ur.revcomp(b"ACGTNacgtnRYKMBDHVSWxX-*") == b"*-XXWSBDHVKMRYNACGTNACGT"
    assert all(ur.RC_TABLE[c] == c for c in range(256) if not chr(c).isalpha())


def test_link_line_counts_line_and_names():
    import mhap_amd
    lib = mhap_amd.load_library()
    row = np.array([0, 1, 11, 0, 17000, 5], np.int32)
    assert mhap_amd.format_gfa_unitig_link(row) == "L\tutg000001l\t-\tutg000012l\t+\t17000M"
    buf = C.create_string_buffer(8)
    n = lib.mhap_format_gfa_unitig_link(row.ctypes.data_as(C.c_void_p), buf, C.c_size_t(8))
    assert n == len("L\tutg000001l\t-\tutg000012l\t+\t17000M") and buf.value == b"L\tutg00"
    assert lib.mhap_format_gfa_unitig_link(None, buf, C.c_size_t(8)) == -1
    assert lib.mhap_format_gfa_unitig_link(row.ctypes.data_as(C.c_void_p), None, C.c_size_t(8)) == -1
    assert tuple(mhap_amd.api.UNITIG_COUNTS) == ur.COUNT_NAMES
    assert mhap_amd.api.unitig_counts_line(range(1, 8)) == "Unitigs: 1 unitigs (2 circular) of 3 reads, 4 joined arcs, 5 links; longest 6 bases, 7 bases in all"
    ids, lengths, recs = ur.forks()
    u = ur.of_graph(ur.graph_of(ids, lengths, recs))
    seqs = [b"A" * n for n in u.unitig_len]
    assert mhap_amd.format_unitig_gfa(ids, u.tables(), seqs) == u.gfa(ids, seqs)


def test_driver_refuses_unitigs_without_gfa_and_lists_the_flag(tmp_path):
    p = subprocess.run([CLI, "-s", os.path.join(GOLD, "small_reads.fasta"), "--realign", "--gfa-unitigs", str(tmp_path / "u.gfa")], capture_output=True, timeout=60)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--gfa-unitigs" in out and "--gfa too" in out, (out, p.stderr[-500:])
    assert not (tmp_path / "u.gfa").exists()
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "\t--gfa-unitigs," in h.stdout
    t = subprocess.run([sys.executable, "-m", "mhap_amd.graph", "--help"], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert t.returncode == 0 and "--unitigs" in t.stdout
