"""The unitig-consensus reference (tests/unitig_consensus_ref.py) against an example small enough to check by eye, the flag validation
of `python -m mhap_amd.graph` and the GFA writer with consensus.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import string_graph_ref as sg
import unitig_consensus_ref as ucr
import unitig_ref as ur

from mhap_amd import api, graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
GOLD = os.path.join(ROOT, "tests", "golden")

# A genome of 100 bases without two equal neighbours, so that every gap has one place.  Three members R1 = G[0:50), R2 = G[25:75),
# R3 = G[50:100) and two reads contained in R1: C1 = G[20:48), C2 = G[22:49).  R2, which spells the draft over [25, 50), is stored with
# three errors: G[30] substituted, G[36:38) missing, one base extra after G[42].  R1, C1 and C2 outvote it there: depth 4 = min_cov.
def draw_genome(n, seed):
    rng, out = np.random.default_rng(seed), []
    for _ in range(n):
        out.append(int(rng.choice([c for c in b"ACGT" if not out or c != out[-1]])))
    return bytes(out)


def other(*cs):
    return next(c for c in b"ACGT" if c not in cs)


G = draw_genome(100, 5)
R2_ERR = G[25:30] + bytes([other(G[29], G[30], G[31])]) + G[31:36] + G[38:43] + bytes([other(G[42], G[43])]) + G[43:75]
READS = [G[0:50], R2_ERR, G[50:100], G[20:48], G[22:49]]
IDS = [1, 2, 3, 4, 5]
LENGTHS = [len(r) for r in READS]
PARAMS = dict(max_hang=5, int_frac_permille=800, min_ovlp=10, fuzz=5)


def hand_records():
    return np.concatenate([
        sg.record(1, 2, 25, 49, 50, 0, 23, 49, 0),      # R1[25, 50) on R2[0, 24): dovetail, the arc R1 -> R2 of length 25
        sg.record(2, 3, 24, 48, 49, 0, 24, 50, 0),      # R2[24, 49) on R3[0, 25): dovetail, the arc R2 -> R3 of length 24
        sg.record(4, 1, 0, 27, 28, 20, 47, 50, 0),      # C1 whole on R1[20, 48): the `from` read is contained
        sg.record(1, 5, 22, 48, 50, 0, 26, 27, 0),      # R1[22, 49) on C2 whole: the `to` read is contained
    ])


def hand_run(**kw):
    g = ur.graph_of(IDS, LENGTHS, hand_records(), **PARAMS)
    u = ur.of_graph(g)
    offsets = np.concatenate([[0], np.cumsum(LENGTHS)])[:5]
    drafts = u.sequences(b"".join(READS), offsets, LENGTHS)
    return u, drafts, ucr.consensus(IDS, LENGTHS, READS, hand_records(), u.tables(), drafts, sg.Params(**PARAMS), band=5, **kw)


def test_genome_has_no_equal_neighbours():
    assert len(G) == 100 and all(G[i] != G[i + 1] for i in range(99)) and LENGTHS == [50, 49, 50, 28, 27]


def test_hand_worked_example():
    u, drafts, res = hand_run()
    assert u.vertex == [0, 2, 4] and u.offset == [0, 25, 49] and u.unitig_len == [99]
    assert drafts == [G[0:25] + R2_ERR[:24] + G[50:100]]
    # members at their offsets; C1 at (20 + 48 - 28) / 2 = 20 and C2 at (22 + 49 - 27) / 2 = 22 through R1, forward
    assert res.placements.tolist() == [[0, 0, 0, 0, 1], [0, 0, 25, 0, 1], [0, 0, 49, 0, 1], [0, 0, 20, 1, 1], [0, 0, 22, 1, 1]]
    assert res.seqs == [G]
    # depth 4 holds over G[25:48): 23 genome bases, 2 of them missing from the draft and 1 draft base extra: 22 draft positions
    assert res.stats.tolist() == [[99, 100, 1, 1, 2, 99 - 22]]
    assert res.counts == dict(members=3, placed_by_record=2, unplaced=0, aligned=5, no_alignment=0, bases_in=99, bases_out=100,
                              substitutions=1, deletions=1, insertions=2, low=77)
    # the map: unchanged up to the missing bases, + 2 behind them, + 1 behind the extra base
    m = res.maps[0]
    assert m[:36].tolist() == list(range(36)) and m[36] == 38 and m[49] == 50 and m[98] == 99
    assert int(res.votes[0][30, :4].sum()) == 4 and res.votes[0][:, 22:].sum() == 0


def test_min_cov_above_the_depth_changes_nothing():
    _, drafts, res = hand_run(min_cov=5)
    assert res.seqs == drafts and res.stats.tolist() == [[99, 99, 0, 0, 0, 99]]


def test_guard_names_the_tile():
    with pytest.raises(ucr.Refused, match="unitig 0 tile 0 is met by 5 reads, more than 4"):
        hand_run(tile_cap=4)
    hand_run(tile_cap=5)


def test_a_member_is_never_placed_from_a_record_and_order_does_not_matter():
    u, drafts, res = hand_run()
    recs = hand_records()
    again = ucr.place(IDS, LENGTHS, np.concatenate([recs[::-1], recs]), u.tables(), sg.Params(**PARAMS))
    assert again[:, :4].tolist() == res.placements[:, :4].tolist()
    # without its record C2 is unplaced
    some = ucr.place(IDS, LENGTHS, recs[:3], u.tables(), sg.Params(**PARAMS))
    assert some[4].tolist() == [-1, 0, 0, 2, 0]


def test_gfa_with_consensus():
    u, _, res = hand_run()
    text = api.format_consensus_gfa(IDS, u.tables(), res.seqs, res.maps)
    assert text == ucr.gfa(IDS, u.tables(), res.seqs, res.maps)
    assert text.splitlines() == ["H\tVN:Z:1.0", f"S\tutg000001l\t{G.decode()}\tLN:i:100\tnr:i:3", "a\tutg000001l\t0\t1:1-25\t+\t25",
                                 "a\tutg000001l\t25\t2:1-24\t+\t24", "a\tutg000001l\t50\t3:1-50\t+\t50"]
    assert api.consensus_counts_line([res.counts[k] for k in api.CONSENSUS_COUNTS]) == (
        "Consensus: 3 members, 2 reads placed by an overlap, 0 unplaced; 5 aligned, 0 without alignment; 99 bases in, 100 out: "
        "1 substitutions, 1 deletions, 2 insertions, 77 low positions")
    assert api.CONSENSUS_COUNTS == ucr.COUNT_NAMES and api.CONSENSUS_TILE == ucr.TILE


@pytest.mark.parametrize("argv", [["--consensus"], ["--consensus-fasta", "c.fa", "--unitigs", "u.gfa"], ["--consensus-min-cov", "3", "--unitigs", "u.gfa"],
                                  ["--consensus", "--unitigs", "u.gfa", "--consensus-min-cov", "0"]])
def test_tool_refuses_flags(argv, capsys):
    with pytest.raises(SystemExit) as e:
        graph.main(["overlaps.txt", "reads.fasta"] + argv)
    assert e.value.code == 2 and "--consensus" in capsys.readouterr().err


def test_consensus_fasta_text():
    assert graph.consensus_fasta([b"ACGT", b"GG"], [0, 1]) == ">utg000001l\nACGT\n>utg000002c\nGG\n"


@pytest.mark.parametrize("flags,word", [(["--gfa", "g.gfa", "--gfa-consensus"], "--gfa-unitigs too"),
                                        (["--gfa", "g.gfa", "--gfa-unitigs", "u.gfa", "--gfa-consensus-fasta", "c.fa"], "--gfa-consensus too"),
                                        (["--gfa", "g.gfa", "--gfa-unitigs", "u.gfa", "--gfa-consensus-min-cov", "3"], "--gfa-consensus too"),
                                        (["--gfa", "g.gfa", "--gfa-unitigs", "u.gfa", "--gfa-consensus", "--gfa-consensus-min-cov", "0"], ">=1")])
def test_driver_refuses_flags(tmp_path, flags, word):
    p = subprocess.run([CLI, "-s", os.path.join(GOLD, "small_reads.fasta"), "--realign"] + flags, capture_output=True, timeout=60, cwd=tmp_path)
    out = p.stdout.decode()
    assert p.returncode == 1 and out.count("\n") == 1 and "--gfa-consensus" in out and word in out, (out, p.stderr[-500:])
    assert not (tmp_path / "g.gfa").exists()


def test_both_tools_list_the_flags_and_the_header_has_the_section():
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and all(f"\t{n}," in h.stdout for n in ("--gfa-consensus", "--gfa-consensus-fasta", "--gfa-consensus-min-cov"))
    with open(os.path.join(ROOT, "include", "mhap_hip.h")) as fh:
        text = fh.read()
    assert f"#define MHAP_CONSENSUS_COUNTS {len(ucr.COUNT_NAMES)}\n" in text and "unitig consensus" in text
    api.load_library()                                                       # every new entry point resolves
