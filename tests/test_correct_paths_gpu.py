"""The vote and call kernels (correct_kernels.hip) on hand-made paths (tests/handmade_paths.py): every kind of column put on purpose
where vote_kernel changes its chunk of 64 runs, its deal of 64 columns, its plane or its launch, and where call_kernel changes its
tile of 256 positions; every counter brought to the cap of 65 535; and the refusal of paths that repeat a code.  As in
test_correct_gpu.py every counter of every read, the bytes, the offsets, the six counts and skipped_views equal the restatement's
(tests/consensus_ref.py); on top of that the session's votes obey the coverage identity, which holds whatever the paths are, and the
tests that can name the expected bytes do.  Every test asserts the precondition that makes it cover what its docstring says."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
import consensus_ref as cref  # noqa: E402
import handmade_paths as hp  # noqa: E402
from align_ref import rc_bytes  # noqa: E402
from test_correct_gpu import _check, _fasta  # noqa: E402

pytestmark = pytest.mark.gpu

OP_I, OP_D, OP_EQ, OP_X = cref.OP_I, cref.OP_D, cref.OP_EQ, cref.OP_X
INS0, DEL, SPAN = cref.INS0, cref.DEL, cref.SPAN


class Pile:
    """Reads and records for one add.  pair() makes two reads of their own for a path; record() names reads that are there already.
    `views` keeps the target interval of every view per read, for the coverage identity."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.reads, self.recs, self.paths, self.views = [], [], [], {}

    def record(self, x, y, s1, s2, fa, fb, runs, to_rc, copies=1):
        """`copies` records of the path `runs` from (fa, fb) over read x (s1) and read y (stored: rc_bytes(s2) when to_rc)."""
        assert self.reads[x] == s1 and self.reads[y] == (rc_bytes(s2) if to_rc else s2)
        rec = hp.record_for(x + 1, y + 1, s1, s2, fa, fb, runs, to_rc)
        ia, ib = hp.target_intervals(rec)
        for _ in range(copies):
            self.recs.append(rec)
            self.paths.append([int(r) for r in runs])
            self.views.setdefault(x, []).append(ia)
            self.views.setdefault(y, []).append(ib)
        return rec

    def pair(self, runs, to_rc, flank_a=(0, 0), flank_b=(0, 0), copies=1, edit=None):
        """Two new reads that fit `runs` (edit(s1, s2) -> (s1, s2) may change bytes afterwards); returns (x, s1, s2), read B being x + 1."""
        s1, s2 = hp.pair_from_runs(self.rng, runs, flank_a, flank_b)
        if edit:
            s1, s2 = edit(bytearray(s1), bytearray(s2))
            s1, s2 = bytes(s1), bytes(s2)
        x = len(self.reads)
        self.reads += [s1, rc_bytes(s2) if to_rc else s2]
        self.record(x, x + 1, s1, s2, flank_a[0], flank_b[0], runs, to_rc, copies)
        return x, s1, s2

    def add(self):
        off = np.concatenate([[0], np.cumsum([len(p) for p in self.paths])]).astype(np.int64)
        ops = np.array([r for p in self.paths for r in p], np.uint32)
        return np.concatenate(self.recs), off, ops

    def check(self, min_cov=4, identity=True):
        """_check of test_correct_gpu.py on one add of everything, then the coverage identity on the session's own votes."""
        seqs, stats, skipped, votes = _check(self.reads, [self.add()], min_cov)
        if identity:
            for r in range(len(self.reads)):
                bad = hp.coverage_identity(votes[r], self.views.get(r, []))
                assert not bad, (r, bad[:5])
        return seqs, stats, skipped, votes


def _ins_slots(row, group, copies=1):
    """The 16 insertion counters of one position against the bytes of the group after it, in the view's order: byte k < 4 has `copies`
    votes in slot k when it is A, C, G or T and leaves the slot empty otherwise; bytes from the fifth on vote nowhere."""
    want = np.zeros(16, np.int64)
    for k, e in enumerate(bytes(group)[:cref.KI]):
        if e in cref.ACGT:
            want[4 * k + cref.ACGT.index(e)] = copies
    assert row[INS0:INS0 + 16].astype(np.int64).tolist() == want.tolist(), (row[INS0:INS0 + 16].tolist(), want.tolist(), bytes(group))


def _first_column(runs, index):
    """(row offset, column offset, path column) at which run `index` begins."""
    i = sum(r >> 4 for r in runs[:index] if r & 15 != OP_D)
    j = sum(r >> 4 for r in runs[:index] if r & 15 != OP_I)
    return i, j, sum(r >> 4 for r in runs[:index])


# ---- B1: the edges of a chunk of 64 runs -------------------------------------------------------------------------------------------

def test_every_kind_of_run_on_the_edges_of_a_chunk_of_runs():
    """vote_kernel takes the runs 64 at a time, carries (ci, cj) from chunk to chunk through __shfl(si, 63) and, for an Ins group,
    reads the neighbouring run runs[nb] from global memory, which is the only access that leaves the chunk: nb = ridx - 1 for a group
    on run 64 or 128, nb = ridx + 1 for one on run 63 or 127 of a reversed view.  Here an I, a D and an X run of 1, 4 and 6 columns
    stand on each of the run indices 62 .. 65, 127 and 128, on both strands, and paths have exactly 1, 3, 63, 65 and 129 runs (the
    last chunk holds 1, 3, 63, 1 and 1 runs).  One add holds all of them."""
    pile = Pile(31)
    where = {}
    for to_rc in (0, 1):
        for kind in "IDX":
            for length in (1, 4, 6):
                for at in (62, 63, 64, 65, 127, 128):
                    total = 129 if at < 127 else 131
                    runs = hp.runs_with(kind, length, at, total, pile.rng)
                    assert len(runs) == total and runs[at] == hp.run(kind, length) and hp.check_canonical(runs)      # the precondition
                    n = len(where)
                    where[to_rc, kind, length, at] = pile.pair(runs, to_rc, (n % 3, n % 2), (n % 2, n % 4)) + (runs,)
        for total, kind, at in ((1, "=", 0), (3, "X", 1), (63, "I", 31), (65, "D", 63), (65, "I", 63), (129, "I", 127), (129, "D", 1)):
            runs = hp.runs_with(kind, 5, at, total, pile.rng)
            assert len(runs) == total
            pile.pair(runs, to_rc, (1, 2), (3, 0))
    assert len(where) == 108 and len(pile.recs) == 108 + 14
    _, _, skipped, votes = pile.check(min_cov=1)
    assert skipped == 0
    # the Ins groups whose neighbouring run lies in another chunk, against the bytes themselves: a D run on index 64 and on 128 in
    # view A (the neighbour is run 63, 127), an I run on index 63 and on 127 in the reversed view B (the neighbour is run 64, 128)
    for at in (64, 128):
        x, s1, s2, runs = where[0, "D", 6, at]
        i, j, _ = _first_column(runs, at)
        fa, fb = int(pile.recs[x // 2][0]["a1"]), int(pile.recs[x // 2][0]["b1"])
        _ins_slots(votes[x][fa + i - 1], s2[fb + j:fb + j + 4])
    for at in (63, 127):
        x, s1, s2, runs = where[1, "I", 6, at]
        i, j, _ = _first_column(runs, at)
        fa, fb = int(pile.recs[x // 2][0]["a1"]), len(s2) - 1 - int(pile.recs[x // 2][0]["b2"])
        _ins_slots(votes[x + 1][len(s2) - 1 - (fb + j)], rc_bytes(s1[fa + i + 2:fa + i + 6]))


# ---- B2: the edges of a deal of 64 columns ------------------------------------------------------------------------------------------

def _deal_paths():
    """(runs, index of the long run): a run of 63, 64, 65 and 200 columns of every kind, beginning at column 3, 63 and 64 of its chunk."""
    out = []
    for n in (63, 64, 65, 200):
        for kind in "XID":
            for pre in (3, 63, 64):
                out.append((hp.cigar(f"{pre}= {n}{kind} 3="), 1))
        for pre in (2, 62, 63):
            out.append((hp.cigar(f"{pre}= 1X {n}= 1X 2="), 2))
    return out


def test_long_runs_on_the_edges_of_a_deal_of_columns():
    """The columns of a chunk are dealt to the lanes 64 at a time and every lane finds its run by a binary search over s_col: a run of
    63, 64, 65 and 200 columns of each kind, beginning at column 3, 63 and 64, on both strands.  An Ins group of 63 to 200 columns
    votes with its first four bytes only, which in the reversed view of a to_rc record are its last four in path order, complemented;
    these are asserted against the bytes themselves."""
    pile = Pile(32)
    cases = []
    for to_rc in (0, 1):
        for runs, at in _deal_paths():
            n, code = runs[at] >> 4, runs[at] & 15
            assert n in (63, 64, 65, 200) and _first_column(runs, at)[2] in (3, 63, 64)                              # the precondition
            x, s1, s2 = pile.pair(runs, to_rc, (2, 1), (1, 2))
            cases.append((x, s1, s2, runs, at, to_rc))
    assert len(cases) == 2 * 48 and {(c[3][c[4]] & 15, c[3][c[4]] >> 4) for c in cases} == {(k, n) for k in (OP_EQ, OP_X, OP_I, OP_D) for n in (63, 64, 65, 200)}
    _, _, skipped, votes = pile.check(min_cov=1)
    assert skipped == 0
    seen = 0
    for x, s1, s2, runs, at, to_rc in cases:
        n, code = runs[at] >> 4, runs[at] & 15
        i, j, _ = _first_column(runs, at)
        i, j = i + 2, j + 1                                          # the flanks
        if code == OP_D:                                             # view A: the group after row i - 1 is s2[j .. j + n)
            _ins_slots(votes[x][i - 1], s2[j:j + 4])
            assert votes[x][:, INS0:].sum() == 4
            seen += 1
        elif code == OP_I and not to_rc:                             # view B: the group after column j - 1 is s1[i .. i + n)
            _ins_slots(votes[x + 1][j - 1], s1[i:i + 4])
            assert votes[x + 1][:, INS0:].sum() == 4
            seen += 1
        elif code == OP_I:                                           # reversed: after the position of column j, the last four backwards
            _ins_slots(votes[x + 1][len(s2) - 1 - j], rc_bytes(s1[i + n - 4:i + n]))
            assert votes[x + 1][:, INS0:].sum() == 4
            seen += 1
    assert seen == 2 * 12 + 12 + 12


# ---- B3: gap runs next to each other ------------------------------------------------------------------------------------------------

def test_gap_runs_next_to_each_other():
    """= I D =, = D I =, = I D I = and = D I D = with 1 to 6 columns in each place, on both strands: paths that the aligner never
    returns (at its costs a gap never follows a gap of the other kind) and that add accepts.  In view A an I D pair is a Del followed
    by an Ins group that belongs to the deleted position, D I an Ins group followed by a Del; the reversed view B turns both round."""
    pile = Pile(33)
    lens = range(1, 7)
    for to_rc in (0, 1):
        for a in lens:
            for b in lens:
                for text in (f"3= {a}I {b}D 3=", f"3= {a}D {b}I 3="):
                    pile.pair(hp.cigar(text), to_rc, (1, 0), (0, 2))
                for c in lens:
                    for text in (f"2= {a}I {b}D {c}I 3=", f"2= {a}D {b}I {c}D 3="):
                        pile.pair(hp.cigar(text), to_rc, (0, 1), (1, 0))
    assert len(pile.recs) == 2 * (72 + 432)
    kinds = {tuple(r & 15 for r in p) for p in pile.paths}
    assert kinds == {(7, 1, 2, 7), (7, 2, 1, 7), (7, 1, 2, 1, 7), (7, 2, 1, 2, 7)}                                    # the precondition
    _, _, skipped, votes = pile.check(min_cov=1)
    assert skipped == 0
    # = 2I 5D 3= from (1, 0): view A deletes rows 4, 5 and the group of five belongs to row 5; view B's group of two belongs to column 2
    q = pile.paths.index(hp.cigar("3= 2I 5D 3="))
    s1, s2 = pile.reads[2 * q], pile.reads[2 * q + 1]
    assert votes[2 * q][4:6, DEL].tolist() == [1, 1]
    _ins_slots(votes[2 * q][5], s2[3:7])
    _ins_slots(votes[2 * q][4], b"")
    _ins_slots(votes[2 * q + 1][2], s1[4:6])
    assert votes[2 * q + 1][3:8, DEL].tolist() == [1] * 5


# ---- B4: bytes that are not A, C, G, T --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("to_rc", [0, 1])
def test_n_bytes_take_their_slot_and_vote_nothing(to_rc):
    """An N in slot 0 and in slot 3 of an Ins group, in both reads' bytes of an X column and in the target under an '=' column: the
    slot stays empty, the bytes behind it keep their own slots, an M column with N votes no base and the view still spans it.  In the
    reversed view the slots count from the other end of the group."""
    pile = Pile(34 + to_rc)
    N = ord("N")

    def put(where):
        def edit(s1, s2):
            for read, pos in where:
                (s1 if read == 0 else s2)[pos] = N
            return s1, s2
        return edit

    # 4= 5D 4=: the group is s2[4:9];  4= 5I 4=: the group is s1[4:9]
    d0 = pile.pair(hp.cigar("4= 5D 4="), to_rc, edit=put([(1, 4)]))
    d3 = pile.pair(hp.cigar("4= 5D 4="), to_rc, edit=put([(1, 7)]))
    i0 = pile.pair(hp.cigar("4= 5I 4="), to_rc, edit=put([(0, 8 if to_rc else 4)]))      # slot 0 of view B
    i3 = pile.pair(hp.cigar("4= 5I 4="), to_rc, edit=put([(0, 5 if to_rc else 7)]))      # slot 3 of view B
    xa = pile.pair(hp.cigar("3= 1X 3="), to_rc, edit=put([(0, 3)]))                      # evidence of view B, target of view A
    xb = pile.pair(hp.cigar("3= 1X 3="), to_rc, edit=put([(1, 3)]))
    eq = pile.pair(hp.cigar("7="), to_rc, edit=put([(0, 2), (1, 2)]))                    # N on N
    for min_cov in (1, 4):
        _, _, _, votes = pile.check(min_cov, identity=False)
    for (x, s1, s2), slot in ((d0, 0), (d3, 3)):
        assert s2[4 + slot] == N
        _ins_slots(votes[x][3], s2[4:9])
        assert votes[x][3, INS0 + 4 * slot:INS0 + 4 * slot + 4].sum() == 0 and votes[x][3, INS0:INS0 + 16].sum() == 3
    for (x, s1, s2), slot in ((i0, 0), (i3, 3)):
        group = rc_bytes(s1[4:9]) if to_rc else s1[4:9]
        assert group[slot] == N
        t = len(s2) - 1 - 4 if to_rc else 3
        _ins_slots(votes[x + 1][t], group)
        assert votes[x + 1][t, INS0 + 4 * slot:INS0 + 4 * slot + 4].sum() == 0 and votes[x + 1][t, INS0:INS0 + 16].sum() == 3
    tb = 3                                                              # (7 columns: position 3 is its own mirror image)
    assert votes[xa[0] + 1][tb, :5].sum() == 0 and votes[xa[0] + 1][tb, SPAN] == 1 and votes[xa[0]][3, :4].sum() == 1
    assert votes[xb[0]][3, :5].sum() == 0 and votes[xb[0]][3, SPAN] == 1 and votes[xb[0] + 1][tb, :4].sum() == 1
    assert votes[eq[0]][2, :5].sum() == 0 and votes[eq[0] + 1][6 - 2 if to_rc else 2, :5].sum() == 0
    for x, _, _ in (d0, d3, i0, i3, xa, xb, eq):
        assert votes[x][:, 22:].sum() == 0 and votes[x + 1][:, 22:].sum() == 0


# ---- B5: the ends of the reads and of their planes ---------------------------------------------------------------------------------

TABLE = (1, 0, 63, 64, 65, 0, 255, 256, 257, 513)


def _ends_path(rows, cols):
    """A path from (0, 0) to (rows - 1, cols - 1), rows > cols: row 1 and row rows - 2 are deleted (view A has a Del at t = 1 and at
    L - 2; view B an Ins group after its t = 0 and after its L - 2), and what else the lengths ask for is made up in the middle."""
    extra = rows - cols - 2
    if extra == 0:
        return hp.cigar(f"1= 1I {cols - 2}= 1I 1=")
    if extra == -1:
        half = (cols - 3) // 2
        return hp.cigar(f"1= 1I {half}= 1D {cols - 3 - half}= 1I 1=")
    half = (cols - 2) // 2
    return hp.cigar(f"1= 1I {half}= {extra}I {cols - 2 - half}= 1I 1=")


def _swap(runs):
    return [r >> 4 << 4 | {OP_I: OP_D, OP_D: OP_I}.get(r & 15, r & 15) for r in runs]


@pytest.mark.parametrize("pairs", [((4, 2, 0), (8, 6, 1), (9, 8, 0)), ((3, 2, 1), (7, 6, 0), (4, 3, 0))],
                         ids=["64_and_256_between_voted_reads", "64_and_256_voted"])
def test_paths_from_the_first_base_to_the_last_and_reads_in_between(pairs):
    """Reads of 1, 0, 63, 64, 65, 0, 255, 256, 257 and 513 bases in this order, and paths from (0, 0) to (alen - 1, blen - 1): word p
    of position t of a read is table[12 v + p L + t], so the last position of one plane is the word before the first of the next, and
    the last plane of one read the word before the first of the next read.  Every record is there twice, and once more with the reads
    in the other roles (the same alignment: I and D change places), so that both reads are the target of a view A and of a view B with
    a Del at t = 1 and L - 2 or an Ins group after t = 0 and L - 2.  Every read of the table is compared; the ones nobody voted on
    stay all zero, between two that were voted on."""
    pile = Pile(36)
    reads = [None] * len(TABLE)
    for x, y, to_rc in pairs:                                        # (from, to): `to` may be a read an earlier pair has made
        runs = _ends_path(TABLE[x], TABLE[y])
        assert hp.rows_cols(runs) == (TABLE[x], TABLE[y]) and hp.check_canonical(runs)
        given = None if reads[y] is None else (rc_bytes(reads[y]) if to_rc else reads[y])
        assert reads[x] is None
        s1, s2 = hp.pair_from_runs(pile.rng, runs, s2=given)
        reads[x], reads[y] = s1, rc_bytes(s2) if to_rc else s2
    voted = {x for x, y, _ in pairs} | {y for x, y, _ in pairs}
    for r, length in enumerate(TABLE):
        if reads[r] is None:
            reads[r] = bytes(int(c) for c in pile.rng.choice(list(b"ACGT"), length))
    pile.reads = reads
    assert [len(r) for r in reads] == list(TABLE)
    for x, y, to_rc in pairs:
        runs = _ends_path(TABLE[x], TABLE[y])
        s2 = rc_bytes(reads[y]) if to_rc else reads[y]
        rec = pile.record(x, y, reads[x], s2, 0, 0, runs, to_rc, copies=2)
        assert (rec[0]["a1"], rec[0]["a2"], rec[0]["b1"], rec[0]["b2"]) == (0, TABLE[x] - 1, 0, TABLE[y] - 1)            # the precondition
        assert runs[1] == hp.run("I", 1) and runs[-2] == hp.run("I", 1) and runs[0] == runs[-1] == hp.run("=", 1)
        # the other way round: from y to x.  With to_rc both reads are complemented, which turns the path round
        back = _swap(runs)[::-1] if to_rc else _swap(runs)
        pile.record(y, x, reads[y], rc_bytes(reads[x]) if to_rc else reads[x], 0, 0, back, to_rc, copies=2)
    unvoted = [r for r in range(len(TABLE)) if r not in voted]
    if 3 not in voted:
        assert {3, 7} <= set(unvoted) and {2, 4, 6, 8} <= voted         # reads of 64 and 256 bases that stay zero between their neighbours
    for min_cov in (1, 4):
        seqs, stats, skipped, votes = pile.check(min_cov)
        assert skipped == 0
        for r in unvoted:
            assert votes[r].sum() == 0 and seqs[r] == reads[r]
    for x, y, to_rc in pairs:
        assert votes[x][[1, TABLE[x] - 2], DEL].tolist() == [4, 4]                     # two records and their two counterparts
        assert (votes[y][[0, TABLE[y] - 2], INS0:INS0 + 4].sum(axis=1) == 4).all()


# ---- B6: the edges of a tile of 256 positions of the call ---------------------------------------------------------------------------

DEL_AT = (1, 63, 64, 255, 256, 511)
INS_AFTER = (0, 62, 63, 64, 254, 255, 256, 510, 511)


def _tile_path(L):
    """(runs, deleted positions, junctions) for a target of L bases: a deletion at 1, 63, 64, 255, 256, 511 and L - 2 and four inserted
    bytes after 0, 62, 63, 64, 254, 255, 256, 510, 511 and L - 2, as far as the target has these positions (a path ends with '=', so
    position L - 1 cannot be deleted and has no junction after it)."""
    dels = sorted({t for t in DEL_AT + (L - 2,) if 1 <= t <= L - 2})
    ins = sorted({t for t in INS_AFTER + (L - 2,) if 0 <= t <= L - 2})
    cols = []
    for t in range(L):
        cols.append(OP_I if t in dels else OP_EQ)
        if t in ins:
            cols += [OP_D] * 4
    runs, k = [], 0
    while k < len(cols):
        n = k
        while n < len(cols) and cols[n] == cols[k]:
            n += 1
        runs.append((n - k) << 4 | cols[k])
        k = n
    return runs, dels, ins


@pytest.mark.parametrize("copies,min_cov", [(2, 1), (4, 4)])
def test_decided_deletions_and_insertions_on_the_edges_of_a_call_tile(copies, min_cov):
    """call_kernel decides 256 positions at a time, scans the emitted lengths (0 to 5 bytes a position) over four waves and carries
    `written` from tile to tile.  Targets of 255, 256, 257, 512 and 513 bases with a decided deletion (0 bytes) and a decided four-byte
    insertion (5 bytes, or 4 after a deleted position) on the last position of a wave and of a tile and on the first of the next, and a
    substitution at 0 and at L - 1 (a path begins and ends with '=', so these are '=' columns over different bytes: the vote reads
    the bytes, not the code).  With two identical views at min_cov = 1, 2 del = 4 > 3 and 2 m = 4 > span + 1 = 3; with four at
    min_cov = 4, 8 > 5.  Besides the restatement there is a second oracle: the corrected target is the evidence read, byte for byte,
    and the corrected evidence read is the target."""
    pile = Pile(37)
    made = []
    for k, L in enumerate((255, 256, 257, 512, 513)):
        runs, dels, ins = _tile_path(L)
        assert hp.check_canonical(runs) and hp.rows_cols(runs) == (L, L - len(dels) + 4 * len(ins))
        for t in (1, 63, 64, L - 2):                                 # the precondition, from the runs themselves
            assert t in dels
        assert all((t in dels) == (t <= L - 2) for t in (255, 256, 511)) and all((t in ins) == (t <= L - 2) for t in INS_AFTER)
        va, _ = cref.views_of(bytes(L), bytes(L + 4 * len(ins)), 0, 0, runs, False, 0)
        assert [c[1] for c in va if c[0] == "Del"] == dels
        assert [va[n - 1][1] for n in range(1, len(va)) if va[n][0] == "Ins" and va[n - 1][0] != "Ins"] == ins
        assert sum(c[0] == "Ins" for c in va) == 4 * len(ins)

        def edit(s1, s2):
            s2[0], s2[-1] = cref.complement(s1[0]), cref.complement(s1[-1])
            return s1, s2
        x, s1, s2 = pile.pair(runs, k % 2, copies=copies, edit=edit)
        assert len(s1) == L and s1[0] != s2[0] and s1[-1] != s2[-1]
        made.append((x, s1, s2, k % 2, len(dels), len(ins)))
    seqs, stats, skipped, _ = pile.check(min_cov)
    assert skipped == 0
    for x, s1, s2, to_rc, n_del, n_ins in made:
        assert seqs[x] == s2, (x, stats[x].tolist())
        assert seqs[x + 1] == (rc_bytes(s1) if to_rc else s1), (x + 1, stats[x + 1].tolist())
        assert stats[x].tolist() == [len(s1), len(s2), 2, n_del, 4 * n_ins, 0]
        assert stats[x + 1].tolist() == [len(s2), len(s1), 2, 4 * n_ins, n_del, 0]


# ---- B7: every counter at the cap -----------------------------------------------------------------------------------------------------

def test_every_counter_at_65535():
    """One record 65 537 times in one add.  Its view A has M columns with the evidence A, C, G and T, a junction with AAAA, with CCCC,
    with GGGG and with TTTT, and one Del column that is not the view's last, where del and span are both 65 535 and the word is
    0xFFFFFFFF.  So every one of the 22 counters is at 65 535 at a position where the other half of its word is 0 (del and span: where
    the other half is full as well): an add that carried, or a shift or mask in mhap_correct_votes or in decide that took the wrong
    half, shows.  The call on these counts equals the restatement's."""
    s1 = b"ACGTAGC"
    s2 = b"A" + b"AAAA" + b"C" + b"CCCC" + b"G" + b"GGGG" + b"T" + b"TTTT" + b"A" + b"C"
    runs = hp.cigar("1= 4D 1= 4D 1= 4D 1= 4D 1= 1I 1=")
    assert hp.check_canonical(runs) and hp.rows_cols(runs) == (len(s1), len(s2))
    rec = hp.record_for(1, 2, s1, s2, 0, 0, runs, 0)
    n = 65537
    reads = [s1, s2, b"ACGT"]
    adds = [(np.repeat(rec, n), np.arange(n + 1, dtype=np.int64) * len(runs), np.tile(np.array(runs, np.uint32), n))]
    seqs, stats, skipped, votes = _check(reads, adds)
    assert skipped == 4
    cap = cref.CAP
    va = votes[0].astype(np.int64)
    want = np.zeros((7, 24), np.int64)
    for t in range(4):                                               # evidence A, C, G, T and the junction of four of the same
        want[t, t] = cap
        want[t, [INS0 + 4 * k + t for k in range(4)]] = cap
    want[4, 0] = want[5, DEL] = want[6, 1] = cap
    want[:6, SPAN] = cap
    assert va.tolist() == want.tolist()
    for c in range(22):
        at = [t for t in range(7) if va[t, c] == cap and (va[t, c ^ 1] == (cap if c in (DEL, SPAN) else 0))]
        assert at, c
    assert (va[5, DEL] << 16 | va[5, SPAN]) == 0xFFFFFFFF
    vb = votes[1].astype(np.int64)
    assert vb[1:5, DEL].tolist() == [cap] * 4 and vb[20, INS0 + 2] == cap and vb[:21, SPAN].tolist() == [cap] * 21 and vb[21, SPAN] == 0
    assert votes[2].sum() == 0
    # the call: read A becomes the evidence, read B loses the sixteen inserted bytes and gains the G
    assert seqs[0] == s2 and seqs[1] == s1 and seqs[2] == b"ACGT"
    assert stats.tolist() == [[7, 22, 0, 1, 16, 0], [22, 7, 0, 16, 1, 0], [4, 4, 0, 0, 0, 4]]


# ---- B8: more than 2^20 accepted views in one add ------------------------------------------------------------------------------------

def test_more_than_a_million_views_in_one_add():
    """mhap_correct_add launches vote_kernel over at most 2^20 views at a time, uploading the next items into the same buffer after
    the launch before has finished.  18 reads of 8 bases in a ring, the record (r, r + 1) with the path 8= given 32 768 times, pair
    after pair: every read accepts 65 535 views, 32 768 of the record that arrives first and 32 767 of the other, 1 179 630 in all,
    so the loop runs twice.  The expected counters are these multiples of the restatement's votes for the two distinct views of each
    read; a second launch that read stale items, or none, would leave the reads of the second half short."""
    rng = np.random.default_rng(39)
    n_reads, times = 18, 32768
    reads = []
    while len(reads) < n_reads:
        r = bytes(int(c) for c in rng.choice(list(b"ACGT"), 8))
        if r not in reads:
            reads.append(r)
    runs = hp.cigar("8=")
    ring = [hp.record_for(r + 1, (r + 1) % n_reads + 1, reads[r], reads[(r + 1) % n_reads], 0, 0, runs, 0) for r in range(n_reads)]
    recs = np.repeat(np.concatenate(ring), times)
    assert len(recs) == 589824 and recs[times - 1]["from_id"] == 1 and recs[times]["from_id"] == 2                    # pair after pair
    # arrival order: read 0 gets record 0's view A first and record 17's view B last; read r > 0 record r - 1's view B first
    accepted = np.zeros((n_reads, 2), np.int64)                      # (view A of record r, view B of record r - 1)
    count, skipped_want = np.zeros(n_reads, np.int64), 0
    for q in range(n_reads):
        for target, which in ((q, 0), ((q + 1) % n_reads, 1)):
            take = min(times, cref.CAP - count[target])
            count[target] += take
            accepted[target, which] += take
            skipped_want += times - take
    assert accepted.tolist() == [[32768, 32767]] + [[32767, 32768]] * 17 and skipped_want == 18
    assert int(accepted.sum()) == 1179630 > 1 << 20                  # the precondition: a second launch
    ref = cref.Consensus(reads, range(1, n_reads + 1))
    for r in range(n_reads):
        va, _ = cref.views_of(reads[r], reads[(r + 1) % n_reads], 0, 0, runs, False, 8)
        _, vb = cref.views_of(reads[r - 1], reads[r], 0, 0, runs, False, 8)
        for view, mult in ((va, accepted[r, 0]), (vb, accepted[r, 1])):
            for t, c in cref.tally(view):
                ref.votes[r][t, c] += mult
    with mhap_amd.CorrectSession(_fasta(reads)) as cs:
        cs.add(recs, np.arange(len(recs) + 1, dtype=np.int64), np.repeat(np.array(runs, np.uint32), len(recs)))
        votes = [cs.votes(r) for r in range(n_reads)]
        seqs, stats, skipped = cs.finish(4)
    assert skipped == 18
    for r in range(n_reads):
        assert votes[r].astype(np.int64).tolist() == ref.votes[r].tolist(), r
        assert hp.coverage_identity(votes[r], [(0, 7, cref.CAP)]) == []
    wseqs, wstats = ref.call(4)
    assert seqs == wseqs and stats.tolist() == wstats.tolist()


# ---- B9: paths that repeat a code are refused -------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad,merged", [("3= 2D 3D 3=", "3= 5D 3="), ("3= 2I 3I 3=", "3= 5I 3=")])
@pytest.mark.parametrize("to_rc", [0, 1])
def test_adjacent_runs_of_one_code_are_refused(bad, merged, to_rc):
    """vote_kernel takes a run whose neighbour has its code for the continuation of a run split at 2^28 - 1 columns and votes nothing
    for its Ins columns; the contract counts slots on (D2 D3 in view A votes slots 2 and 3 from the second run).  mhap_correct_add
    refuses such a path unless the earlier run is that long, naming the record; the refused call casts no vote and takes back the
    views it had counted, and the same columns as one run are accepted."""
    pile = Pile(40)
    good = hp.cigar(merged)
    x, s1, s2 = pile.pair(good, to_rc, (1, 2), (2, 1))
    rec, repeated = pile.recs[0], hp.cigar(bad)
    assert hp.rows_cols(repeated) == hp.rows_cols(good)
    with pytest.raises(ValueError):
        hp.check_canonical(repeated)
    with mhap_amd.CorrectSession(_fasta(pile.reads)) as cs:
        with pytest.raises(mhap_amd.MhapError, match="record 1 has runs 1 and 2 of one code"):
            cs.add(np.concatenate([rec, rec]), [0, len(good), len(good) + len(repeated)], good + repeated)
        assert cs.votes(0).sum() == 0 and cs.votes(1).sum() == 0      # a refused call has cast no vote, its first record included
        with pytest.raises(mhap_amd.MhapError, match="record 0 has runs 1 and 2 of one code"):
            cs.add(rec, [0, len(repeated)], repeated)
        assert cs.votes(0).sum() == 0 and cs.votes(1).sum() == 0
    pile.check(min_cov=1)                                            # the merged runs: accepted, and equal to the restatement
