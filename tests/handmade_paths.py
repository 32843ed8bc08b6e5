"""Hand-made alignment paths for the read-correction tests: reads built to fit a given list of runs, so that every kind of column can
be put on purpose where the vote and call kernels change chunk, deal, plane, tile or launch (the aligner's own paths put them there
by accident, and never put an 'I' run next to a 'D' run).  Plain Python over numpy; nothing here calls the library.

    runs = cigar("3= 2I 1= 1D 2=")                       # or runs_with("D", 4, 64, 129)
    A, s2 = pair_from_runs(rng, runs, (fa, ta), (fb, tb))
    rec = record_for(1, 2, A, s2, fa, fb, runs, to_rc)   # the stored read B is rc_bytes(s2) when to_rc
"""
import numpy as np

import consensus_ref as cref
from consensus_ref import OP_D, OP_EQ, OP_I, OP_X

CODES = {"=": OP_EQ, "X": OP_X, "I": OP_I, "D": OP_D}
NAMES = {v: k for k, v in CODES.items()}


def run(kind, length):
    return int(length) << 4 | CODES[kind]


def cigar(text):
    """Runs from "3= 2I 1=" (blanks are optional)."""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        elif ch in CODES:
            out.append(run(ch, int(n)))
            n = ""
        elif not ch.isspace():
            raise ValueError(f"run kind {ch!r}")
    if n:
        raise ValueError("a length without a kind")
    return out


def as_text(runs):
    return "".join(f"{int(r) >> 4}{NAMES[int(r) & 15]}" for r in runs)


def rows_cols(runs):
    """(rows of s1, columns of s2) that the runs consume."""
    rows = sum(int(r) >> 4 for r in runs if int(r) & 15 != OP_D)
    cols = sum(int(r) >> 4 for r in runs if int(r) & 15 != OP_I)
    return rows, cols


def check_canonical(runs):
    """The header's rules for a path, except the split at 2^28 - 1: the first and the last run are '=', every length is at least 1,
    every code is one of the four and no two adjacent runs have the same code.  Raises ValueError, else returns the runs."""
    runs = [int(r) for r in runs]
    if not runs or runs[0] & 15 != OP_EQ or runs[-1] & 15 != OP_EQ:
        raise ValueError("a path begins and ends with '='")
    for u, r in enumerate(runs):
        if r & 15 not in NAMES or r >> 4 < 1:
            raise ValueError(f"run {u} is {r >> 4} columns of code {r & 15}")
        if u and runs[u - 1] & 15 == r & 15:
            raise ValueError(f"runs {u - 1} and {u} have the same code")
    return runs


def pair_from_runs(rng, runs, flank_a=(0, 0), flank_b=(0, 0), alphabet=b"ACGT", s2=None):
    """(A, s2): random reads over `alphabet` with fa / fb bases before the path and ta / tb after it, such that `runs` is a path from
    (fa, fb): the bytes are equal on '=' columns and different on 'X' columns, 'I' columns consume A only and 'D' columns s2 only.
    With s2 given (a read that another record has fixed already: fb + columns + tb bytes) only A is made, to fit it."""
    (fa, ta), (fb, tb) = flank_a, flank_b
    letters = list(alphabet)

    def draw(n):
        return [int(x) for x in rng.choice(letters, n)]

    if s2 is not None and len(s2) != fb + rows_cols(runs)[1] + tb:
        raise ValueError("the given s2 has another length than its flanks and the path's columns")
    a, b = draw(fa), (list(s2[:fb]) if s2 is not None else draw(fb))
    for r in runs:
        length, code = int(r) >> 4, int(r) & 15
        given = list(s2[len(b):len(b) + length]) if s2 is not None else None
        if code == OP_EQ:
            same = given or draw(length)
            a += same
            b += same
        elif code == OP_X:
            for c in given or draw(length):
                a.append(int(rng.choice([x for x in letters if x != c])))
                b.append(c)
        elif code == OP_I:
            a += draw(length)
        elif code == OP_D:
            b += given or draw(length)
        else:
            raise ValueError(f"run code {code}")
    return bytes(a + draw(ta)), bytes(b + (list(s2[len(b):]) if s2 is not None else draw(tb)))


def record_for(ida, idb, A, s2, fa, fb, runs, to_rc):
    """The realigned record (consensus_ref.RECORD_DTYPE, one row) of the path `runs` from (fa, fb) over read A and s2: a1, a2 the first
    and last row, b1, b2 the first and last column, flipped back to the stored strand when to_rc (the stored read B is rc_bytes(s2))."""
    rows, cols = rows_cols(runs)
    alen, blen = len(A), len(s2)
    j0, j1 = fb, fb + cols - 1
    if not (rows >= 1 and cols >= 1 and fa + rows <= alen and j1 < blen):
        raise ValueError("the path does not fit the reads")
    n = sum(int(r) >> 4 for r in runs)
    errors = sum(int(r) >> 4 for r in runs if int(r) & 15 != OP_EQ)
    rec = np.zeros(1, cref.RECORD_DTYPE)
    rec[0] = (ida, idb, 1.0 - errors / n, 0.0, fa, fa + rows - 1, alen, blen - 1 - j1 if to_rc else j0, blen - 1 - j0 if to_rc else j1, blen,
              int(bool(to_rc)), 0)
    return rec


def runs_with(kind, length, at_index, total_runs, rng=None):
    """A canonical path of total_runs runs (an odd number) whose run at_index is `kind` with `length` columns.  The rest are fillers:
    '=' of 1 to 3 columns on the even indices and 'X' of 1 column on the odd ones, so that the first and the last run are '='.  Where
    that would put `kind` next to a run of its own code (an 'X' on an even index, an '=' on an odd one) the parity is shifted between
    the ends and at_index by the only means there is, two adjacent runs that are not '=': runs 1, 2 become X, D and the last
    two before the final '=' become I, X (only the D, only the I, where at_index is 2 or total_runs - 3 and leaves room for one)."""
    rng = rng or np.random.default_rng(total_runs * 1000 + at_index)
    if total_runs % 2 != 1 or not 0 <= at_index < total_runs:
        raise ValueError("an odd number of runs and an index among them")
    if at_index in (0, total_runs - 1) and kind != "=":
        raise ValueError("the first and the last run are '='")
    codes = ["=" if u % 2 == 0 else "X" for u in range(total_runs)]
    neighbour = "X" if at_index % 2 == 0 else "="
    if kind == neighbour:
        if not 2 <= at_index <= total_runs - 3:
            raise ValueError("no room to shift the parity")
        codes[1:at_index] = (["X", "D"] + ["=" if u % 2 == 1 else "X" for u in range(3, at_index)])[-(at_index - 1):]
        codes[at_index + 1:total_runs - 1] = (["=" if u % 2 == 1 else "X" for u in range(at_index + 1, total_runs - 3)] + ["I", "X"])[:total_runs - 2 - at_index]
    codes[at_index] = kind
    out = [run(c, int(rng.integers(1, 4)) if c == "=" else 1) for c in codes]
    out[at_index] = run(kind, length)
    return check_canonical(out)


def target_intervals(rec):
    """((lo, hi) of view A on read A, (lo, hi) of view B on the stored read B) of a record_for row: both ends included."""
    r = rec[0]
    return (int(r["a1"]), int(r["a2"])), (int(r["b1"]), int(r["b2"]))


def coverage_identity(votes, intervals):
    """The identity every vote table obeys whose views' bytes are all A, C, G, T, whatever the paths: with `intervals` the (lo, hi) of
    the accepted views on this read (or (lo, hi, n) for n views of one interval), base[t].sum() + del[t] is the number of views that
    contain t, span[t] the number that contain t and t + 1, and the two spare counters are 0.  Returns the list of (t, what, got,
    want) that differ."""
    v = np.asarray(votes).astype(np.int64)
    L = len(v)
    cover, span = np.zeros(L + 1, np.int64), np.zeros(L + 1, np.int64)
    for lo, hi, *n in intervals:
        cover[lo:hi + 1] += n[0] if n else 1
        span[lo:hi] += n[0] if n else 1
    bad = []
    for t in range(L):
        if v[t, :4].sum() + v[t, cref.DEL] != cover[t]:
            bad.append((t, "cover", int(v[t, :4].sum() + v[t, cref.DEL]), int(cover[t])))
        if v[t, cref.SPAN] != span[t]:
            bad.append((t, "span", int(v[t, cref.SPAN]), int(span[t])))
        if v[t, 22:].any():
            bad.append((t, "spare", v[t, 22:].tolist(), [0, 0]))
    return bad
