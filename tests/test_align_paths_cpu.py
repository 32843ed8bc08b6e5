"""The realignment stage's paths without a GPU: the path restatement (tests/align_paths_ref.py) against the merged banded one
(tests/align_banded_ref.py) on the generators of tests/test_realign_gpu.py, and the host-side PAF and CIGAR formatters."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
import align_ref  # noqa: E402
import align_banded_ref as bref  # noqa: E402
import align_paths_ref as pref  # noqa: E402
import test_realign_gpu as gen  # noqa: E402   (its generators only; its tests are collected from their own file)


def _replay_batch(bases, pairs, results, offsets, ops):
    raw = np.asarray(bases, np.uint8).tobytes()
    for q, (ao, al, bo, bl, rc, _, _) in enumerate(np.asarray(pairs).tolist()):
        s1, s2 = raw[ao:ao + al], raw[bo:bo + bl]
        pref.replay(s1, align_ref.rc_bytes(s2) if rc else s2, results[q], ops[offsets[q]:offsets[q + 1]])


def test_path_restatement_equals_the_banded_one_and_replays():
    """The random pairs, bands and diagonals of test_realign_gpu.test_random_pairs_bands_and_diagonals: the seven fields that come
    out of the trace-back equal the ones align_banded_ref carries through the matrix, and every path replays."""
    segs = []
    for s, t, rc, d in gen._random_pairs(21, 8):
        cover = max(len(s), len(t), 1)
        for band in (0, 1, 7, 64, 500, cover + abs(d)):
            for diag in (d, d + band, d - band, gen.FAR, -gen.FAR) if band != cover + abs(d) else (d,):
                segs.append((s, t, rc, diag, band))
    bases, pairs = gen._batch(segs)
    results, offsets, ops = pref.align_pairs_banded_paths(bases, pairs)
    want = bref.align_pairs_banded(bases, pairs)
    assert results.tolist() == want.tolist()
    assert (results[:, 0] > 0).sum() > len(segs) // 3
    _replay_batch(bases, pairs, results, offsets, ops)


def test_small_paths_spelled_out():
    eq, x, ins, dele = pref.OP_EQ, pref.OP_X, pref.OP_I, pref.OP_D
    assert pref.align_path(b"ACGT", b"ACGT", 0, 0) == ((8, 0, 3, 0, 3, 4, 0), [4 << 4 | eq])
    # one substitution inside: 5 = 1 X 5 =
    f, runs = pref.align_path(b"ACGTAGACGTA", b"ACGTATACGTA", 0, 2)
    assert f == (18, 0, 10, 0, 10, 11, 1) and runs == [5 << 4 | eq, 1 << 4 | x, 5 << 4 | eq]
    # s1 has two extra bases: an insertion (consumes s1 only); the other way round a deletion
    a, b = b"ACGTACGATTGGCCAAGGTT", b"ACGTACGAGGCCAAGGTT"
    f, runs = pref.align_path(a, b, 0, 5)
    assert [(r >> 4, r & 15) for r in runs] == [(8, eq), (2, ins), (10, eq)] and f == (36 - 3, 0, 19, 0, 17, 20, 2)
    f, runs = pref.align_path(b, a, 0, 5)
    assert [(r >> 4, r & 15) for r in runs] == [(8, eq), (2, dele), (10, eq)] and f == (36 - 3, 0, 17, 0, 19, 20, 2)
    assert pref.align_path(b"AAAA", b"CCCC", 0, 4) == (pref.NONE, [])
    assert pref.encode([eq] * 3 + [x] + [dele] * 2) == [3 << 4 | eq, 1 << 4 | x, 2 << 4 | dele]


# ---- mhap_format_paf and cigar_string ---------------------------------------------------------------------------------------------------

def _rec(from_id, to_id, score, a1, a2, alen, b1, b2, blen, to_rc):
    r = np.zeros(1, api.RECORD_DTYPE)
    r[0] = (from_id, to_id, score, 55.0, a1, a2, alen, b1, b2, blen, to_rc, 0)
    return r[0]


def _ops(*runs):
    code = {"=": 7, "X": 8, "I": 1, "D": 2}
    return np.array([length << 4 | code[c] for length, c in runs], np.uint32)


def test_cigar_string():
    ops = _ops((5, "="), (1, "X"), (2, "I"), (7, "="), (3, "D"), (4, "="))
    assert mhap_amd.cigar_string(ops) == "5=1X2I7=3D4="
    assert mhap_amd.cigar_string(ops, reverse=True) == "4=3D7=2I1X5="
    assert mhap_amd.cigar_string([]) == "" and mhap_amd.cigar_string(np.zeros(0, np.uint32), reverse=True) == ""
    big = (1 << 28) - 1
    assert mhap_amd.cigar_string(_ops((big, "="), (5, "="), (1, "X"))) == f"{big}=5=1X"


def test_format_paf_forward_and_reverse():
    ops = _ops((5, "="), (1, "X"), (2, "I"), (7, "="), (3, "D"), (4, "="))
    # 22 columns: 19 of the query (a 100..118), 20 of the target (b 40..59); errors 1 + 2 + 3, score 2 * 16 - 2 - 3 - 4
    detail = [23, 22, 6]
    fwd = _rec(12, 7, 1 - 6 / 22, 100, 118, 4000, 40, 59, 5000, 0)
    line = mhap_amd.format_paf(fwd, detail, ops)
    assert line == "12\t4000\t100\t119\t+\t7\t5000\t40\t60\t16\t22\t255\tNM:i:6\tAS:i:23\tcg:Z:5=1X2I7=3D4="
    assert "\n" not in line and len(line.split("\t")) == 15
    rev = _rec(12, 7, 1 - 6 / 22, 100, 118, 4000, 40, 59, 5000, 1)
    assert mhap_amd.format_paf(rev, detail, ops) == "12\t4000\t100\t119\t-\t7\t5000\t40\t60\t16\t22\t255\tNM:i:6\tAS:i:23\tcg:Z:4=3D7=2I1X5="
    # names: whatever columns 1 and 2 of the 12-column line would be
    named = mhap_amd.format_paf(fwd, detail, ops, qname="readA", tname="chr/1")
    assert named.split("\t")[0] == "readA" and named.split("\t")[5] == "chr/1" and named.split("\t")[1:5] == line.split("\t")[1:5]
    # a run split at 2^28 - 1 is printed as the two runs it is
    big = (1 << 28) - 1
    split = mhap_amd.format_paf(fwd, [2 * (big + 5), big + 5, 0], _ops((big, "="), (5, "=")))
    assert split.endswith(f"\t{big + 5}\t{big + 5}\t255\tNM:i:0\tAS:i:{2 * (big + 5)}\tcg:Z:{big}=5=")


def test_format_paf_cap_too_small_returns_the_needed_length():
    lib = mhap_amd.load_library()
    ops = _ops((5, "="), (1, "X"), (9, "="))
    rec = np.zeros(1, api.RECORD_DTYPE)
    rec[0] = _rec(3, 4, 0.9, 0, 14, 100, 10, 24, 200, 0)
    detail = np.array([26, 15, 1], np.int32)
    want = mhap_amd.format_paf(rec[0], detail, ops).encode()

    def call(cap):
        buf = C.create_string_buffer(b"\xff" * max(cap, 1), max(cap, 1))
        n = lib.mhap_format_paf(api._ptr(rec), api._ptr(detail), api._ptr(ops), C.c_int64(len(ops)), b"3", b"4", buf if cap else None,
                                C.c_size_t(cap))
        return n, buf.raw

    n, raw = call(len(want) + 1)
    assert n == len(want) and raw[:n + 1] == want + b"\0"
    n, raw = call(10)                                      # too small: the needed length, a truncated NUL-terminated line
    assert n == len(want) and raw[:10] == want[:9] + b"\0"
    n, _ = call(0)
    assert n == len(want)
    n, raw = call(len(want))                               # one short: still the needed length
    assert n == len(want) and raw[:len(want)] == want[:-1] + b"\0"
    assert lib.mhap_format_paf(None, api._ptr(detail), api._ptr(ops), C.c_int64(3), b"3", b"4", None, C.c_size_t(0)) == -1


def _replay_cigar(cigar, q, t):
    """A CIGAR with = X I D over query bytes q and target bytes t, both consumed completely."""
    i = j = 0
    for length, c in ((int(a), b) for a, b in re.findall(r"(\d+)([=XID])", cigar)):
        if c in "=X":
            for u in range(length):
                assert (q[i + u] == t[j + u]) == (c == "="), (i + u, j + u, c)
            i, j = i + length, j + length
        elif c == "I":
            i += length
        else:
            j += length
    assert re.fullmatch(r"(\d+[=XID])*", cigar) and (i, j) == (len(q), len(t)), (cigar, i, j)


def test_reverse_strand_paf_replays_over_the_reverse_complemented_query():
    """A `-` record end to end on the CPU: the aligner's s2 is rc(target); the path restatement aligns the query against it; the
    record's b interval is flipped back onto the target's own strand as mhap_realign_records does; and the printed CIGAR, which is the
    path's runs reversed, replays over rc(query[qstart:qend]) and target[tstart:tend]."""
    rng = np.random.default_rng(77)
    g = bytes(rng.choice(list(b"ACGT"), 700).tolist())
    query = g[50:600]
    target_fwd = gen._mutate(rng, g[200:], 0.12)           # what the aligner sees as s2
    target = align_ref.rc_bytes(target_fwd)                # what the file stores
    fields, runs = pref.align_path(query, target_fwd, -150, 60)
    score, rb, re_, fb, fe, cols, errs = fields
    assert score > 200 and errs > 5 and any(r & 15 == pref.OP_I for r in runs) and any(r & 15 == pref.OP_D for r in runs)
    blen = len(target)
    rec = _rec(1, 2, 1 - errs / cols, rb, re_, len(query), blen - fe - 1, blen - fb - 1, blen, 1)
    cols15 = mhap_amd.format_paf(rec, [score, cols, errs], runs).split("\t")
    assert cols15[4] == "-" and cols15[14] == "cg:Z:" + mhap_amd.cigar_string(runs, reverse=True)
    qs, qe, ts, te = int(cols15[2]), int(cols15[3]), int(cols15[7]), int(cols15[8])
    assert (qs, qe) == (rb, re_ + 1) and te - ts == fe - fb + 1                     # qend and tend are exclusive
    _replay_cigar(cols15[14][5:], align_ref.rc_bytes(query[qs:qe]), target[ts:te])
    assert int(cols15[9]) == cols - errs and int(cols15[10]) == cols
    # and the `+` line of the same alignment replays in path order
    rec = _rec(1, 2, 1 - errs / cols, rb, re_, len(query), fb, fe, len(target_fwd), 0)
    cols15 = mhap_amd.format_paf(rec, [score, cols, errs], runs).split("\t")
    _replay_cigar(cols15[14][5:], query[int(cols15[2]):int(cols15[3])], target_fwd[int(cols15[7]):int(cols15[8])])


def test_driver_lists_realign_paf_and_refuses_it_alone(tmp_path):
    import subprocess
    cli = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "\t--realign-paf," in p.stdout
    fa = tmp_path / "reads.fasta"
    fa.write_text(">r1\nACGTACGTACGT\n")
    p = subprocess.run([cli, "-s", str(fa), "--realign-paf"], capture_output=True, text=True, timeout=60)     # before a handle exists
    assert p.returncode == 1 and "--realign-paf" in p.stdout and "--realign" in p.stdout and p.stdout.count("\n") == 1, (p.stdout, p.stderr[-500:])
    assert "--paf" in subprocess.run([sys.executable, "-m", "mhap_amd.realign", "--help"], capture_output=True, text=True, timeout=60,
                                     cwd=ROOT).stdout
