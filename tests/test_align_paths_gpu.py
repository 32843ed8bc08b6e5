"""The realignment stage's paths on the GPU (mhap_align_pairs_banded_paths, mhap_realign_records_paths, realign_kernels.hip) against their
CPU restatement (tests/align_paths_ref.py): the seven fields and every run, exactly; then `mhap-hip --realign --realign-paf` and
`python -m mhap_amd.realign --paf` end to end."""
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
from mhap_amd import realign as realign_tool  # noqa: E402
import align_ref  # noqa: E402
import align_banded_ref as bref  # noqa: E402
import align_paths_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")
R = 8                 # rows per lane (BA_R)
ONE_WAVE = 64 * R     # band rows one wave holds in one pass
PASS = 256 * R        # band rows of one pass of the four-wave kernel
FAR = 10 ** 7         # a diagonal far outside any matrix here


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


def _batch(segs):
    """(bases, pairs7) of (s1, s2, b_rc, diag, band) rows; s2 is stored as given (the aligner reverse-complements it when b_rc)."""
    bases, pairs, off, seen = bytearray(), [], 0, {}
    for s1, s2, rc, diag, band in segs:
        key = (s1, s2)
        if key not in seen:
            seen[key] = off
            bases += s1
            bases += s2
            off += len(s1) + len(s2)
        o = seen[key]
        pairs.append((o, len(s1), o + len(s1), len(s2), rc, diag, band))
    return np.frombuffer(bytes(bases) or b"\0", np.uint8), np.array(pairs, np.int64).reshape(-1, 7)


def _replay_all(bases, pairs, results, offsets, ops):
    raw = np.asarray(bases, np.uint8).tobytes()
    for q, (ao, al, bo, bl, rc, _, _) in enumerate(np.asarray(pairs).tolist()):
        s2 = raw[bo:bo + bl]
        pref.replay(raw[ao:ao + al], align_ref.rc_bytes(s2) if rc else s2, results[q], ops[offsets[q]:offsets[q + 1]])


def _check(segs, planted=None):
    """The shared check.  planted: the pairs in which the generator planted a real alignment (default: all): their score must be > 0."""
    bases, pairs = _batch(segs)
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, pairs)
    plain = mhap_amd.align_pairs_banded(bases, pairs)
    assert results.tolist() == plain.tolist()
    want, woffsets, wops = pref.align_pairs_banded_paths(bases, pairs)
    for q in range(len(pairs)):
        assert results[q].tolist() == want[q].tolist(), (q, pairs[q].tolist(), results[q].tolist(), want[q].tolist())
        got_runs, want_runs = ops[offsets[q]:offsets[q + 1]].tolist(), wops[woffsets[q]:woffsets[q + 1]].tolist()
        assert got_runs == want_runs, (q, pairs[q].tolist(), mhap_amd.cigar_string(got_runs), mhap_amd.cigar_string(want_runs))
    assert offsets.tolist() == woffsets.tolist() and ops.tolist() == wops.tolist()
    assert offsets.dtype == np.int64 and ops.dtype == np.uint32 and len(offsets) == len(pairs) + 1
    _replay_all(bases, pairs, results, offsets, ops)
    for q in (range(len(pairs)) if planted is None else planted):
        assert results[q, 0] > 0 and offsets[q + 1] > offsets[q], (q, pairs[q].tolist())
    return results, offsets, ops


def _boundary_segs(m):
    """The four placements of test_realign_gpu.test_strip_wave_and_pass_boundaries at bands R - 1, R, R + 1 and 100."""
    rng = np.random.default_rng(m)
    g = bytes(rng.choice(list(b"ACGT"), m + 400).tolist())
    s1 = g[:m]
    s2 = _mutate(rng, g[max(0, m - 250):m + 150], 0.1)     # the alignment ends near the last rows of s1
    s3 = _mutate(rng, g[:300], 0.1)                        # ... and near the first
    s4 = _mutate(rng, g, 0.08)                             # ... and runs through every row
    segs = []
    for band in (R - 1, R, R + 1, 100):
        segs += [(s1, s2, 0, -max(0, m - 250), band), (s1, s3, 0, 0, band), (s2, s1, 0, max(0, m - 250), band), (s1, s4, 0, 0, band)]
    return segs


@pytest.mark.parametrize("m", [R - 1, R, R + 1, ONE_WAVE - 1, ONE_WAVE, ONE_WAVE + 1, PASS - 1, PASS, PASS + 1, 2 * PASS + 5])
def test_strip_wave_and_pass_boundaries(m):
    """s1 of 7, 8, 9, 511, 512, 513, 2047, 2048, 2049 and 4101 bases: a lane's 8 rows, a wave's 512, one and two passes of the
    four-wave kernel (these small batches spread a tall pair over four waves)."""
    _check(_boundary_segs(m))


def _tall_segs():
    """The tall batch of test_realign_gpu.test_small_grid_takes_the_one_wave_passes."""
    rng = np.random.default_rng(9)
    segs = []
    for m in (600, 1100, 1500, 2047, 2048, 2500, 3100, 3700, 4097, 4500, 300, 0, 40):
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        st = m // 10
        t = _mutate(rng, s[st:], 0.12)
        rc = int(rng.integers(0, 2))
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc, -st, int(rng.choice([30, 100, 257]))))
    return segs


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import mhap_amd
z = np.load(sys.argv[2])
results, offsets, ops = mhap_amd.align_pairs_banded_paths(z["bases"], z["pairs"])
np.savez(sys.argv[3], results=results, offsets=offsets, ops=ops)
"""


def _in_child(tmp_path, bases, pairs, **env):
    np.savez(tmp_path / "in.npz", bases=bases, pairs=pairs)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(tmp_path / "out.npz")
    return z["results"], z["offsets"], z["ops"]


def test_small_grid_takes_the_one_wave_passes(tmp_path):
    """MHAP_NUM_CUS=2: ten tall pairs are enough for both passes to run one wave per pair, several passes each; at the full grid the
    same batch spreads each tall pair over four waves.  The same runs either way, and the restatement's."""
    segs = _tall_segs()
    full = _check(segs, planted=range(11))
    bases, pairs = _batch(segs)
    small = _in_child(tmp_path, bases, pairs, MHAP_NUM_CUS="2")
    for a, b in zip(small, full):
        assert a.tolist() == b.tolist()


def test_several_trace_groups(tmp_path):
    """MHAP_REALIGN_TRACE_BYTES = 60 000 on 40 pairs of 300 - 1 500 bases.  The band covers every matrix, so a pair's trace is its
    (insertions + deletions + 1) diagonals x its rows at 4 bits a cell, rows rounded up to whole groups of 8: the bound below is what
    the pairs need at the least, and it makes the call cross at least three groups, one of them a pair beyond the budget on its own.
    A budget of 1 byte puts every pair into a group of its own.  Offsets and runs equal those under the default budget."""
    budget = 60000
    rng = np.random.default_rng(40)
    segs = []
    for k in range(40):
        m = 1500 if k == 17 else int(rng.integers(300, 1501))
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        t = _mutate(rng, s, 0.2 if k == 17 else rng.uniform(0.05, 0.15))
        rc = k % 2
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc, 0, 2000))
    results, offsets, ops = _check(segs)
    rows = results[:, 2] - results[:, 1] + 1
    gaps = (results[:, 5] - rows) + (results[:, 5] - (results[:, 4] - results[:, 3] + 1))
    least = 4 * (gaps + 1).astype(np.int64) * ((rows + 7) // 8)
    assert least.sum() >= 3 * budget and least.max() > budget and (least < budget // 2).sum() >= 10, (least.sum(), least.max())
    bases, pairs = _batch(segs)
    for b in (budget, 1):
        got = _in_child(tmp_path, bases, pairs, MHAP_REALIGN_TRACE_BYTES=str(b))
        assert got[0].tolist() == results.tolist() and got[1].tolist() == offsets.tolist() and got[2].tolist() == ops.tolist(), b


def test_ties_gaps_and_the_band_edge():
    a, b = b"A" * 500, b"A" * 400
    segs = []
    for band in (3, 40, 1000):
        segs += [(a, b, 0, 0, band), (a, b"T" * 400, 1, 0, band), (a, b, 0, -50, band), (b, b"T" * 500, 1, 37, band)]
    rng = np.random.default_rng(60)
    g = bytes(rng.choice(list(b"ACGT"), 900).tolist())
    cut60 = g[:400] + g[460:]
    segs += [(g, cut60, 0, 0, 100), (cut60, g, 0, 0, 100)]             # 60 I in one path, 60 D in the other: extension against open
    segs += [(g, cut60, 0, -30, 30), (cut60, g, 0, 30, 30)]            # the path runs along both edges of the band
    cut10 = g[:300] + g[310:]
    segs += [(g, cut10, 0, 0, 10), (cut10, g, 0, 0, 10), (g, cut10, 0, -10, 10)]   # the path touches the band's edge
    segs += [(g, cut60, 0, 0, 10), (cut60, g, 0, 0, 10), (g, cut60, 0, -60, 10)]   # the band cuts the alignment: the longest piece
    results, offsets, ops = _check(segs)
    n = len(segs)
    runs = [[(int(r) >> 4, int(r) & 15) for r in ops[offsets[q]:offsets[q + 1]]] for q in range(n)]
    assert runs[12] == [(400, pref.OP_EQ), (60, pref.OP_I), (440, pref.OP_EQ)] and runs[13] == [(400, pref.OP_EQ), (60, pref.OP_D), (440, pref.OP_EQ)]
    assert runs[14] == runs[12] and runs[15] == runs[13]
    assert [c for _, c in runs[16]] == [pref.OP_EQ, pref.OP_I, pref.OP_EQ] and [c for _, c in runs[17]] == [pref.OP_EQ, pref.OP_D, pref.OP_EQ]
    # cut by the band, the identical piece in it is kept whole and the path goes on through unrelated bases while its score stays positive
    assert runs[n - 3][0] == (400, pref.OP_EQ) and runs[n - 2][0] == (400, pref.OP_EQ) and runs[n - 1][-1] == (440, pref.OP_EQ)
    assert all(len(runs[q]) > 100 for q in (n - 3, n - 2, n - 1))
    assert runs[0] == [(400, pref.OP_EQ)] and results[0].tolist()[:5] == [800, 0, 399, 0, 399]


def test_empty_and_degenerate_pairs_between_neighbours_with_runs():
    rng = np.random.default_rng(3)
    s = bytes(rng.choice(list(b"ACGT"), 700).tolist())
    t = _mutate(rng, s, 0.1)
    good = (s, t, 0, 0, 50)
    n_read = bytearray(s)
    n_read[350] = ord("N")
    n_read = bytes(n_read)
    segs = [(b"", t, 0, 0, 5), good, (s, b"", 0, 0, 5), (b"", b"", 0, 0, 5), good, (b"A", b"C", 0, 0, 1), (b"A", b"A", 0, 0, 0), good,
            (s, t, 0, FAR, 50), (s, t, 0, -FAR, 50), good, (b"AAAAAAAAAAAA", b"CCCCCCCCCCCCCCC", 0, 0, 20), (b"G", t, 0, 0, 10 ** 6), good,
            (n_read, align_ref.rc_bytes(t), 1, 0, 50), (n_read, n_read, 0, 0, 3)]
    planted = [1, 4, 6, 7, 10, 12, 13, 14, 15]
    results, offsets, ops = _check(segs, planted=planted)
    for q in (0, 2, 3, 5, 8, 9, 11):
        assert results[q].tolist() == list(bref.NONE) and offsets[q + 1] == offsets[q], q
    assert ops[offsets[6]:offsets[7]].tolist() == [1 << 4 | pref.OP_EQ]
    assert ops[offsets[15]:offsets[16]].tolist() == [700 << 4 | pref.OP_EQ]          # N against N is an equal byte
    assert ops[offsets[1]:offsets[2]].tolist() == ops[offsets[13]:offsets[14]].tolist()
    empty = mhap_amd.align_pairs_banded_paths(np.zeros(1, np.uint8), np.zeros((0, 7), np.int64))
    assert empty[0].shape == (0, 7) and empty[1].tolist() == [0] and len(empty[2]) == 0


def test_random_pairs_both_strands_and_an_n():
    """The random pairs of test_realign_gpu (even ones forward, odd ones b_rc, one with an N) around their true diagonal."""
    rng = np.random.default_rng(21)
    segs = []
    for k in range(8):
        n = int(rng.integers(0, 3001)) if k > 1 else k * 5
        s = bytearray(rng.choice(list(b"ACGT"), n).tolist())
        if k == 3 and n > 10:
            s[n // 2] = ord("N")
        s = bytes(s)
        st = int(rng.integers(0, max(1, n // 4)))
        t = _mutate(rng, s[st:], rng.uniform(0, 0.2))
        rc = k % 2
        for band in (7, 64, 500):
            segs.append((s, align_ref.rc_bytes(t) if rc else t, rc, -st, band))
    _check(segs, planted=range(6, len(segs)))


def test_invalid_pairs_are_refused_with_their_index():
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    ok = [0, 4, 4, 4, 0, 0, 2]
    results, offsets, ops = mhap_amd.align_pairs_banded_paths(bases, [ok])
    assert results.tolist() == [[8, 0, 3, 0, 3, 4, 0]] and offsets.tolist() == [0, 1] and ops.tolist() == [4 << 4 | pref.OP_EQ]
    with pytest.raises(mhap_amd.MhapError, match="pair 1"):
        mhap_amd.align_pairs_banded_paths(bases, [ok, [0, 4, 4, 4, 0, 0, -1]])
    with pytest.raises(mhap_amd.MhapError, match="pair 2"):
        mhap_amd.align_pairs_banded_paths(bases, [ok, ok, [0, 4, 6, 4, 0, 0, 2]])
    # the C entry point itself: no object comes back with an error
    import ctypes as C
    from mhap_amd import api
    pairs = np.array([ok, [0, 4, 6, 4, 0, 0, 2]], np.int64)
    out = np.zeros((2, 7), np.int32)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        obj = C.c_void_p(12345)
        rc = ms._lib.mhap_align_pairs_banded_paths(ms._h, api._ptr(bases), C.c_int64(8), api._ptr(pairs), C.c_int64(2), api._ptr(out), C.byref(obj))
        assert rc == -1 and obj.value is None and b"pair 1" in ms._lib.mhap_last_error(ms._h)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

N_READS, READ_LEN, SEED = 120, 2000, 0x5EA1


@pytest.fixture(scope="module")
def searched():
    fasta = mhap_amd.synth_reads(N_READS, READ_LEN, seed=SEED, coverage=30.0, error_rate=0.15)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
        ms.add_data(fasta)
        recs = ms.find_matches()
        recs = recs[np.lexsort((recs["to_rc"], recs["to_id"], recs["from_id"]))].copy()
        plain = mhap_amd.realign_records(recs, fasta, handle=ms)
        paths = mhap_amd.realign_records_paths(recs, fasta, handle=ms)
    return fasta, recs, plain, paths


def test_realign_records_paths_equals_realign_records_and_the_restatement(searched):
    fasta, recs, (out0, detail0), (out, detail, offsets, ops) = searched
    assert len(recs) >= 64 and out.tobytes() == out0.tobytes() and detail.tobytes() == detail0.tobytes()
    pairs = mhap_amd.realign_plan(recs, fasta)
    want, woffsets, wops = pref.align_pairs_banded_paths(fasta.bases, pairs)
    wout, wdetail = bref.to_records(recs, want)
    assert out.tolist() == wout.tolist() and detail.tolist() == wdetail.tolist()
    assert offsets.tolist() == woffsets.tolist() and ops.tolist() == wops.tolist()
    _replay_all(fasta.bases, pairs, want, offsets, ops)
    assert (detail[:, 0] > 0).sum() >= 64 and (recs["to_rc"][detail[:, 0] > 0] != 0).any() and (recs["to_rc"][detail[:, 0] > 0] == 0).any()
    # a given band, a handle of its own
    out2, detail2, offsets2, ops2 = mhap_amd.realign_records_paths(recs[:8], fasta, band=25)
    want2, woffsets2, wops2 = pref.align_pairs_banded_paths(fasta.bases, mhap_amd.realign_plan(recs[:8], fasta, band=25))
    assert out2.tolist() == bref.to_records(recs[:8], want2)[0].tolist() and offsets2.tolist() == woffsets2.tolist() and ops2.tolist() == wops2.tolist()


def _write_fasta(path, fasta):
    with open(path, "w") as fh:
        for i in range(len(fasta)):
            fh.write(f">read{i}\n{fasta.sequence(i)}\n")


def _replay_paf_line(line, fasta):
    """12 fixed columns and three tags; the CIGAR over the FASTA's bases: on `-` over rc(query[qstart:qend]) and target[tstart:tend]."""
    c = line.split("\t")
    assert len(c) == 15 and c[11] == "255" and c[4] in "+-", line
    assert re.fullmatch(r"NM:i:\d+", c[12]) and re.fullmatch(r"AS:i:\d+", c[13]) and re.fullmatch(r"cg:Z:(\d+[=XID])+", c[14]), line
    row = {int(i): k for k, i in enumerate(fasta.ids.tolist())}
    q, t = fasta.sequence(row[int(c[0])]).encode(), fasta.sequence(row[int(c[5])]).encode()
    qs, qe, ts, te = int(c[2]), int(c[3]), int(c[7]), int(c[8])
    assert int(c[1]) == len(q) and int(c[6]) == len(t) and 0 <= qs < qe <= len(q) and 0 <= ts < te <= len(t)
    qseg, tseg = (align_ref.rc_bytes(q[qs:qe]) if c[4] == "-" else q[qs:qe]), t[ts:te]
    i = j = match = cols = 0
    for length, op in ((int(a), b) for a, b in re.findall(r"(\d+)([=XID])", c[14][5:])):
        if op in "=X":
            assert all((qseg[i + u] == tseg[j + u]) == (op == "=") for u in range(length)), (line[:80], i, j, op)
            match += length if op == "=" else 0
            i, j = i + length, j + length
        elif op == "I":
            i += length
        else:
            j += length
        cols += length
    assert (i, j) == (len(qseg), len(tseg)) and int(c[9]) == match and int(c[10]) == cols and int(c[12][5:]) == cols - match, line[:120]


def test_driver_and_tool_print_the_same_paf_lines(searched, tmp_path):
    fasta, recs, (out0, _), (out, detail, offsets, ops) = searched
    path = tmp_path / "reads.fasta"
    _write_fasta(path, fasta)

    def run(extra, code=0):
        p = subprocess.run([CLI, "-s", str(path)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == code, p.stderr[-2000:]
        return sorted(l for l in p.stdout.split("\n") if l), p.stderr

    plain, err0 = run([])
    assert plain == sorted(mhap_amd.records_to_lines(recs)) and "realign" not in err0
    lines, err = run(["--realign"])                      # without the new flag: what it printed before
    kept = realign_tool.keep(out0)
    assert lines == sorted(mhap_amd.records_to_lines(kept)) and "--realign-paf" in err
    paf, err = run(["--realign", "--realign-paf"])
    rows = realign_tool.kept_rows(out).tolist()
    assert paf == sorted(mhap_amd.format_paf(out[q], detail[q], ops[offsets[q]:offsets[q + 1]]) for q in rows) and len(paf) == len(kept) > 0
    assert f"({len(kept)} overlaps kept, {len(recs) - len(kept)} dropped" in err and "Time (s) to realign:" in err
    assert any(l.split("\t")[4] == "-" for l in paf) and any(l.split("\t")[4] == "+" for l in paf)
    for l in paf:
        _replay_paf_line(l, fasta)
    paf9, _ = run(["--realign", "--realign-paf", "--realign-min-identity", "0.8", "--realign-band", "40"])
    out40, _ = mhap_amd.realign_records(recs, fasta, band=40)
    assert 0 < len(paf9) == len(realign_tool.keep(out40, 0.8))
    for l in paf9:
        _replay_paf_line(l, fasta)
    # the stand-alone tool on the driver's own output
    (tmp_path / "ovl.txt").write_text("\n".join(plain) + "\n")
    p = subprocess.run([sys.executable, "-m", "mhap_amd.realign", str(tmp_path / "ovl.txt"), str(path), "--paf"], capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(l for l in p.stdout.split("\n") if l) == paf
    # --realign-paf alone is refused with one line
    p = subprocess.run([CLI, "-s", str(path), "--realign-paf"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--realign-paf" in p.stdout and p.stdout.count("\n") == 1, (p.stdout, p.stderr[-500:])
