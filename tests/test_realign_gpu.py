"""The realignment stage on the GPU: the banded aligner (mhap_align_pairs_banded, realign_kernels.hip) against its CPU restatement
(tests/align_banded_ref.py), all seven fields, exactly; mhap_realign_records and `mhap-hip --realign` end to end; and the reason the
stage exists — realigned intervals are closer to the truth than the sketch's estimates."""
import os
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


def _check(segs, handle=None):
    bases, pairs = _batch(segs)
    got = mhap_amd.align_pairs_banded(bases, pairs, handle=handle)
    want = bref.align_pairs_banded(bases, pairs)
    for q in range(len(pairs)):
        assert got[q].tolist() == want[q].tolist(), (q, pairs[q].tolist(), got[q].tolist(), want[q].tolist())
    return got


def _random_pairs(seed, count):
    """(s1, stored s2, b_rc, true diagonal): s2 is a mutated suffix of s1 that starts at s1's base `st`, so the alignment lies near
    j - i = -st; one pair carries an N."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 3001)) if k > 1 else k * 5
        s = bytearray(rng.choice(list(b"ACGT"), n).tolist())
        if k == 3 and n > 10:
            s[n // 2] = ord("N")
        s = bytes(s)
        st = int(rng.integers(0, max(1, n // 4)))
        t = _mutate(rng, s[st:], rng.uniform(0, 0.2))
        rc = k % 2
        out.append((s, align_ref.rc_bytes(t) if rc else t, rc, -st))
    return out


def test_random_pairs_bands_and_diagonals():
    segs = []
    for s, t, rc, d in _random_pairs(21, 8):
        cover = max(len(s), len(t), 1)
        for band in (0, 1, 7, 64, 500, cover + abs(d)):
            for diag in (d, d + band, d - band, FAR, -FAR) if band != cover + abs(d) else (d,):
                segs.append((s, t, rc, diag, band))
    got = _check(segs)
    assert (got[:, 0] > 0).sum() > len(segs) // 3


@pytest.mark.parametrize("m", [R - 1, R, R + 1, ONE_WAVE - 1, ONE_WAVE, ONE_WAVE + 1, PASS - 1, PASS, PASS + 1, 2 * PASS + 1, 3 * PASS + 5])
def test_strip_wave_and_pass_boundaries(m):
    rng = np.random.default_rng(m)
    g = bytes(rng.choice(list(b"ACGT"), m + 400).tolist())
    s1 = g[:m]
    s2 = _mutate(rng, g[max(0, m - 250):m + 150], 0.1)     # the alignment ends near the last rows of s1
    s3 = _mutate(rng, g[:300], 0.1)                        # ... and near the first
    s4 = _mutate(rng, g, 0.08)                             # ... and runs through every row
    segs = []
    for band in (R - 1, R, R + 1, 100):
        segs += [(s1, s2, 0, -max(0, m - 250), band), (s1, s3, 0, 0, band), (s2, s1, 0, max(0, m - 250), band), (s1, s4, 0, 0, band)]
    _check(segs)


@pytest.mark.parametrize("band", [ONE_WAVE - 1, ONE_WAVE, ONE_WAVE + 1, PASS // 2, PASS // 2 + 1])
def test_bands_at_the_tiling_constants(band):
    """2 band + 1 diagonals around one wave's rows and one pass's rows, on pairs a little longer than a pass."""
    rng = np.random.default_rng(band)
    g = bytes(rng.choice(list(b"ACGT"), PASS + 300).tolist())
    t = _mutate(rng, g[100:], 0.12)
    _check([(g, t, 0, -100, band), (t, g, 0, 100, band), (g, t, 0, -100 + band, band)])


def test_ties_and_the_covering_band():
    a, b = b"A" * 500, b"A" * 400
    _check([(a, b, 0, 0, 3), (a, b, 0, -50, 40), (a, b, 0, 0, 1000), (b, a, 1, 37, 0)])
    rng = np.random.default_rng(5)
    segs = []
    for m in (0, 5, 100, 600, 1500, 2100, 4500):
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        t = _mutate(rng, s, 0.12)
        rc = int(rng.integers(0, 2))
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc, int(rng.integers(-30, 30)), max(len(s), len(t)) + 30))
    bases, pairs = _batch(segs)
    banded = mhap_amd.align_pairs_banded(bases, pairs)
    full = mhap_amd.align_pairs(bases, pairs[:, :5])
    assert banded.tolist() == full.tolist()
    assert (banded[1:, 0] > 0).all()


def test_invalid_pairs_are_refused_with_their_index():
    bases = np.frombuffer(b"ACGTACGT", np.uint8)
    ok = [0, 4, 4, 4, 0, 0, 2]
    assert mhap_amd.align_pairs_banded(bases, [ok]).tolist() == [[8, 0, 3, 0, 3, 4, 0]]
    with pytest.raises(mhap_amd.MhapError, match="pair 1"):
        mhap_amd.align_pairs_banded(bases, [ok, [0, 4, 4, 4, 0, 0, -1]])
    with pytest.raises(mhap_amd.MhapError, match="pair 2"):
        mhap_amd.align_pairs_banded(bases, [ok, ok, [0, 4, 6, 4, 0, 0, 2]])


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import mhap_amd
z = np.load(sys.argv[2])
np.save(sys.argv[3], mhap_amd.align_pairs_banded(z["bases"], z["pairs"]))
"""


def test_small_grid_takes_the_one_wave_passes(tmp_path):
    """MHAP_NUM_CUS=2: the persistent grids shrink, every workgroup takes several pairs, and ten tall pairs are enough for the batch to run
    one wave per pair with several passes each; at the full grid the same batch spreads each pair over four waves."""
    rng = np.random.default_rng(9)
    segs = []
    for m in (600, 1100, 1500, 2047, 2048, 2500, 3100, 3700, 4097, 4500, 300, 0, 40):
        s = bytes(rng.choice(list(b"ACGT"), m).tolist())
        st = m // 10
        t = _mutate(rng, s[st:], 0.12)
        rc = int(rng.integers(0, 2))
        segs.append((s, align_ref.rc_bytes(t) if rc else t, rc, -st, int(rng.choice([30, 100, 257]))))
    bases, pairs = _batch(segs)
    np.savez(tmp_path / "in.npz", bases=bases, pairs=pairs)
    env = dict(os.environ, MHAP_NUM_CUS="2")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npy")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    small_grid = np.load(tmp_path / "out.npy")
    full_grid = mhap_amd.align_pairs_banded(bases, pairs)
    assert small_grid.tolist() == full_grid.tolist()
    assert full_grid.tolist() == bref.align_pairs_banded(bases, pairs).tolist()
    assert (full_grid[:10, 0] > 0).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

N_READS, READ_LEN, SEED = 120, 2000, 0x5EA1


@pytest.fixture(scope="module")
def searched():
    fasta = mhap_amd.synth_reads(N_READS, READ_LEN, seed=SEED, coverage=30.0, error_rate=0.15)
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms:
        ms.add_data(fasta)
        recs = ms.find_matches()
        recs = recs[np.lexsort((recs["to_rc"], recs["to_id"], recs["from_id"]))].copy()
        out, detail = mhap_amd.realign_records(recs, fasta, handle=ms)
    return fasta, recs, out, detail


def test_realign_records_equals_plan_and_restatement(searched):
    fasta, recs, out, detail = searched
    k = 64
    assert len(recs) >= k
    pairs = bref.plan(recs[:k], fasta.ids, fasta.offsets, fasta.lengths, 0.2, 0)
    assert mhap_amd.realign_plan(recs[:k], fasta).tolist() == pairs.tolist()
    want, wdetail = bref.to_records(recs[:k], bref.align_pairs_banded(fasta.bases, pairs))
    for q in range(k):
        assert out[q].tolist() == want[q].tolist(), (q, recs[q], out[q], want[q])
    assert detail[:k].tolist() == wdetail.tolist()
    # a given band, and a handle of its own with another max_shift
    out2, _ = mhap_amd.realign_records(recs[:8], fasta, band=25)
    want2, _ = bref.to_records(recs[:8], bref.align_pairs_banded(fasta.bases, bref.plan(recs[:8], fasta.ids, fasta.offsets, fasta.lengths, 0.2, 25)))
    assert out2.tolist() == want2.tolist()
    out3, _ = mhap_amd.realign_records(recs[:8], fasta, max_shift=0.05)
    want3, _ = bref.to_records(recs[:8], bref.align_pairs_banded(fasta.bases, bref.plan(recs[:8], fasta.ids, fasta.offsets, fasta.lengths, 0.05, 0)))
    assert out3.tolist() == want3.tolist()


def _write_fasta(path, fasta):
    with open(path, "w") as fh:
        for i in range(len(fasta)):
            fh.write(f">read{i}\n{fasta.sequence(i)}\n")


def test_driver_and_tool_print_the_realigned_records(searched, tmp_path):
    fasta, recs, out, _ = searched
    path = tmp_path / "reads.fasta"
    _write_fasta(path, fasta)

    def run(extra):
        p = subprocess.run([CLI, "-s", str(path)] + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        return sorted(l for l in p.stdout.split("\n") if l), p.stderr

    plain, err0 = run([])
    assert plain == sorted(mhap_amd.records_to_lines(recs))                       # without the flag: the lines it prints today
    assert "realign" not in err0
    lines, err = run(["--realign"])
    kept = realign_tool.keep(out)
    assert lines == sorted(mhap_amd.records_to_lines(kept))
    assert f"({len(kept)} overlaps kept, {len(recs) - len(kept)} dropped" in err and "Time (s) to realign:" in err
    lines9, _ = run(["--realign", "--realign-min-identity", "0.8", "--realign-band", "40"])
    out40, _ = mhap_amd.realign_records(recs, fasta, band=40)
    assert lines9 == sorted(mhap_amd.records_to_lines(realign_tool.keep(out40, 0.8))) and 0 < len(lines9)
    # the stand-alone tool on the driver's own output
    (tmp_path / "ovl.txt").write_text("\n".join(plain) + "\n")
    p = subprocess.run([sys.executable, "-m", "mhap_amd.realign", str(tmp_path / "ovl.txt"), str(path)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sorted(l for l in p.stdout.split("\n") if l) == lines


def _shared(truth, G, a, b):
    """Genome bases two reads share: their intervals [start, start + span) on the circular genome of length G."""
    s1, e1 = int(truth["start"][a]), int(truth["start"][a] + truth["span"][a])
    s2, e2 = int(truth["start"][b]), int(truth["start"][b] + truth["span"][b])
    return sum(max(0, min(e1, e2 + k) - max(s1, s2 + k)) for k in (-G, 0, G))


def test_realigned_intervals_are_closer_to_the_truth(searched):
    """Over ALL records whose two reads share at least 200 genome bases, the expected overlap length on read A is
    shared x length_A / span_A.  The sum of |reported length - expected| must be smaller after realignment than before; a record that
    came back without an alignment counts with length 0.  (Measured: see EXPERIMENTS.md, "Realignment stage".)"""
    fasta, recs, out, _ = searched
    truth, G = mhap_amd.synth_truth(N_READS, READ_LEN, seed=SEED, coverage=30.0, error_rate=0.15)
    row = {int(i): k for k, i in enumerate(fasta.ids.tolist())}
    sketch_sum = realigned_sum = 0.0
    counted = unaligned = 0
    for r, o in zip(recs, out):
        a, b = row[int(r["from_id"])], row[int(r["to_id"])]
        sh = _shared(truth, G, a, b)
        if sh < 200:
            continue
        expected = sh * float(truth["length"][a]) / float(truth["span"][a])
        counted += 1
        unaligned += int(o["a2"] == 0 and o["a1"] == 0 and o["score"] == 0.0)
        sketch_sum += abs((int(r["a2"]) - int(r["a1"])) - expected)
        realigned_sum += abs((int(o["a2"]) - int(o["a1"])) - expected)
    print(f"\nrealign accuracy: {counted} records (of {len(recs)}), {unaligned} without an alignment; "
          f"sum |length - expected|: sketch {sketch_sum:.1f}, realigned {realigned_sum:.1f}")
    assert counted >= 64          # (a population, not a handful: at least the records the parity test above compares)
    assert realigned_sum < sketch_sum
