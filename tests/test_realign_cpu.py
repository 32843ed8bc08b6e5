"""The realignment stage without a GPU: the banded restatement against the full one, mhap_realign_plan against the Python plan, and the
driver's refusals (tests/align_banded_ref.py restates the contract of include/mhap_hip.h)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
import align_ref  # noqa: E402
import align_banded_ref as bref  # noqa: E402

CLI = os.path.join(ROOT, "mhap_amd", "lib", "mhap-hip")


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


def _pairs(seed, count, max_len=400):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(rng.integers(1, max_len))
        s = bytes(rng.choice(list(b"ACGT"), n).tolist())
        t = _mutate(rng, s[int(rng.integers(0, max(1, n // 3))):], rng.uniform(0, 0.2))
        yield rng, s, t


def test_covering_band_equals_the_full_restatement():
    for rng, s, t in _pairs(11, 12):
        if not t:
            continue
        cover = max(len(s), len(t))
        for diag in (0, int(rng.integers(-50, 50))):
            assert bref.align_banded(s, t, diag, cover + abs(diag)) == align_ref.align(s, t), (s, t, diag)
    assert bref.align_banded(b"ACGT", b"ACGT", 0, 0) == (8, 0, 3, 0, 3, 4, 0)


def test_score_never_decreases_as_the_band_widens():
    for rng, s, t in _pairs(12, 8):
        if not t:
            continue
        diag = int(rng.integers(-20, 20))
        scores = [bref.align_banded(s, t, diag, w)[0] for w in (0, 1, 2, 5, 17, 60, 200, 1000)]
        assert scores == sorted(scores), scores
        assert scores[-1] == align_ref.align(s, t)[0]


def test_band_off_the_matrix_and_empty_segments_are_empty():
    s, t = b"ACGTACGTAC", b"ACGTACG"
    assert bref.align_banded(s, t, len(t) + 3, 3) == bref.NONE       # right of the last column: j - i <= n - 1
    assert bref.align_banded(s, t, -len(s) - 3, 3) == bref.NONE      # below the last row
    assert bref.align_banded(b"", t, 0, 5) == bref.NONE and bref.align_banded(s, b"", 0, 5) == bref.NONE
    assert bref.align_banded(s, t, 10 ** 9, 5) == bref.NONE
    # a band of one diagonal sees exactly that diagonal: the last base of s against the first of t
    assert bref.align_banded(b"CCCA", b"AGGG", -3, 0) == (2, 3, 3, 0, 0, 1, 0)


def _reads(lengths, first_id=1):
    lengths = np.asarray(lengths, np.int32)
    offsets = np.zeros(len(lengths), np.int64)
    offsets[1:] = np.cumsum(lengths[:-1])
    return np.arange(first_id, first_id + len(lengths), dtype=np.int64), offsets, lengths


def _rec(from_id, to_id, a1, a2, alen, b1, b2, blen, to_rc):
    r = np.zeros(1, api.RECORD_DTYPE)
    r[0] = (from_id, to_id, 0.9, 55.0, a1, a2, alen, b1, b2, blen, to_rc, 0)
    return r


def _lib_plan(recs, ids, offsets, lengths, max_shift, band):
    lib = mhap_amd.load_library()
    recs = np.ascontiguousarray(recs, api.RECORD_DTYPE)
    out = np.zeros((len(recs), 7), np.int64)
    rc = lib.mhap_realign_plan(api._ptr(recs), C.c_int64(len(recs)), api._ptr(ids), api._ptr(offsets), api._ptr(lengths),
                               C.c_int64(len(ids)), C.c_double(max_shift), C.c_int32(band), api._ptr(out))
    return rc, out, lib.mhap_realign_plan_error().decode()


def test_plan_equals_the_python_plan_on_crafted_records():
    ids, offsets, lengths = _reads([1000, 2500, 800, 40], first_id=7)
    ids = ids[::-1].copy()                      # ids in no particular order: reads are found by id, not by position
    recs = np.concatenate([
        _rec(10, 9, 100, 900, 1000, 0, 810, 2500, 0),        # ids[0] = 10 is the 1000-base read; forward, negative diagonal
        _rec(10, 9, 0, 500, 1000, 1900, 2499, 2500, 0),      # forward, positive diagonal
        _rec(10, 9, 100, 900, 1000, 0, 810, 2500, 1),        # to_rc: the interval is flipped back first
        _rec(9, 8, 11, 700, 2500, 0, 600, 800, 1),           # odd coordinate sum on a negative diagonal: the floor
        _rec(9, 8, 10, 700, 2500, 1, 600, 800, 0),           # odd sum again, other parity mix
        _rec(8, 9, 0, 600, 800, 1500, 2101, 2500, 0),        # odd sum on a positive diagonal
        _rec(7, 10, 0, 39, 40, 500, 539, 1000, 1),
        _rec(10, 10, 0, 999, 1000, 0, 999, 1000, 0),
    ])
    for max_shift in (0.2, 0.05, 1.0, 0.0, -0.5, 0.0013):
        rc, got, msg = _lib_plan(recs, ids, offsets, lengths, max_shift, 0)
        assert rc == 0, msg
        want = bref.plan(recs, ids, offsets, lengths, max_shift, 0)
        assert got.tolist() == want.tolist(), max_shift
        if max_shift <= 0:
            assert (got[:, 6] == 1).all()
    rc, got, _ = _lib_plan(recs, ids, offsets, lengths, 0.2, 37)
    assert rc == 0 and got.tolist() == bref.plan(recs, ids, offsets, lengths, 0.2, 37).tolist() and (got[:, 6] == 37).all()
    # spelled out once: record 3 is to_rc with b = [0, 600] of 800 -> b' = [199, 799]; diag = floor((998 - 711) / 2) = 143; and a
    # negative odd sum floors away from zero: record 0 has (0 + 810) - (100 + 900) = -190 -> -95, record 4 (601 - 710) = -109 -> -55
    assert got[3, 4] == 1 and got[3, 5] == 143 and got[0, 5] == -95 and got[4, 5] == -55
    assert got[0, :4].tolist() == [int(offsets[0]), 1000, int(offsets[1]), 2500]
    assert api.realign_plan(recs, api.FastaData(np.zeros(int(lengths.sum()), np.uint8), offsets, lengths, ids), band=37).tolist() == got.tolist()


def test_plan_refuses_unknown_ids_and_wrong_lengths():
    ids, offsets, lengths = _reads([1000, 2500])
    good = _rec(1, 2, 0, 10, 1000, 0, 10, 2500, 0)
    for bad, word in ((_rec(1, 3, 0, 10, 1000, 0, 10, 2500, 0), "read 3"), (_rec(5, 2, 0, 10, 1000, 0, 10, 2500, 0), "read 5"),
                      (_rec(1, 2, 0, 10, 999, 0, 10, 2500, 0), "length 999"), (_rec(1, 2, 0, 10, 1000, 0, 10, 2501, 0), "length 2501")):
        rc, _, msg = _lib_plan(np.concatenate([good, bad]), ids, offsets, lengths, 0.2, 0)
        assert rc == -1 and "record 1" in msg and word in msg, msg           # MHAP_E_INVALID, naming the record
        with pytest.raises(ValueError):
            bref.plan(np.concatenate([good, bad]), ids, offsets, lengths)
    rc, _, msg = _lib_plan(good, ids, offsets, lengths, 0.2, -1)
    assert rc == -1 and msg
    with pytest.raises(mhap_amd.MhapError):
        api.realign_plan(_rec(1, 9, 0, 10, 1000, 0, 10, 2500, 0), api.FastaData(np.zeros(3500, np.uint8), offsets, lengths, ids))


def test_record_conversion_restatement():
    recs = np.concatenate([_rec(1, 2, 5, 50, 100, 7, 60, 200, 0), _rec(1, 2, 5, 50, 100, 7, 60, 200, 1), _rec(1, 2, 5, 50, 100, 7, 60, 200, 1)])
    out, detail = bref.to_records(recs, [(180, 3, 98, 10, 108, 100, 5), (180, 3, 98, 10, 108, 100, 5), (0, -1, -1, -1, -1, 0, 0)])
    assert (out[0]["a1"], out[0]["a2"], out[0]["b1"], out[0]["b2"]) == (3, 98, 10, 108) and out[0]["score"] == 0.95
    assert (out[1]["b1"], out[1]["b2"]) == (200 - 108 - 1, 200 - 10 - 1)
    assert (out[2]["a1"], out[2]["a2"], out[2]["b1"], out[2]["b2"], out[2]["score"]) == (0, 0, 0, 0, 0.0) and detail[2].tolist() == [0, 0, 0]
    assert out[0]["raw"] == 55.0 and detail[0].tolist() == [180, 100, 5]


def test_driver_lists_the_realign_flags():
    p = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for flag in ("--realign,", "--realign-band,", "--realign-min-identity,"):
        assert "\t" + flag in p.stdout, flag


def test_driver_refuses_realign_without_bases_or_on_several_gpus(tmp_path):
    fa = tmp_path / "reads.fasta"
    fa.write_text(">r1\nACGTACGTACGT\n")
    dat = tmp_path / "reads.dat"
    dat.write_bytes(b"")
    p = subprocess.run([CLI, "-s", str(dat), "--realign"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--realign needs the reads' bases" in p.stdout and p.stdout.count("\n") == 1, (p.stdout, p.stderr[-500:])
    p = subprocess.run([CLI, "-s", str(fa), "-q", str(dat), "--realign"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--realign needs the reads' bases" in p.stdout
    for extra in (["--gpus", "2"], ["--devices", "0,1"]):
        p = subprocess.run([CLI, "-s", str(fa), "--realign"] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--realign runs on one GPU" in p.stdout and p.stdout.count("\n") == 1, (p.stdout, p.stderr[-500:])


def test_realign_tool_parses_and_refuses_named_ids(tmp_path):
    from mhap_amd import realign
    good = tmp_path / "ovl.txt"
    good.write_text("1 2 0.100000 55.000000 0 5 50 100 1 7 60 200\n")
    recs = realign.read_overlaps(str(good))
    assert len(recs) == 1 and recs[0]["to_rc"] == 1 and recs[0]["blen"] == 200 and recs[0]["raw"] == 55.0 and abs(recs[0]["score"] - 0.9) < 1e-12
    named = tmp_path / "named.txt"
    named.write_text("readA readB 0.100000 55.000000 0 5 50 100 1 7 60 200\n")
    with pytest.raises(mhap_amd.MhapError, match="--store-full-id"):
        realign.read_overlaps(str(named))
