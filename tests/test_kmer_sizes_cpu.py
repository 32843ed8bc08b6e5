"""The host side of every k-mer size from 1 to 255 (mhap_create accepts kmer_size and ordered_kmer_size in that range): the hash arithmetic the
kernels share with the host, the second stage's tables at other ordered k-mer sizes, the scratch layout where k and k2 swap which one is larger,
and the refusals just outside the range.  No GPU: the kernels themselves are pinned in test_kmer_sizes_gpu.py."""
import random

import numpy as np
import pytest

import mhap_amd
import oracle_lib as O
from test_host_logic import _RD_MAT, _RD_RAW, _RD_SKIP, _assert_early_reject_table, _expected_sketch_plan, _hash_windows, _sketch_plan


def _hash_string():
    """640 chars: ACGTNRY, a stretch of lower-case bases, and bytes of 0x80 and above (latin-1 chars, UTF-16 code units with a zero high byte)."""
    rnd = random.Random(255)
    s = [rnd.choice("ACGTNRY") for _ in range(640)]
    for i in range(200, 260):
        s[i] = rnd.choice("acgtn")
    for i, c in ((7, "\x80"), (301, "\xff"), (302, "\xe9"), (631, "\x9c")):
        s[i] = c
    return "".join(s)


def test_hash_windows_at_every_kmer_size():
    """murmur128_h1_chars / murmur32_chars (device_common.hpp, compiled for the host) on every window of one string at every k and k2 from 1 to
    255: every tail length of both hashes and up to 31 blocks of the 128-bit one, against the oracle's hashes of the same string."""
    seq = _hash_string()
    assert len(seq) >= 600 and any(c.islower() for c in seq) and any(ord(c) >= 0x80 for c in seq)
    for k in range(1, 256):
        h64, h32 = _hash_windows(seq, k, k)
        assert len(h64) == len(h32) == len(seq) - k + 1
        assert h64.tolist() == O.kmer_hashes64(seq, k).tolist(), k
        assert h32.tolist() == O.kmer_hashes32(seq, k).tolist(), k


@pytest.mark.parametrize("S", [1, 64, 200])
@pytest.mark.parametrize("k2", [1, 2, 7, 12, 13, 64, 255])
def test_early_reject_table_at_other_ordered_kmer_sizes(k2, S):
    """fill_score_table(S, k2) and build_pass_min away from k2 = 12: the same three properties as test_host_logic's test, with every row of
    the identity table compared with the oracle's jaccardToIdentity."""
    _assert_early_reject_table(S, k2, rows=range(S + 1))


@pytest.mark.parametrize("k,k2", [(1, 255), (255, 1), (16, 13), (15, 12), (255, 255)])
def test_scratch_layout_where_k_and_k2_swap(k, k2):
    """layout_group / plan_launch_groups with lengths around k and k2: key_stride = align4(L - k + 1) and h2_stride = align4(L - k2 + 1) each
    follow their own k (at (1, 255) the key arrays are the larger ones, at (255, 1) the 32-bit ones), a read shorter than both has a descriptor
    and no elements, and every read that is not skipped is MHAP_RD_MAT because (k, k2) is not (16, 12)."""
    edges = sorted({x + d for x in (k, k2) for d in (-1, 0, 1) if x + d >= 1} | {1, 2, 300, 1278, 2303})
    rnd = random.Random(1000 * k + k2)
    cases = [(edges, [0] * len(edges), 10**9, 1), (edges, [0] * len(edges), 600, 1), (edges[::-1], [0] * len(edges), 3000, 0)]
    for _ in range(12):
        ls = [rnd.choice(edges) for _ in range(rnd.randrange(1, 30))]
        fl = [(_RD_SKIP if rnd.random() < 0.15 else 0) | (_RD_RAW if rnd.random() < 0.3 else 0) for _ in ls]
        cases.append((ls, fl, rnd.choice((1, 700, 3000, 10**9)), rnd.randrange(2)))
    for ls, fl, gb, fused in cases:
        got = _sketch_plan(ls, fl, k=k, k2=k2, fused=fused, override=gb)
        want = _expected_sketch_plan(ls, fl, gb, k, k2, fused)
        assert got == tuple(want), (ls, fl, gb, fused)
        head, group_of, layout, totals, order = got
        for i, (w, key, h2, nk, nk2, flags) in enumerate(layout):
            assert nk == (max(0, ls[i] - k + 1) + 3) // 4 * 4 and nk2 == (max(0, ls[i] - k2 + 1) + 3) // 4 * 4
            assert bool(flags & _RD_MAT) == (not fl[i] & _RD_SKIP), (i, flags)
        for g, (key_total, h2_total, w_total, _, _, bases) in enumerate(totals):
            idx = [i for i in range(len(ls)) if group_of[i] == g and not fl[i] & _RD_SKIP]
            assert key_total == w_total == sum(2 * layout[i][3] for i in idx)
            assert h2_total == sum(2 * layout[i][4] for i in idx)
            assert bases == sum(ls[i] for i in range(len(ls)) if group_of[i] == g)
        if k != k2 and any(not f & _RD_SKIP and x >= max(k, k2) + 1 for x, f in zip(ls, fl)):
            assert (head[2] > head[3]) == (k < k2), head       # the larger k has the fewer windows


@pytest.mark.parametrize("field,value,message", [("kmer_size", 0, "k-mer size must be in [1,255]"), ("kmer_size", 256, "k-mer size must be in [1,255]"),
                                                 ("ordered_kmer_size", 0, "ordered k-mer size must be in [1,255]"),
                                                 ("ordered_kmer_size", 256, "ordered k-mer size must be in [1,255]")])
def test_kmer_sizes_outside_the_range_are_refused(field, value, message):
    """mhap_create checks its parameters before it touches a device, so the refusal needs no GPU."""
    with pytest.raises(mhap_amd.MhapError) as e:
        mhap_amd.MinHashSearch(mhap_amd.MhapParams(**{field: value}))
    assert str(e.value) == message
