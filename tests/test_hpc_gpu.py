"""Homopolymer compression on the GPU (hpc_kernels.hip) against tests/hpc_ref.py, byte for byte: the compressed reads, coff, clen,
the maps and the counts on crafted reads at every edge of the kernels' shapes (16 bytes per lane, 64 lanes per wave, MHAP_HPC_TILE
positions per workgroup, MHAP_HPC_SCAN_BLOCK tile counts per scan block, groups of reads), the refusals, the records expanded on the
device, and the whole path on the noisy reads of the motivating figure: compress, search, expand, plan."""
import numpy as np
import pytest

import mhap_amd
from mhap_amd import api, hpc

import hpc_cases as hc
import hpc_ref as ref
import oracle_lib as O

pytestmark = pytest.mark.gpu
T, B = api.HPC_TILE, api.HPC_SCAN_BLOCK


@pytest.fixture(scope="module")
def ms():
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as h:
        yield h


def _check(hp, fasta):
    """Everything an HpcReads holds against the restatement; returns the restatement."""
    want = ref.compress(fasta)
    n = len(fasta)
    assert hp.counts == want["counts"]
    assert hp.fasta.lengths.dtype == np.int32 and hp.fasta.lengths.tobytes() == want["clen"].tobytes()
    assert hp.fasta.offsets.tobytes() == want["coff"][:n].tobytes()
    assert hp.fasta.bases.tobytes() == want["cbases"].tobytes()
    assert hp.starts.dtype == np.int32 and hp.starts.tobytes() == want["starts"].tobytes()
    assert hp.start_offsets.tolist() == (want["coff"][:n] + np.arange(n)).tolist()
    assert hp.fasta.ids.tolist() == np.asarray(fasta.ids).tolist() and hp.raw_lengths.tolist() == np.asarray(fasta.lengths).tolist()
    return want


def test_crafted_reads(ms):
    fa = hc.crafted_table(T)
    assert set(fa.lengths.tolist()) >= {0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1} and (np.diff(fa.offsets) < 0).any()
    with hpc.compress(fa, handle=ms) as hp:
        want = _check(hp, fa)
        for r in (0, len(fa) // 2, len(fa) - 1):
            assert hp.start_of(r).tolist() == ref.start_of(want, r).tolist()
    assert want["counts"]["longest_run"] == 3 * T + 2 and want["counts"]["empty_reads"] == 2


def test_more_tiles_than_a_scan_block(ms):
    fa = hc.scan_table(T, B)
    assert int(((fa.lengths.astype(np.int64) + T - 1) // T).sum()) == 2 * B + 1
    with hpc.compress(fa, handle=ms) as hp:
        _check(hp, fa)


def test_groups_do_not_change_the_result(ms):
    fa = hc.group_table(T)
    with hpc.compress(fa, handle=ms) as one, hpc.compress(fa, handle=ms, group_bases=3 * T) as many:
        _check(one, fa)
        _check(many, fa)
        assert many.starts.tobytes() == one.starts.tobytes() and many.fasta.bases.tobytes() == one.fasta.bases.tobytes()
    with hpc.compress(fa, handle=ms, group_bases=1) as each:   # every read a group of its own, the empty ones too
        _check(each, fa)


def test_no_reads_and_only_empty_reads(ms):
    for seqs in ([], [np.zeros(0, np.uint8)] * 3):
        fa = hc.table(seqs)
        with hpc.compress(fa, handle=ms) as hp:
            _check(hp, fa)
            assert hp.starts.tolist() == [0] * len(seqs)


def test_refusals(ms):
    fa = hc.table([hc.alternating(40), hc.alternating(30)])
    for offsets, lengths, word in (([0, 41], [40, 30], "read 1"), ([0, 40], [40, -1], "read 1"), ([-1, 40], [40, 30], "read 0"),
                                   ([0, 71], [40, 0], "read 1")):
        bad = api.FastaData(fa.bases, offsets, lengths, fa.ids)
        with pytest.raises(api.MhapError, match=word):
            hpc.compress(bad, handle=ms)
    with pytest.raises(api.MhapError, match="group_bases"):
        hpc.compress(fa, handle=ms, group_bases=(1 << 30) + 1)
    with hpc.compress(fa, handle=ms) as hp:
        ok = hc.rec(1, 2, 0, 39, 40, 0, 29, 30, 0)
        assert hp.expand(np.array([ok], api.RECORD_DTYPE))[0]["alen"] == 40
        assert len(hp.expand(np.zeros(0, api.RECORD_DTYPE))) == 0
        for change, word in ((dict(to_id=7), "record 1 names read 7"), (dict(from_id=9), "record 1 names read 9"), (dict(alen=39), "record 1 gives read 1"),
                             (dict(blen=31), "record 1 gives read 2")):
            recs = np.array([ok, ok], api.RECORD_DTYPE)
            for k, v in change.items():
                recs[1][k] = v
            with pytest.raises(api.MhapError, match=word):
                hp.expand(recs)


def test_expand_records_against_the_restatement(ms):
    rng = np.random.default_rng(11)
    a, _ = hc.noisy_reads(0.2, seed=3, n=6, length=600, genome=3000)
    odd = [np.zeros(0, np.uint8), np.frombuffer(b"A", np.uint8), np.frombuffer(b"AAAAAAA", np.uint8), hc.alternating(50),
           hc.runs_of(rng, 300, [ord("N"), ord("a"), ord("A"), 0, 255])]
    b = hc.table(odd, ids=np.arange(101, 101 + len(odd), dtype=np.int64))
    ra, rb = ref.compress(a), ref.compress(b)
    with hpc.compress(a, handle=ms) as ha, hpc.compress(b, handle=ms) as hb:
        same = hc.random_records(np.random.default_rng(2), ra, ra, 700)       # more than two workgroups of lanes
        assert ha.expand(same).tobytes() == ref.expand(same, ra).tobytes()
        two = hc.random_records(np.random.default_rng(3), ra, rb, 700)
        got = ha.expand(two, to=hb)
        assert got.tobytes() == ref.expand(two, ra, rb).tobytes()
        assert api.realign_plan(got, a, query_fasta=b).shape == (700, 7)
        back = hc.random_records(np.random.default_rng(4), rb, ra, 300)
        assert hb.expand(back, to=ha).tobytes() == ref.expand(back, rb, ra).tobytes()


def test_end_to_end_on_the_noisy_reads():
    """Compressed on the GPU, searched on the GPU, expanded on the GPU: the oracle's records on the restated compression, carried to raw
    coordinates by the restatement; every true pair is among them and the realignment's planner takes them all."""
    fa, true = hc.noisy_reads(0.2, seed=20261020)
    want_c = ref.compress(fa)
    oracle = O.run_self(want_c["fasta"], nthreads=4)["records"]
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams()) as ms, hpc.compress(fa, handle=ms) as hp:
        _check(hp, fa)
        ms.add_data(hp.fasta)
        recs = ms.find_matches()
        assert sorted(api.records_to_lines(recs)) == O.record_lines(oracle) and len(recs) >= len(true)
        raw = hp.expand(recs)
    want = ref.expand(oracle.astype(api.RECORD_DTYPE), want_c)
    assert sorted(api.records_to_lines(raw)) == sorted(api.records_to_lines(want))
    assert true <= hc.pairs_of(raw)
    assert (raw["alen"] == fa.lengths[raw["from_id"] - 1]).all() and (raw["blen"] == fa.lengths[raw["to_id"] - 1]).all()
    assert api.realign_plan(raw, fa).shape == (len(raw), 7)
