#!/usr/bin/env python
"""Cost of compacting the string graph into unitigs and of spelling them, next to the finish they follow.

    python tools/unitig_bench.py [--reads 1000000] [--spell-reads 100000] [--length 6000] [--repeats 5] > profiles/unitig_bench.txt
    python tools/unitig_bench.py --config c2        # the graph of one C2-shaped search instead of the fabricated chain

The fabricated layout is one chain of --reads reads of 20 000 positions (no bases are needed): the worst case for list ranking, every
read on one unitig.  The spelling is timed on a chain of --spell-reads reads of --length drawn bases, each overlapping the next by
about half, with the bases already on the device (mhap_graph_spell_device); its output goes to the host, so a device-to-device and a
device-to-host copy of the output's size are timed beside it.  Times are host clocks around calls that end in a synchronise, the
first pass being the warm-up.  A run without a GPU fails: there is no fallback."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mhap_amd  # noqa: E402
from mhap_amd import api  # noqa: E402
from mhap_amd import workloads as W  # noqa: E402
from mhap_amd.graph import counts_line  # noqa: E402
from mhap_amd.realign import kept_rows  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:.2f} ms (min {ts[0] * 1e3:.2f}, max {ts[-1] * 1e3:.2f}, n = {len(ts)})"


def chain_records(n, length, rng):
    """The dovetails read i -> read i + 1 of n reads of one length, arc lengths drawn in [length / 4, length / 2]."""
    recs = np.zeros(max(n - 1, 0), api.RECORD_DTYPE)
    ln = rng.integers(length // 4, length // 2 + 1, len(recs)).astype(np.int32)
    recs["from_id"], recs["to_id"] = np.arange(1, n), np.arange(2, n + 1)
    recs["score"], recs["a1"], recs["a2"], recs["alen"] = 0.9, ln, length - 1, length
    recs["b1"], recs["b2"], recs["blen"] = 0, length - ln - 1, length
    return recs


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def run(ms, ids, lengths, recs, repeats, label):
    """finish and unitigs of one session, repeated; returns the session's last unitig counts."""
    t_finish, t_unitigs = [], []
    gc, uc = np.zeros(len(api.GRAPH_COUNTS), np.int64), np.zeros(len(api.UNITIG_COUNTS), np.int64)
    with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
        for part in np.array_split(recs, 8):
            gs.add(part)
        ms.synchronize()
        for rep in range(max(3, repeats) + 1):
            tf = timed(lambda: ms._chk(gs._lib.mhap_graph_finish(gs._s, api._ptr(gc))))
            tu = timed(lambda: ms._chk(gs._lib.mhap_graph_unitigs(gs._s, api._ptr(uc))))
            if rep:
                t_finish.append(tf)
                t_unitigs.append(tu)
    print(f"{label}: {len(ids)} reads, {len(recs)} records")
    print(counts_line(dict(zip(api.GRAPH_COUNTS, gc.tolist()))))
    print(api.unitig_counts_line(uc))
    print(f"mhap_graph_finish:  {spread(t_finish)}")
    print(f"mhap_graph_unitigs: {spread(t_unitigs)}")


def run_spell(ms, n, length, repeats):
    import torch
    rng = np.random.default_rng(3)
    ids, lengths = np.arange(1, n + 1, dtype=np.int64), np.full(n, length, np.int32)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * length)]
    offsets = np.arange(n, dtype=np.int64) * length
    d_bases = torch.from_numpy(bases).cuda()
    uc = np.zeros(len(api.UNITIG_COUNTS), np.int64)
    t_spell, t_d2d, t_d2h = [], [], []
    with mhap_amd.GraphSession(ids, lengths, handle=ms) as gs:
        gs.add(chain_records(n, length, rng))
        gs.finish()
        ms._chk(gs._lib.mhap_graph_unitigs(gs._s, api._ptr(uc)))
        total = int(uc[api.UNITIG_COUNTS.index("total_bases")])
        out = np.zeros(total, np.uint8)
        src, dst, host = d_bases[:total], torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8)
        torch.cuda.synchronize()
        for rep in range(max(3, repeats) + 1):
            ts = timed(lambda: ms._chk(gs._lib.mhap_graph_spell_device(gs._s, C.c_void_p(d_bases.data_ptr()), C.c_int64(len(bases)),
                                                                          api._ptr(offsets), api._ptr(out))))
            tc = timed(lambda: (dst.copy_(src), torch.cuda.synchronize()))
            th = timed(lambda: (host.copy_(dst), torch.cuda.synchronize()))
            if rep:
                t_spell.append(ts)
                t_d2d.append(tc)
                t_d2h.append(th)
    print(f"spelling: a chain of {n} reads x {length} bases, {total / 1e6:.1f} MB of unitig sequence")
    print(api.unitig_counts_line(uc))
    print(f"mhap_graph_spell_device (kernel and the output down): {spread(t_spell)}")
    print(f"device-to-device copy of the output's size:           {spread(t_d2d)}")
    print(f"device-to-host copy of the output's size (pageable):  {spread(t_d2h)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--spell-reads", type=int, default=100000)
    ap.add_argument("--length", type=int, default=6000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", default=None, help="a workload of mhap_amd.workloads (c2): search, realign and time its graph instead")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("unitig_bench: no GPU")
    if a.config:
        fasta = W.config_reads(a.config)
        with mhap_amd.MinHashSearch(W.params_for(a.config)) as ms:
            ms.add_data(fasta)
            out, _ = mhap_amd.realign_records(ms.find_matches(), fasta, handle=ms)
            run(ms, fasta.ids, fasta.lengths, out[kept_rows(out)], a.repeats, f"{a.config}-shaped search")
        return
    with mhap_amd.MinHashSearch(mhap_amd.MhapParams(num_hashes=1, ordered_sketch_size=1)) as ms:
        rng = np.random.default_rng(1)
        run(ms, np.arange(1, a.reads + 1, dtype=np.int64), np.full(a.reads, 20000, np.int32), chain_records(a.reads, 20000, rng), a.repeats,
            "fabricated chain")
        run_spell(ms, a.spell_reads, a.length, a.repeats)


if __name__ == "__main__":
    main()
