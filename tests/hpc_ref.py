"""The "homopolymer compression" section of include/mhap_hip.h restated in numpy: heads, the compressed read, its map start[], the
counts, lo / hi and a record's expansion.  Written from the prose, read by the tests of the host rule (test_hpc_cpu.py), of the
kernels (test_hpc_gpu.py) and of the drivers (test_hpc_cli_gpu.py)."""
import numpy as np

from mhap_amd import api

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "CG", "at", "cg"):
    _COMP[ord(_a)], _COMP[ord(_b)] = ord(_b), ord(_a)


def revcomp(x):
    """The reverse complement of a read's bytes (A<->T, C<->G, every other byte itself)."""
    return _COMP[np.asarray(x, np.uint8)[::-1]]


def compress_read(x):
    """(head bytes, start): position p is a head iff p = 0 or x[p] != x[p - 1]; start holds the heads' positions and then len(x)."""
    x = np.asarray(x, np.uint8)
    head = np.ones(len(x), bool)
    head[1:] = x[1:] != x[:-1]
    pos = np.flatnonzero(head)
    return x[pos], np.concatenate([pos, [len(x)]]).astype(np.int32)


def compress(fasta):
    """Every read of a FastaData compressed: a dict of cbases, coff (n + 1), clen, starts (read r's map at coff[r] + r), the counts
    (api.HPC_COUNTS) and fasta, the compressed reads under the same ids."""
    n = len(fasta)
    cb, st = [], []
    clen = np.zeros(n, np.int32)
    long_runs = longest = 0
    for r in range(n):
        o, L = int(fasta.offsets[r]), int(fasta.lengths[r])
        c, s = compress_read(fasta.bases[o:o + L])
        cb.append(c)
        st.append(s)
        clen[r] = len(c)
        if len(c):
            runs = np.diff(s)
            long_runs += int((runs > 1).sum())
            longest = max(longest, int(runs.max()))
    coff = np.zeros(n + 1, np.int64)
    np.cumsum(clen, out=coff[1:])
    cbases = np.concatenate(cb).astype(np.uint8) if n else np.zeros(0, np.uint8)
    starts = np.concatenate(st).astype(np.int32) if n else np.zeros(0, np.int32)
    counts = dict(zip(api.HPC_COUNTS, [n, int(np.asarray(fasta.lengths, np.int64).sum()), int(coff[n]), long_runs, longest,
                                       int((np.asarray(fasta.lengths) == 0).sum())]))
    return dict(cbases=cbases, coff=coff, clen=clen, starts=starts, counts=counts,
                fasta=api.FastaData(cbases, coff[:n], clen, fasta.ids), raw_lengths=np.asarray(fasta.lengths, np.int32))


def start_of(ref, r):
    o = int(ref["coff"][r]) + r
    return ref["starts"][o:o + int(ref["clen"][r]) + 1]


def lo(start, p):
    clen = len(start) - 1
    return -1 if p < 0 else int(start[p]) if p < clen else int(start[clen])


def hi(start, p):
    clen = len(start) - 1
    return -1 if p < 0 else int(start[p + 1]) - 1 if p < clen else int(start[clen])


def expand_record(rec, start_from, start_to):
    """One record through two maps: a copy with a1, a2, alen, b1, b2, blen rewritten."""
    out = np.array(rec, dtype=api.RECORD_DTYPE).reshape(1).copy()
    out["a1"], out["a2"], out["alen"] = lo(start_from, int(rec["a1"])), hi(start_from, int(rec["a2"])), int(start_from[-1])
    out["b1"], out["b2"], out["blen"] = lo(start_to, int(rec["b1"])), hi(start_to, int(rec["b2"])), int(start_to[-1])
    return out[0]


def expand(records, ref_from, ref_to=None):
    """Records whose `from` reads are those of ref_from and whose `to` reads those of ref_to (None: the same), looked up by id; of two
    reads with one id the first counts."""
    ref_to = ref_from if ref_to is None else ref_to
    rows = []
    for ref in (ref_from, ref_to):
        by_id = {}
        for r, i in enumerate(np.asarray(ref["fasta"].ids).tolist()):
            by_id.setdefault(i, r)
        rows.append(by_id)
    out = np.zeros(len(records), api.RECORD_DTYPE)
    for q, rec in enumerate(records):
        out[q] = expand_record(rec, start_of(ref_from, rows[0][int(rec["from_id"])]), start_of(ref_to, rows[1][int(rec["to_id"])]))
    return out
