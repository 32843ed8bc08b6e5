"""Case builders of tests/test_group_ranks_gpu.py: data sets, FASTA files, and every expectation — all from the oracle, none from the
library (oracle_lib: O.run_self for self searches, O.minhash / O.ordered / O.overlap over every (query, stored strand) for -q)."""
import functools

import numpy as np

import oracle_lib as O
import mhap_amd
from mhap_amd import FastaData

H, S = 64, 256                      # --num-hashes / --ordered-sketch-size of every case
MIN_OLAP = 116                      # --min-olap-length (default)
FIRST_GROUP_FLOOR = 1 << 20         # ingest_pipeline: the first group's cap is max(group_bases / 4, 2^20) bases


def params(k=16, k2=12):
    return mhap_amd.MhapParams(kmer_size=k, ordered_kmer_size=k2, num_hashes=H, ordered_sketch_size=S, device=0)


def lines(recs):
    return sorted(mhap_amd.records_to_lines(recs))


def with_ids(fa, first_id):
    return FastaData(fa.bases, fa.offsets, fa.lengths, np.arange(len(fa), dtype=np.int64) + first_id)


def empty_reads():
    return FastaData(np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64))


def sequences(fa):
    return [fa.sequence(i) for i in range(len(fa))]


def write_fasta(path, seqs, width=0):
    """One record per sequence, names r0, r1, ...; width > 0 wraps every third record's lines."""
    with open(path, "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(f">r{i}\n")
            if width and i % 3 == 1:
                fh.write("\n".join(s[j:j + width] for j in range(0, len(s), width)) + "\n")
            else:
                fh.write(s + "\n")
    return str(path)


def ingest_groups(lengths, group_bases=256 << 20):
    """The planning rule of ingest_pipeline (mhap_ingest.hip) restated: [lo, hi) of every ingest group over a rank's share.  A group is
    closed in front of the read that would pass its cap, always takes its first read, and holds at most 2^21 reads; the first group's
    cap is max(group_bases / 4, 2^20) bases, every later one's is group_bases."""
    groups, lo, n = [], 0, len(lengths)
    while lo < n:
        cap = max(group_bases >> 2, FIRST_GROUP_FLOOR) if not groups else group_bases
        hi, tot = lo, 0
        while hi < n and (hi == lo or tot + int(lengths[hi]) <= cap) and hi - lo < (1 << 21):
            tot += int(lengths[hi])
            hi += 1
        groups.append((lo, hi))
        lo = hi
    return groups


def self_oracle(fa, k=16, k2=12):
    """O.run_self at the cases' H and S: its dict, plus 'lines' (sorted record lines) and 'sketchable' (reads with a forward sketch)."""
    want = O.run_self(fa, k=k, H=H, k2=k2, S=S, nthreads=8)
    want["lines"] = O.record_lines(want["records"])
    want["sketchable"] = int((want["status"][0::2] == 0).sum())
    return want


def lines_among(want, max_id):
    """The oracle's records between reads with ids <= max_id: a record is a function of its two reads alone (no -f filter here)."""
    r = want["records"]
    return O.record_lines(r[(r["from_id"] <= max_id) & (r["to_id"] <= max_id)])


def query_oracle(index, queries, k=16, k2=12, num_min_matches=3, threshold=0.78, max_shift=0.2):
    """-q (toSelf = false) by brute force from the oracle's primitives, as test_index_vs_stream_mode does, for any k, k2 at the cases' H and
    S: every sketchable query's forward strand against both strands of every sketchable stored read.  A read below --min-olap-length or
    one whose forward sketch fails (no k-mer) is neither stored nor a query; a stored read's reverse strand that fails is dropped alone.
    Query ids must lie above the stored ids (the id rules of MinHashSearch.java:215-219 then never apply).  Sorted record lines."""
    assert len(queries) == 0 or len(index) == 0 or int(queries.ids.min()) > int(index.ids.max())
    ent = []
    for i in range(len(index)):
        s = index.sequence(i)
        if len(s) < MIN_OLAP:
            continue
        for fwd, t in ((1, s), (0, O.rc(s))):
            rc1, mh = O.minhash(t, k, H)
            rc2, od, olen = O.ordered(t, k2, S)
            if rc1 or rc2:
                if fwd:
                    break                                   # the forward sketch failed: the read is dropped
                continue
            ent.append((int(index.ids[i]), fwd, len(s), mh, od, olen))
    table = np.stack([e[3] for e in ent]) if ent else np.zeros((0, H), np.int32)
    want = []
    for qi in range(len(queries)):
        s = queries.sequence(qi)
        if len(s) < MIN_OLAP:
            continue
        rc1, qmh = O.minhash(s, k, H)
        rc2, qo, qlen = O.ordered(s, k2, S)
        if rc1 or rc2:
            continue
        for e in np.nonzero((table == qmh[None, :]).sum(axis=1) >= num_min_matches)[0]:
            mid, fwd, L, _, mo, mlen = ent[int(e)]
            r = O.overlap(qo, qlen, mo, mlen, k2=k2, max_shift=max_shift)
            if r["score"] >= threshold:
                b1, b2 = (r["b1"], r["b2"]) if fwd else (L - r["b2"] - 1, L - r["b1"] - 1)
                want.append(O.format_record({"from_id": int(queries.ids[qi]), "to_id": mid, "score": r["score"], "raw": r["raw"],
                                             "a1": r["a1"], "a2": r["a2"], "alen": len(s), "b1": b1, "b2": b2, "blen": L,
                                             "to_rc": 0 if fwd else 1}))
    return sorted(want)


# ---- the data sets, made once per process and never changed -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_set():
    """450 stored reads of 2 500 bases (1.125 Mbase: one rank's share of it is above 2^20 bases, a third of it is not) and 60 query reads
    of the same genome with the ids behind them: (index, queries, the self oracle of the index)."""
    base = mhap_amd.synth_reads(510, 2500, seed=1201, error_rate=0.06)
    index = with_ids(base.subset(np.arange(0, 450)), 1)
    queries = with_ids(base.subset(np.arange(450, 510)), 451)
    return index, queries, self_oracle(index)


@functools.lru_cache(maxsize=None)
def main_query_lines():
    index, queries, _ = main_set()
    return query_oracle(index, queries)


@functools.lru_cache(maxsize=None)
def long_short_set():
    """600 reads, even ordinals 4 000 bases and odd ordinals 1 000: dealt to two ranks, rank 0's share is 1.2 Mbase and rank 1's 0.3."""
    fa = mhap_amd.synth_reads(600, 4000, seed=1202, error_rate=0.05)
    seqs = [s if i % 2 == 0 else s[:1000] for i, s in enumerate(sequences(fa))]
    fa = FastaData.from_strings(seqs)
    return fa, seqs, self_oracle(fa)


def _interleave(reads, extra):
    """reads[i] followed by extra(i) (a sequence or None)."""
    out = []
    for i, s in enumerate(reads):
        out.append(s)
        x = extra(i)
        if x is not None:
            out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def unsketchable_share_set():
    """400 records for two ranks: the even ordinals are reads, every odd ordinal is below --min-olap-length (100 bases) or shorter than k
    (10 bases), so rank 1's whole share has no sketch."""
    index, _, _ = main_set()
    reads = sequences(index)[:200]
    seqs = _interleave(reads, lambda i: reads[i][:100] if i % 2 == 0 else reads[i][:10])
    fa = FastaData.from_strings(seqs)
    return fa, seqs, self_oracle(fa)


@functools.lru_cache(maxsize=None)
def ragged_set():
    """253 records, not a multiple of 3 or 4: 205 reads with a 100-base record behind every 7th and a 10-base one behind every 11th."""
    index, _, _ = main_set()
    reads = sequences(index)[:205]
    seqs = []
    for i, s in enumerate(reads):
        seqs.append(s)
        if i % 7 == 3:
            seqs.append(s[:100])
        if i % 11 == 5:
            seqs.append(s[:10])
    fa = FastaData.from_strings(seqs)
    return fa, self_oracle(fa)


@functools.lru_cache(maxsize=None)
def overlapping_pair():
    """Two reads of the main set that the oracle reports as overlapping, as a data set of their own (ids 1, 2), and its self oracle."""
    index, _, want = main_set()
    r = want["records"][0]
    pair = FastaData.from_strings([index.sequence(int(r["to_id"]) - 1), index.sequence(int(r["from_id"]) - 1)])
    return pair, self_oracle(pair)


@functools.lru_cache(maxsize=None)
def edge_queries():
    """23 queries against the main index: 20 of the query reads, one of them again with IUPAC codes in it (a raw-byte read), one shorter
    than k and one below --min-olap-length: (queries, expected lines)."""
    index, queries, _ = main_set()
    seqs = sequences(queries)[:20]
    iupac = seqs[4][:300] + "NRYKM" + seqs[4][305:]
    seqs = seqs[:7] + ["ACGTACGTAC"] + seqs[7:13] + [seqs[2][:100]] + seqs[13:] + [iupac]
    q = FastaData.from_strings(seqs, id_offset=len(index))
    return q, query_oracle(index, q)


@functools.lru_cache(maxsize=None)
def kmer_set():
    """300 stored reads and 60 queries at 4 % error for the other k-mer sizes: (index, queries)."""
    base = mhap_amd.synth_reads(360, 2500, seed=1203, error_rate=0.04)
    return with_ids(base.subset(np.arange(0, 300)), 1), with_ids(base.subset(np.arange(300, 360)), 301)


@functools.lru_cache(maxsize=None)
def kmer_oracles(k, k2):
    index, queries = kmer_set()
    return self_oracle(index, k, k2), query_oracle(index, queries, k, k2)
