"""CPU restatement of the read-correction contract (include/mhap_hip.h, "read correction"): the two views of a realigned record, the
22 counters per target position, the 65 535-view cap and the call.  Written from the header's prose, column by column, in plain Python
over numpy arrays; nothing here follows the kernels' layout or schedule.

    c = Consensus(reads, ids)                 # reads: bytes per read; ids: the ids the records name
    c.add(records, op_offsets, ops)           # what realign_records_paths returned (or records_from_results + the aligner's runs)
    seqs, stats = c.call(min_cov=4)           # corrected bytes per read, int32 (n, 6) {len_in, len_out, n_sub, n_del, n_ins, n_low}
    c.votes[r]                                # int64 (len, 24): base A C G T, del, span, ins[k][A C G T] for k = 0 .. 3, two spare

A view is a list of columns in increasing target order: ("M", t, e), ("Del", t) or ("Ins", e); add_view takes one directly."""
import numpy as np

from align_ref import rc_bytes

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
KI = 4
CAP = 65535
RUN_MAX = (1 << 28) - 1                   # the longest run of a path; a longer one is split into several of its code
NCOUNT = 24
DEL, SPAN, INS0 = 4, 5, 6
ACGT = b"ACGT"


def complement(e):
    """One byte through the aligner's table (Utils.rc): a byte the table does not change stays what it is."""
    return rc_bytes(bytes([e]))[0]


def views_of(s1, s2, i0, j0, runs, to_rc, blen):
    """(view A, view B) of one realigned record.  s1: read A; s2: read B as the aligner saw it (reverse-complemented when to_rc);
    (i0, j0): the path's first row and column; runs: len << 4 | code."""
    a, b = [], []
    i, j = i0, j0
    for r in runs:
        length, code = int(r) >> 4, int(r) & 15
        for _ in range(length):
            if code in (OP_EQ, OP_X):
                a.append(("M", i, s2[j]))
                b.append(("M", j, s1[i]))
                i, j = i + 1, j + 1
            elif code == OP_I:            # consumes s1 only
                a.append(("Del", i))
                b.append(("Ins", s1[i]))
                i += 1
            elif code == OP_D:            # consumes s2 only
                a.append(("Ins", s2[j]))
                b.append(("Del", j))
                j += 1
            else:
                raise ValueError(f"run code {code}")
    if to_rc:
        turned = []
        for col in reversed(b):
            if col[0] == "M":
                turned.append(("M", blen - 1 - col[1], complement(col[2])))
            elif col[0] == "Del":
                turned.append(("Del", blen - 1 - col[1]))
            else:
                turned.append(("Ins", complement(col[1])))
        b = turned
    return a, b


def tally(view):
    """The (t, counter) increments of one view, one entry per vote."""
    out = []
    t_prev, k = None, 0
    for col in view:
        if col[0] == "Ins":
            assert t_prev is not None, "a view begins with a target-consuming column"
            if k < KI and col[1] in ACGT:
                out.append((t_prev, INS0 + 4 * k + ACGT.index(col[1])))
            k += 1                        # any byte takes its slot
            continue
        t = col[1]
        if t_prev is not None:
            assert t > t_prev, "target order"
            out.append((t_prev, SPAN))    # two consecutive target-consuming columns t_prev, t
        if col[0] == "M":
            if col[2] in ACGT:
                out.append((t, ACGT.index(col[2])))
        else:
            out.append((t, DEL))
        t_prev, k = t, 0
    return out


class Consensus:
    def __init__(self, reads, ids):
        self.reads = [bytes(r) for r in reads]
        self.row = {}
        for k, i in enumerate(ids):
            self.row.setdefault(int(i), k)
        self.votes = [np.zeros((len(r), NCOUNT), np.int64) for r in self.reads]
        self.views = [0] * len(self.reads)
        self.skipped_views = 0
        self._memo = {}

    def add_view(self, target, view):
        """One view on read `target` (its position among the reads), through the cap."""
        self._apply(target, tally(view))

    def _apply(self, target, incs):
        if self.views[target] >= CAP:
            self.skipped_views += 1
            return
        self.views[target] += 1
        if len(incs):
            arr = incs if isinstance(incs, np.ndarray) else np.array(incs, np.int64).reshape(-1, 2)
            np.add.at(self.votes[target], (arr[:, 0], arr[:, 1]), 1)

    def add(self, records, op_offsets, ops):
        # refused before any vote: two adjacent runs of one code unless the earlier is a run split at 2^28 - 1
        ops, starts = np.asarray(ops, np.int64), np.asarray(op_offsets, np.int64)
        same = ((ops[:-1] & 15) == (ops[1:] & 15)) & (ops[:-1] >> 4 != RUN_MAX)
        firsts = starts[(starts > 0) & (starts < len(ops))]
        same[firsts - 1] = False                                            # the last run of one record and the first of the next
        for u in np.flatnonzero(same).tolist():
            q = int(np.searchsorted(starts, u, side="right")) - 1          # the record of run u
            if int(records[q]["from_id"]) != int(records[q]["to_id"]):
                raise ValueError(f"record {q} has runs {u - int(starts[q])} and {u + 1 - int(starts[q])} of one code, and the earlier is "
                                 "not a run split at 2^28 - 1 columns")
        for q in range(len(records)):
            rec = records[q]
            runs = tuple(int(x) for x in ops[int(op_offsets[q]):int(op_offsets[q + 1])])
            fid, tid = int(rec["from_id"]), int(rec["to_id"])
            if not runs or fid == tid:
                continue
            ia, ib = self.row[fid], self.row[tid]
            s1, sb = self.reads[ia], self.reads[ib]
            assert len(s1) == int(rec["alen"]) and len(sb) == int(rec["blen"])
            to_rc = int(rec["to_rc"]) != 0
            blen = len(sb)
            i0 = int(rec["a1"])
            j0 = blen - int(rec["b2"]) - 1 if to_rc else int(rec["b1"])
            key = (ia, ib, i0, j0, to_rc, runs)
            if key not in self._memo:      # (the same record again: the same votes)
                va, vb = views_of(s1, rc_bytes(sb) if to_rc else sb, i0, j0, runs, to_rc, blen)
                self._memo[key] = tuple(np.array(tally(v), np.int64).reshape(-1, 2) for v in (va, vb))
            ta, tb = self._memo[key]
            self._apply(ia, ta)            # arrival order: view A, then view B
            self._apply(ib, tb)

    def call_read(self, r, min_cov=4):
        own_seq, v = self.reads[r], self.votes[r]
        L = len(own_seq)
        out = bytearray()
        n_sub = n_del = n_ins = n_low = 0
        for t in range(L):
            own = own_seq[t]
            base = [int(x) for x in v[t, 0:4]]
            dele, span = int(v[t, DEL]), int(v[t, SPAN])
            d = sum(base) + dele
            if d < min_cov:
                out.append(own)
                n_low += 1
            else:
                if own in ACGT:
                    base[ACGT.index(own)] += 1
                total = d + 1
                if 2 * dele > total:
                    n_del += 1
                else:
                    top = max(base)
                    if top == 0:
                        emit = own
                    elif own in ACGT and base[ACGT.index(own)] == top:
                        emit = own
                    else:
                        emit = ACGT[base.index(top)]
                    out.append(emit)
                    n_sub += emit != own
            if t < L - 1 and span >= min_cov:
                for k in range(KI):
                    ins = [int(x) for x in v[t, INS0 + 4 * k:INS0 + 4 * k + 4]]
                    m = max(ins)
                    if 2 * m > span + 1:
                        out.append(ACGT[ins.index(m)])
                        n_ins += 1
                    else:
                        break
        return bytes(out), (L, len(out), n_sub, n_del, n_ins, n_low)

    def call(self, min_cov=4):
        seqs, stats = [], np.zeros((len(self.reads), 6), np.int32)
        for r in range(len(self.reads)):
            s, st = self.call_read(r, min_cov)
            seqs.append(s)
            stats[r] = st
        return seqs, stats


RECORD_DTYPE = np.dtype([("from_id", "<i8"), ("to_id", "<i8"), ("score", "<f8"), ("raw", "<f8"), ("a1", "<i4"), ("a2", "<i4"),
                         ("alen", "<i4"), ("b1", "<i4"), ("b2", "<i4"), ("blen", "<i4"), ("to_rc", "<i4"), ("pad", "<i4")])


def records_from_results(from_ids, to_ids, alens, blens, to_rcs, results):
    """Realigned records from the aligner's seven fields per pair, as mhap_realign_records converts them: a1, a2 = read_begin, read_end;
    b1, b2 = ref_begin, ref_end, flipped back when to_rc; score = 1 - errors / columns; a pair without an alignment gives zeros."""
    out = np.zeros(len(results), RECORD_DTYPE)
    for q, a in enumerate(np.asarray(results).tolist()):
        rc, blen = int(to_rcs[q]) != 0, int(blens[q])
        out[q]["from_id"], out[q]["to_id"], out[q]["alen"], out[q]["blen"], out[q]["to_rc"] = from_ids[q], to_ids[q], alens[q], blen, int(rc)
        if a[0] > 0 and a[5] > 0:
            out[q]["a1"], out[q]["a2"] = a[1], a[2]
            out[q]["b1"] = blen - a[4] - 1 if rc else a[3]
            out[q]["b2"] = blen - a[3] - 1 if rc else a[4]
            out[q]["score"] = 1.0 - a[6] / a[5]
    return out


def levenshtein(a, b):
    """Edit distance of two byte strings (unit costs), one numpy step per row."""
    a, b = np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8)
    n = len(b)
    idx = np.arange(n + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        cur = np.empty(n + 1, np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i - 1]))
        prev = np.minimum.accumulate(cur - idx) + idx      # cur[j] = min over j' <= j of cur[j'] + (j - j')
    return int(prev[n])


# ---- the quality workload of the issue: a 2 500-base genome, 36 reads of 600 - 999 bases at 12 % error ------------------------------

def quality_workload(seed=7, genome_len=2500, n_reads=36, error=0.12, mix=(0.79, 0.12, 0.09), min_shared=200, band=150):
    """(reads, truths, bases, pairs7, meta): reads as stored (a read of strand 1 is the reverse complement of its genome segment),
    truths[r] = the bytes the stored read would be without errors, and one banded pair per two reads whose true placements share at
    least min_shared genome bases, around the diagonal the truth gives; meta[q] = (read A, read B, to_rc)."""
    rng = np.random.default_rng(seed)
    genome = bytes(rng.choice(list(ACGT), genome_len).tolist())
    p_ins, p_del, p_sub = (error * m for m in mix)
    reads, truths, place = [], [], []
    for _ in range(n_reads):
        want = int(rng.integers(600, 1000))
        start = int(rng.integers(0, genome_len - want))
        seg = genome[start:start + want]
        strand = int(rng.integers(0, 2))
        src = rc_bytes(seg) if strand else seg
        out = bytearray()
        for c in src:
            u = rng.random()
            while u < p_ins:                     # an inserted base, then the same source base again
                out.append(int(rng.choice(list(ACGT))))
                u = rng.random()
            if u < p_ins + p_del:
                continue
            if u < p_ins + p_del + p_sub:
                out.append(int(rng.choice([x for x in ACGT if x != c])))
            else:
                out.append(c)
        reads.append(bytes(out))
        truths.append(bytes(src))
        place.append((start, start + want, strand))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bases = np.frombuffer(b"".join(reads), np.uint8)
    pairs, meta = [], []
    for x in range(n_reads):
        for y in range(x + 1, n_reads):
            (sa, ea, ta), (sb, eb, tb) = place[x], place[y]
            lo, hi = max(sa, sb), min(ea, eb)
            if hi - lo < min_shared:
                continue
            g = (lo + hi) / 2.0                  # the middle of the shared stretch, in both reads' coordinates along A's strand
            la, lb = len(reads[x]), len(reads[y])
            i = ((ea - g) if ta else (g - sa)) * la / (ea - sa)
            j = ((eb - g) if ta else (g - sb)) * lb / (eb - sb)
            pairs.append((offsets[x], la, offsets[y], lb, int(ta != tb), int(round(j - i)), band))
            meta.append((x, y, int(ta != tb)))
    return reads, truths, bases, np.array(pairs, np.int64).reshape(-1, 7), meta


def quality_records(reads, meta, results):
    """The realigned records of quality_workload's pairs from the aligner's results; ids are 1-based positions."""
    return records_from_results([x + 1 for x, _, _ in meta], [y + 1 for _, y, _ in meta], [len(reads[x]) for x, _, _ in meta],
                                [len(reads[y]) for _, y, _ in meta], [rc for _, _, rc in meta], results)
