"""EstimateROC (J/main/EstimateROC.java; docs/source/utilities.rst "Validating overlaps"): sensitivity, specificity and PPV of a set
of overlaps against the reads' true positions, with the Smith-Waterman check of computeDP run on the GPU (mhap_amd.align_pairs).

    python -m mhap_amd.roc truth.m4 overlaps.txt reads.fasta [min_ovl [trials [dp [debug [min_identity [max_diff [load_all]]]]]]]

takes EstimateROC's positional arguments in its order (:173-201) and prints its three stdout lines; the phase lines with their times go
to stderr.  Restated literally, line numbers in the comments.  Deliberate deviations:
  - where Java would loop forever (estimateSensitivity without a truth read that has a match >= min_ovl, estimateSpecificity with a
    single truth read, estimatePPV without a record that passes its length test) RocError names the loop;
  - where Java throws or calls System.exit(1) RocError carries Java's message;
  - full mode (trials = 0) counts what fullEstimate's O(N^2) loop counts from the truth pairs and the records alone (full_counts);
  - every computeDP of a run is one batch for the aligner (PPV's draws never depend on an alignment, :848-879);
  - the debug argument is parsed and ignored (DEBUG's per-overlap diagnostics are not restated);
  - the aligner's path rules are this project's (include/mhap_hip.h, mhap_align_pairs): parity with SSW's cigar is not pinned.
"""
import math
import re
import sys
import time
from decimal import ROUND_HALF_EVEN, Context, Decimal, localcontext

import numpy as np

MIN_REF_OVERLAP_DIFFERENCE = 0.8     # :66
REF_IDENTITY_ADJUSTMENT = 0.1        # :68
DEFAULT_NUM_TRIALS = 10000           # :72
DEFAULT_MIN_OVL = 2000               # :73


class RocError(RuntimeError):
    """What EstimateROC would have thrown, exited with, or looped forever on."""


# ---- java.util.Random ------------------------------------------------------------------------------------------------------
class JavaRandom:
    """java.util.Random: the 48-bit LCG, next(bits), nextDouble(), nextInt() and nextInt(bound) with its power-of-two and rejection branches."""
    MULT, ADD, MASK = 0x5DEECE66D, 0xB, (1 << 48) - 1

    def __init__(self, seed=0):
        self.seed = (seed ^ self.MULT) & self.MASK

    def next(self, bits):
        self.seed = (self.seed * self.MULT + self.ADD) & self.MASK
        r = self.seed >> (48 - bits)
        return r - (1 << 32) if r >= 1 << 31 else r     # (int) of the top `bits` bits

    def next_double(self):
        return ((self.next(26) << 27) + self.next(27)) * 2.0 ** -53

    def next_int(self, bound=None):
        if bound is None:
            return self.next(32)
        if bound <= 0:
            raise RocError("bound must be positive")
        r = self.next(31)
        m = bound - 1
        if (bound & m) == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if _i32(u - r + m) >= 0:
                return r
            u = self.next(31)


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


# ---- Utils.DECIMAL_FORMAT = new DecimalFormat("############.########") (J/utils/Utils.java:120) ----------------------------------
def decimal_format(x):
    """HALF_EVEN on the double's exact binary value, at most 8 fraction digits, no trailing zeros, no integer digit below 1."""
    x = float(x)
    if x != x:
        return "�"
    sign = "-" if math.copysign(1.0, x) < 0 else ""
    if math.isinf(x):
        return sign + "∞"
    with localcontext(Context(prec=1000)):
        d = Decimal(abs(x)).quantize(Decimal("1e-8"), rounding=ROUND_HALF_EVEN)
    s = format(d, "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    if s.startswith("0."):
        s = s[1:]
    return sign + (s if s else "0")


# ---- Java parsing ----------------------------------------------------------------------------------------------------------
_WS = re.compile(r"[ \t\n\x0b\f\r]+")
_INT = re.compile(r"[+-]?[0-9]+\Z")
_DBL = re.compile(r"[+-]?(NaN|Infinity|([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?[fFdD]?)\Z")


def java_split(line):
    """line.trim().split("\\\\s+")."""
    t = line.strip("".join(chr(c) for c in range(33)))
    return _WS.split(t) if t else [""]


def parse_int(s):
    """Integer.parseInt: NumberFormatException -> ValueError."""
    if not _INT.match(s) or not -(1 << 31) <= int(s) < (1 << 31):
        raise ValueError(f'For input string: "{s}"')
    return int(s)


def parse_double(s):
    t = s.strip("".join(chr(c) for c in range(33)))
    if not _DBL.match(t):
        raise ValueError(f'For input string: "{s}"')
    return float(t.rstrip("fFdD").replace("Infinity", "inf"))


def java_round(x):
    """Math.round(double): floor(x + 0.5)."""
    return math.floor(x + 0.5)


def get_range_overlap(startA, endA, startB, endB):
    """Utils.getRangeOverlap (J/utils/Utils.java:307-318): inclusive, may be <= 0."""
    return min(max(startA, endA), max(startB, endB)) - max(min(startA, endA), min(startB, endB)) + 1


def ovl_name(a, b):
    """getOvlName (:320-323): String.compareTo order."""
    return a + "_" + b if a <= b else b + "_" + a


def _eq_ignore_case(a, b):
    return len(a) == len(b) and all(x == y or x.upper() == y.upper() or x.lower() == y.lower() for x, y in zip(a, b))


class Overlap:
    """EstimateROC.Overlap (:94-132)."""
    __slots__ = ("afirst", "bfirst", "asecond", "bsecond", "isFwd", "id1", "id2")

    def __init__(self):
        self.afirst = self.bfirst = self.asecond = self.bsecond = 0
        self.isFwd = False
        self.id1 = self.id2 = None

    def get_size(self):   # :107-111
        first = float(max(self.asecond, self.afirst)) - float(min(self.asecond, self.afirst))
        first += float(max(self.bsecond, self.bfirst)) - float(min(self.bsecond, self.bfirst))
        return java_round(first / 2)


def get_sequence_id(id_):
    """getSequenceId (:316-318)."""
    try:
        return parse_int(id_) - 1
    except ValueError as e:
        raise RocError(str(e)) from None


def get_overlap_info(line, seq_len):
    """getOverlapInfo (:375-476); seq_len(index) = this.dataSeq[index].length().  A NumberFormatException warns and returns the fields
    parsed so far, as Java does."""
    o = Overlap()
    sp = java_split(line)
    try:
        if len(sp) in (6, 7):                                            # CA format :381-396
            o.id1, o.id2 = sp[0], sp[1]
            parse_double(sp[5])
            aoffset, boffset = parse_int(sp[3]), parse_int(sp[4])
            o.isFwd = sp[2].upper() == "N"
            alen, blen = seq_len(parse_int(o.id1) - 1), seq_len(parse_int(o.id2) - 1)
            o.afirst = max(0, aoffset)
            o.asecond = min(alen, alen + boffset)
            o.bfirst = -1 * min(0, aoffset)
            o.bsecond = min(blen, blen - boffset)
        elif len(sp) == 12:                                              # mhap format :398-417
            o.id1, o.id2 = sp[0], sp[1]
            parse_double(sp[2])
            o.isFwd = parse_int(sp[8]) == 0
            alen, blen = seq_len(parse_int(o.id1) - 1), seq_len(parse_int(o.id2) - 1)
            o.afirst, o.asecond = parse_int(sp[5]), parse_int(sp[6])
            o.bfirst, o.bsecond = parse_int(sp[9]), parse_int(sp[10])
            o.asecond = min(o.asecond, alen)
            o.bsecond = min(o.bsecond, blen)
        elif len(sp) == 13 and "[" not in line:                          # blasr format :419-450
            o.afirst, o.asecond = parse_int(sp[5]), parse_int(sp[6])
            o.bfirst, o.bsecond = parse_int(sp[9]), parse_int(sp[10])
            o.isFwd = parse_int(sp[8]) == 0
            if not o.isFwd:
                o.bsecond = parse_int(sp[11]) - parse_int(sp[9])
                o.bfirst = parse_int(sp[11]) - parse_int(sp[10])
            o.id1 = sp[0]
            if "/" in o.id1:
                o.id1 = o.id1[:sp[0].index("/")]
            if "," in o.id1:
                o.id1 = _java_split_literal(o.id1, ",")[1]
            o.id2 = sp[1]
            if "," in o.id2:
                o.id2 = _java_split_literal(o.id2, ",")[1]
            alen, blen = seq_len(parse_int(o.id1) - 1), seq_len(parse_int(o.id2) - 1)
            o.asecond = min(o.asecond, alen)
            o.bsecond = min(o.bsecond, blen)
        elif 13 <= len(sp) <= 18:                                        # daligner LAshow :451-468
            o.id1, o.id2 = sp[0].replace(",", ""), sp[1].replace(",", "")
            o.isFwd = sp[2].upper() == "N"
            two = line.split("[")
            a_info, b_info = two[1][:_index(two[1], "]")], two[2][:_index(two[2], "]")]
            a_sp, b_sp = a_info.replace(",", "").split(".."), b_info.replace(",", "").split("..")
            o.afirst, o.asecond = parse_int(a_sp[0].strip()), parse_int(a_sp[1].strip())
            o.bfirst, o.bsecond = parse_int(b_sp[0].strip()), parse_int(b_sp[1].strip())
            if not o.isFwd:
                blen = seq_len(parse_int(o.id2) - 1)
                o.bsecond = blen - parse_int(b_sp[0].strip())
                o.bfirst = blen - parse_int(b_sp[1].strip())
    except ValueError as e:
        print(f"Warning: could not parse input line: {line} {e}", file=sys.stderr)
    return o


def _index(s, sub):
    i = s.find(sub)
    if i < 0:
        raise RocError(f"begin 0, end -1, length {len(s)}")   # substring(0, -1)
    return i


def _java_split_literal(s, sep):
    parts = s.split(sep)
    while parts and parts[-1] == "":
        parts.pop()
    if len(parts) < 2:
        raise RocError(f"Index 1 out of bounds for length {len(parts)}")
    return parts


# ---- IntervalTree / IntervalNode (J/utils/IntervalTree.java, IntervalNode.java, Interval.java) ----------------------------------
class IntervalNode:
    """Median of the distinct endpoints as centre; intervals ending before it go left, starting after it go right, the rest stay here
    in (start, end) order; query: strict Interval.intersects, descending left when target.start < centre, right when target.end > centre."""

    def __init__(self, intervals):
        pts = sorted({p for s, e, _ in intervals for p in (s, e)})
        self.center = pts[len(pts) // 2]
        left, right, here = [], [], {}
        for iv in intervals:
            if iv[1] < self.center:
                left.append(iv)
            elif iv[0] > self.center:
                right.append(iv)
            else:
                here.setdefault((iv[0], iv[1]), []).append(iv)
        self.entries = sorted(here.items())
        self.left = IntervalNode(left) if left else None
        self.right = IntervalNode(right) if right else None

    def query(self, ts, te):
        out = []
        for (s, e), posting in self.entries:
            if te > s and ts < e:
                out.extend(d for _, _, d in posting)
            elif s > te:
                break
        if ts < self.center and self.left is not None:
            out.extend(self.left.query(ts, te))
        if te > self.center and self.right is not None:
            out.extend(self.right.query(ts, te))
        return out


class IntervalTree:
    def __init__(self):
        self.intervals, self.head = [], None

    def add_interval(self, start, end, data):
        self.intervals.append((start, end, data))
        self.head = None

    def get(self, start, end):
        if self.head is None:
            self.head = IntervalNode(self.intervals)
        return self.head.query(start, end)


def intersecting_pairs(starts, ends):
    """Every unordered pair (u, v), u < v, whose intervals intersect as Interval.intersects says (e_v > s_u and s_v < e_u): the pairs
    IntervalTree.get returns, found with one sort (tests/test_roc_cpu.py checks the membership against the literal tree)."""
    s = np.asarray(starts, np.int64)
    e = np.asarray(ends, np.int64)
    o = np.argsort(s, kind="stable")
    ss, es = s[o], e[o]
    hi = np.searchsorted(ss, es, side="left")                 # later entries with s_v < e_u
    cnt = np.maximum(hi - np.arange(len(ss)) - 1, 0)
    u = np.repeat(np.arange(len(ss)), cnt)
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    v = u + 1 + (np.arange(len(u)) - first)
    keep = (es[v] > ss[u]) & (ss[v] < es[u])
    a, b = o[u[keep]], o[v[keep]]
    return np.minimum(a, b), np.maximum(a, b)


# ---- EstimateROC ------------------------------------------------------------------------------------------------------------
class EstimateROC:
    def __init__(self, min_ovl=DEFAULT_MIN_OVL, trials=DEFAULT_NUM_TRIALS, dp=False, min_identity=None, max_diff=None, load_all=False,
                 aligner=None, device=0, log=None):
        self.min_ovl, self.trials, self.dp, self.load_all = int(min_ovl), int(trials), bool(dp), bool(load_all)
        mi = 0.70 if min_identity is None else float(min_identity)                        # MIN_IDENTITY :67, :192
        self.min_ref_identity = mi + REF_IDENTITY_ADJUSTMENT                               # :69, :193
        self.min_alignment_identity = mi - (REF_IDENTITY_ADJUSTMENT if min_identity is None else REF_IDENTITY_ADJUSTMENT / 2)   # :70, :194
        self.max_diff = 0.30 if max_diff is None else float(max_diff)                      # MIN_OVERLAP_DIFFERENCE :71, :197
        self.aligner, self.device, self.log = aligner, device, log
        self.generator = JavaRandom(0)                                                     # :292
        self.tp = self.fn = self.tn = self.fp = 0
        self.ppv = 0.0
        self.dp_pairs = self.dp_cells = 0
        self.dp_seconds = 0.0

    # processReference (:548-627)
    def process_reference(self, path):
        pos, chr_, score, names = {}, {}, {}, []
        with open(path) as fh:
            for line in fh:
                sp = java_split(line.rstrip("\r\n"))
                id_ = sp[0]
                if "/" in id_:
                    id_ = id_[:sp[0].index("/")]
                if "," in id_:
                    id_ = _java_split_literal(id_, ",")[1]
                try:
                    idy = parse_double(sp[3])
                    start, end, _length, seq_is_fwd = parse_int(sp[5]), parse_int(sp[6]), parse_int(sp[7]), parse_int(sp[4])
                    if seq_is_fwd != 0:
                        raise RocError("Error: malformed line, first sequences should always be in fwd orientation")
                    s_ref, e_ref, ref_len, is_rev, sc = parse_int(sp[9]), parse_int(sp[10]), parse_int(sp[11]), parse_int(sp[8]), parse_int(sp[2])
                except ValueError as e:
                    raise RocError(str(e)) from None
                if is_rev == 1:
                    s_ref, e_ref = ref_len - e_ref, ref_len - s_ref
                if idy < self.min_ref_identity * 100:
                    continue
                den = float(e_ref - s_ref)
                num = float(end - start)
                diff = num / den if den != 0 else (math.nan if num == 0 else math.copysign(math.inf, num) * math.copysign(1.0, den))
                if diff < MIN_REF_OVERLAP_DIFFERENCE:
                    continue
                c = sp[1]
                if id_ in pos:
                    if sc < score[id_]:
                        pos[id_], chr_[id_], score[id_] = (s_ref, e_ref), c, sc
                else:
                    pos[id_], chr_[id_], score[id_] = (s_ref, e_ref), c, sc
                    names.append(id_)
        if not pos:
            raise RocError("Error: No sequence matches to reference loaded!")
        self.seq_to_name = names
        self.index = {n: i for i, n in enumerate(names)}
        self.pos = np.array([pos[n] for n in names], np.int64).reshape(-1, 2)
        self.chr = [chr_[n] for n in names]
        self._build_matches()

    def _build_matches(self):
        """getSequenceMatches(id, 0) of every truth read (:347-373) as one pair list: same chromosome, the tree's strict intersection,
        getRangeOverlap >= 0, and not the same id ignoring case."""
        us, vs = [], []
        by_chr = {}
        for i, c in enumerate(self.chr):
            by_chr.setdefault(c, []).append(i)
        for members in by_chr.values():
            mem = np.asarray(members, np.int64)
            a, b = intersecting_pairs(self.pos[mem, 0], self.pos[mem, 1])
            us.append(mem[a])
            vs.append(mem[b])
        u = np.concatenate(us) if us else np.zeros(0, np.int64)
        v = np.concatenate(vs) if vs else np.zeros(0, np.int64)
        p, q = self.pos[u], self.pos[v]
        ov = np.minimum(p.max(1), q.max(1)) - np.maximum(p.min(1), q.min(1)) + 1
        lower = np.unique([n.lower() for n in self.seq_to_name], return_inverse=True)[1] if len(u) else np.zeros(0, np.int64)
        keep = ov >= 0
        if len(u):
            keep &= lower[u] != lower[v]
        self.mu, self.mv, self.mov = u[keep], v[keep], ov[keep]

    def load_fasta(self, fasta):   # loadFasta (:478-486)
        from .api import FastaData
        self.fasta = fasta if isinstance(fasta, FastaData) else FastaData.from_file(str(fasta))

    def _seq_len(self, k):
        if k < 0 or k >= len(self.fasta):
            raise RocError(f"Index {k} out of bounds for length {len(self.fasta)}")
        return int(self.fasta.lengths[k])

    # processOverlaps (:488-538)
    def process_overlaps(self, path):
        names, info, order = {}, {}, []
        in_truth = self.index
        with open(path) as fh:
            for line in fh:
                o = get_overlap_info(line.rstrip("\r\n"), self._seq_len)
                ovl_len = o.get_size()
                a, b = o.id1, o.id2
                if a is None or b is None or _eq_ignore_case(a, b):
                    continue
                if not self.load_all and (a not in in_truth or b not in in_truth):
                    continue
                name = ovl_name(a, b)
                old = names.get(name)
                if old is not None and ovl_len < old:
                    continue
                if old is None:
                    order.append(name)
                names[name] = ovl_len
                info[name] = o
        if not names:
            raise RocError("Error: No sequence matches to reference loaded!")
        self.ovl_names, self.ovl_info, self.ovl_to_name = names, info, order

    # overlapMatches (:633-646) for the truth-read pairs (u, v) with records
    def _overlap_matches(self, ref_overlap, size):
        diff = abs(size - ref_overlap)
        if ref_overlap == 0:
            pct = math.nan if diff == 0 else math.inf
        else:
            pct = diff / ref_overlap
        return not (pct > self.max_diff)

    def _record_pairs(self):
        """The records between two truth reads: (u, v, name) with u < v (seqToName order)."""
        out = []
        for name, o in self.ovl_info.items():
            u, v = self.index.get(o.id1), self.index.get(o.id2)
            if u is None or v is None:
                continue
            out.append((min(u, v), max(u, v), name))
        return out

    def _ref_overlap(self, u, v):
        p, q = self.pos[u], self.pos[v]
        return get_range_overlap(int(p[0]), int(p[1]), int(q[0]), int(q[1]))

    # computeDP (:746-800), every call of a run in one batch
    def _compute_dp(self, names):
        if not self.dp or not names:
            return {n: False for n in names}
        f = self.fasta
        pairs, lens = [], []
        for name in names:
            o = self.ovl_info[name]
            k1, k2 = get_sequence_id(o.id1), get_sequence_id(o.id2)
            l1, l2 = self._seq_len(k1), self._seq_len(k2)
            for a, b, ln in ((o.afirst, o.asecond, l1), (o.bfirst, o.bsecond, l2)):
                if a < 0 or b > ln or a > b:
                    raise RocError(f"begin {a}, end {b}, length {ln}")   # String.substring
            pairs.append((int(f.offsets[k1]) + o.afirst, o.asecond - o.afirst, int(f.offsets[k2]) + o.bfirst, o.bsecond - o.bfirst,
                          0 if o.isFwd else 1))
            lens.append(min(o.asecond - o.afirst, o.bsecond - o.bfirst))
        pairs = np.asarray(pairs, np.int64).reshape(-1, 5)
        self.dp_pairs += len(pairs)
        self.dp_cells += int((pairs[:, 1].astype(np.float64) * pairs[:, 3]).sum())
        t0 = time.time()
        if self.aligner is not None:
            res = np.asarray(self.aligner(f.bases, pairs))
        else:
            from .api import align_pairs
            res = align_pairs(f.bases, pairs, device=self.device)
        self.dp_seconds += time.time() - t0
        out = {}
        with np.errstate(divide="ignore", invalid="ignore"):
            for name, r, ovl_len in zip(names, res.tolist(), lens):
                _, rb, re_, fb, fe, cols, errs = r
                length = max(re_ - rb, fe - fb)                                        # :790
                score = 1 - (errs / cols) if cols else math.nan                       # getScore :693-744
                frac = np.float32(1) - np.float32(length) / np.float32(ovl_len)       # 1-((float)length/ovlLen)
                out[name] = bool(score > self.min_alignment_identity and length > self.min_ovl and float(frac) < self.max_diff)   # :799
        return out

    # estimateSensitivity (:802-817)
    def estimate_sensitivity(self):
        N = len(self.seq_to_name)
        big = self.mov >= self.min_ovl
        u, v, ov = self.mu[big], self.mv[big], self.mov[big]
        recs = {}
        for a, b, name in self._record_pairs():
            recs[(a, b)] = self.ovl_info[name].get_size()
        ok = np.array([(int(a), int(b)) in recs and self._overlap_matches(int(o), recs[(int(a), int(b))])
                       for a, b, o in zip(u, v, ov)], dtype=bool)
        n_match = np.bincount(u, minlength=N) + np.bincount(v, minlength=N)
        n_ok = np.bincount(u[ok], minlength=N) + np.bincount(v[ok], minlength=N)
        if self.trials > 0 and not n_match.any():
            raise RocError(f"estimateSensitivity would loop forever: no truth read has a match of at least {self.min_ovl} bases")
        for _ in range(self.trials):
            while True:
                k = self.generator.next_int(N)
                if n_match[k]:
                    break
            self.tp += int(n_ok[k])
            self.fn += int(n_match[k] - n_ok[k])

    def _neighbours(self):
        if not hasattr(self, "_nb"):
            nb = [set() for _ in self.seq_to_name]
            for a, b in zip(self.mu.tolist(), self.mv.tolist()):
                nb[a].add(b)
                nb[b].add(a)
            self._nb = nb
        return self._nb

    # estimateSpecificity (:819-840)
    def estimate_specificity(self):
        N = len(self.seq_to_name)
        nb = self._neighbours()
        names = self.seq_to_name
        if self.trials > 0 and N < 2:
            raise RocError("estimateSpecificity would loop forever: fewer than two truth reads")
        for _ in range(self.trials):
            k = self.generator.next_int(N)
            o = self.generator.next_int(N)
            while _eq_ignore_case(names[k], names[o]):
                o = self.generator.next_int(N)
            if o not in nb[k]:
                if ovl_name(names[k], names[o]) in self.ovl_names:
                    self.fp += 1
                else:
                    self.tn += 1

    # estimatePPV (:842-883): the accepted draws are the first `trials` draws that pass the length test, whatever the thread order
    def estimate_ppv(self):
        if self.trials <= 0:
            return
        if self.min_ovl <= 0:
            raise RocError(f"Could not find any computed overlaps > {self.min_ovl}")
        names = self.ovl_to_name
        lens = []
        for n in names:
            o = self.ovl_info[n]
            lens.append(get_range_overlap(o.afirst, o.asecond, o.bfirst, o.bsecond))
        if not any(x >= self.min_ovl for x in lens):
            raise RocError(f"estimatePPV would loop forever: no record has an overlap of at least {self.min_ovl} bases")
        nb = self._neighbours()
        tp, need = 0, []
        for _ in range(self.trials):
            while True:
                k = self.generator.next_int(len(names))
                if lens[k] >= self.min_ovl:
                    break
            parts = [p for p in names[k].split("_")]
            a, b = parts[0], parts[1]
            ia, ib = self.index.get(a), self.index.get(b)
            if ia is not None and ib is not None and ib in nb[ia]:
                tp += 1
            else:
                need.append(names[k])
        dp = self._compute_dp(sorted(set(need)))
        tp += sum(1 for n in need if dp[n])
        self.ppv = tp / float(self.trials)

    # fullEstimate (:886-914) without the O(N^2) loop
    def full_estimate(self):
        N = len(self.seq_to_name)
        if N >= 2:
            c0 = self.chr[0]
            for j in range(1, N):
                if not _eq_ignore_case(c0, self.chr[j]):
                    raise RocError(f"Error: comparing wrong chromosomes betweeen sequences {self.seq_to_name[0]} and sequence {self.seq_to_name[j]}")
        matched = {(int(a), int(b)): int(o) for a, b, o in zip(self.mu, self.mv, self.mov)}
        om = set()
        for a, b, name in self._record_pairs():
            if self._overlap_matches(self._ref_overlap(a, b), self.ovl_info[name].get_size()):
                om.add((a, b, name))
        om_keys = {(a, b) for a, b, _ in om}
        for key, ov in matched.items():
            if key not in om_keys and ov > self.min_ovl:
                self.fn += 1
        need = []
        for a, b, name in om:
            if (a, b) in matched:
                self.tp += 1
            else:
                need.append(name)
        dp = self._compute_dp(sorted(need))
        for n in need:
            if dp[n]:
                self.tp += 1
            else:
                self.fp += 1
        self.tn = N * (N - 1) // 2 - len(set(matched) | om_keys)
        self.ppv = self.tp / (float(self.tp) + float(self.fp)) if self.tp + self.fp else math.nan

    def lines(self):   # :256-261
        def div(a, b):
            return a / b if b else (math.nan if a == 0 else math.inf)
        return ["Estimated sensitivity:\t" + decimal_format(div(float(self.tp), float(self.tp + self.fn))),
                "Estimated specificity:\t" + decimal_format(div(float(self.tn), float(self.fp + self.tn))),
                "Estimated PPV:\t " + decimal_format(self.ppv)]


class RocResult:
    __slots__ = ("tp", "fn", "tn", "fp", "ppv", "sensitivity", "specificity", "lines", "dp_pairs", "dp_cells", "dp_seconds", "phases")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def as_dict(self):
        return {k: getattr(self, k) for k in self.__slots__}


def estimate_roc(truth_m4, overlaps, fasta, min_ovl=DEFAULT_MIN_OVL, trials=DEFAULT_NUM_TRIALS, dp=False, verbose=False, min_identity=None,
                 max_diff=None, load_all=False, device=0, aligner=None):
    """EstimateROC.main (:173-262) on files (fasta may also be a FastaData): tp, fn, tn, fp, ppv, sensitivity, specificity and the three
    stdout lines.  aligner: a callable with mhap_amd.align_pairs' (bases, pairs) signature (default: the GPU aligner on `device`).
    verbose: the phase lines with their times on stderr."""
    g = EstimateROC(min_ovl, trials, dp, min_identity, max_diff, load_all, aligner, device)
    phases = {}

    def phase(label, key, fn):
        if verbose:
            print(label, end="", file=sys.stderr, flush=True)
        t0 = time.time()
        fn()
        phases[key] = time.time() - t0
        if verbose:
            print(f"done {phases[key]}s.", file=sys.stderr)

    t_all = time.time()
    phase("Loading reference...", "reference", lambda: g.process_reference(str(truth_m4)))
    phase("Loading fasta...", "fasta", lambda: g.load_fasta(fasta))
    phase("Loading matches...", "matches", lambda: g.process_overlaps(str(overlaps)))
    if g.trials == 0:
        phase(f"Computing full statistics O({len(g.seq_to_name)}^2) operations!...", "full", g.full_estimate)
    else:
        phase("Computing sensitivity...", "sensitivity", g.estimate_sensitivity)
        phase("Computing specificity...", "specificity", g.estimate_specificity)
        phase("Computing PPV...", "ppv", g.estimate_ppv)
    phases["total"] = time.time() - t_all
    if verbose:
        print(f"Total time: {phases['total']}s.", file=sys.stderr)
    lines = g.lines()
    sens = g.tp / (g.tp + g.fn) if g.tp + g.fn else math.nan
    spec = g.tn / (g.fp + g.tn) if g.fp + g.tn else math.nan
    return RocResult(tp=g.tp, fn=g.fn, tn=g.tn, fp=g.fp, ppv=g.ppv, sensitivity=sens, specificity=spec, lines=lines, dp_pairs=g.dp_pairs,
                     dp_cells=g.dp_cells, dp_seconds=g.dp_seconds, phases=phases)


def _parse_bool(s):   # Boolean.parseBoolean
    return s.lower() == "true"


def main(argv=None):
    args = sys.argv[1:] if argv is None else list(argv)
    if len(args) < 3:   # printUsage (:157-171)
        print("This program uses random sampling to estimate PPV/Sensitivity/Specificity\n"
              "The sequences in the fasta file used to generate the truth must be sequentially numbered from 1 to N!\n"
              "\t1. A blasr M4 file mapping sequences to a reference (or reference subset)\n"
              "\t2. All-vs-all mappings of same sequences in CA ovl format\n"
              "\t3. Fasta sequences sequentially numbered from 1 to N.\n"
              f"\t4. Minimum overlap length (default: {DEFAULT_MIN_OVL}\n"
              f"\t5. Number of random trials, 0 means full compute (default : {DEFAULT_NUM_TRIALS}\n"
              "\t6. Compute DP during PPV true/false\n"
              "\t7. Debug output true/false", file=sys.stderr)
        return 1
    try:
        min_ovl = parse_int(args[3]) if len(args) > 3 else DEFAULT_MIN_OVL
        trials = parse_int(args[4]) if len(args) > 4 else DEFAULT_NUM_TRIALS
        dp = _parse_bool(args[5]) if len(args) > 5 else False
        min_identity = parse_double(args[7]) if len(args) > 7 else None
        max_diff = parse_double(args[8]) if len(args) > 8 else None
    except ValueError as e:
        print(f"Error: {e}", file=sys.stderr)
        return 1
    load_all = _parse_bool(args[9]) if len(args) > 9 else False
    print(f"Running, reference: {args[0]} matches: {args[1]}", file=sys.stderr)
    print(f"Number trials:  {'all' if trials == 0 else trials}", file=sys.stderr)
    print(f"Minimum ovl:  {min_ovl}", file=sys.stderr)
    try:
        r = estimate_roc(args[0], args[1], args[2], min_ovl, trials, dp, True, min_identity, max_diff, load_all)
    except RocError as e:
        print(str(e), file=sys.stderr)
        return 1
    for line in r.lines:
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
