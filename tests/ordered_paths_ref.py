"""The path rule of ordered_kernel (mhap_amd/csrc/sketch_kernels.hip) restated on the CPU, from the rule the kernel documents — not a port of
its code.  Given a strand's 32-bit k2-mer hashes, S and the longest read of the launch, `classify` returns the code that the `ordpaths` build
(-DMH_ORD_PATHS) records for the strand, and whether that code is the same for every cut within +-CUT_MARGIN of the computed one.

The rule.  n = the strand's k2-mers, K = min(S, n), cap = the next power of two >= S.  Keys are (hash ^ 0x80000000) << 32 | pos (unsigned order
= signed hash, then position).
  n <= cap               every key goes through the bitonic network ("all").
  one-pass attempt       only if n > cap and t = min(K + 7 sqrt K, cap - 5 sqrt cap) >= K + 3 sqrt K.  The keys whose (hash ^ 0x80000000)
                         is below cut = floor(t / n * 2^32) are staged, m of them.  m < K: rejected short.  m > cap: rejected over.  A
                         first-level bin (top 11 bits, 2 048 bins) with more than ORD_BUCKET_MAX = 32 staged keys: rejected crowded.
                         Otherwise accepted: the staged keys are bucket-ranked into the row.
  exact selection        not attempted or rejected: radix select on the key, 11/11/10 bits of hash then 11/11/10 bits of position.  At each
                         level the bin holding rank K - 1 among the keys that match the prefix is found; the selection ends at the first
                         level where (keys below the bin) + (keys in the bin) <= cap, with bound = prefix | (all lower bits set).  Ending
                         at level 0 with no bin up to the chosen one above 32 keys: bucket-ranked; otherwise the network sorts every key
                         <= bound.

The code: bits 0-3 the one-pass attempt (ATT_*), bits 4-7 how the row was made (HOW_*; HOW_NET0 + L = network after ending at level L),
bit 8 the launch stages 32-bit positions (its longest read has more than 65 535 k2-mers), bit 9 the strand's hashes are read from memory
(MHAP_RD_MAT).  0 = the strand was skipped or has no k2-mer.  The witness line of the ordpaths build:
  [ordered paths] first F count C cap CAP S S codes: xxx xxx ...       (C three-digit hex codes, strands F .. F + C - 1)
"""
import math
import re
from collections import namedtuple

import numpy as np

ORD_BINS = 2048
ORD_BUCKET_MAX = 32
CUT_MARGIN = 4096
WIDE_KMERS = 65535            # more k2-mers than this in the launch's longest read: 32-bit staged positions
CODES_MAX_KMERS = 24 * 1024   # k = 16 / k2 = 12 ACGT reads with at most this many 16-mers are hashed from their 2-bit codes

ATT_NONE, ATT_ACCEPTED, ATT_SHORT, ATT_OVER, ATT_CROWDED = 0, 1, 2, 3, 4
HOW_SKIPPED, HOW_ALL, HOW_ONEPASS, HOW_BUCKETS0, HOW_NET0 = 0, 1, 2, 3, 4
ATT_NAMES = {ATT_NONE: "not-attempted", ATT_ACCEPTED: "accepted", ATT_SHORT: "rejected-short", ATT_OVER: "rejected-over",
             ATT_CROWDED: "rejected-crowded"}
BIT_WIDE, BIT_MAT = 1 << 8, 1 << 9
SHIFTS = (53, 42, 32, 21, 10, 0)
WIDTHS = (11, 11, 10, 11, 11, 10)
WITNESS_RE = re.compile(r"^\[ordered paths\] first (\d+) count (\d+) cap (\d+) S (\d+) codes:((?: [0-9a-f]{3})*)$")

Path = namedtuple("Path", "code stable selected level")   # selected: positions of the keys the kernel keeps for sorting (a superset of the row)


def cap_of(S):
    cap = 1
    while cap < S:
        cap <<= 1
    return cap


def make_code(att, how, wide, mat):
    return att | (how << 4) | (BIT_WIDE if wide else 0) | (BIT_MAT if mat else 0)


def describe(code):
    if code == 0:
        return "skipped"
    how = (code >> 4) & 15
    name = {HOW_ALL: "all-keys network", HOW_ONEPASS: "one-pass buckets", HOW_BUCKETS0: "level-0 buckets"}.get(how) or f"network level {how - HOW_NET0}"
    return f"{ATT_NAMES[code & 15]} -> {name}, {'32' if code & BIT_WIDE else '16'}-bit stage, {'stored' if code & BIT_MAT else 'recomputed'} hashes"


def path_class(code):
    """(attempt, how) without the launch's and the hash source's bits: what the table of classes is about."""
    return code & 15, (code >> 4) & 15


def one_pass_cut(n, S):
    """The cut on (hash ^ 0x80000000) of the one-pass attempt, or None where it is not attempted."""
    cap, K = cap_of(S), min(S, n)
    if n <= cap:
        return None
    ksig, csig = math.sqrt(float(K)), math.sqrt(float(cap))
    target = min(K + 7.0 * ksig, cap - 5.0 * csig)
    if not target >= K + 3.0 * ksig:
        return None
    quant = target / float(n)
    return 0xFFFFFFFF if quant >= 1.0 else int(quant * 4294967296.0)


def _attempt(u, cut, K, cap):
    below = u[u < np.uint32(cut)] if cut < (1 << 32) else u
    m = int(below.size)
    if m < K:
        return ATT_SHORT
    if m > cap:
        return ATT_OVER
    if int(np.bincount(below >> np.uint32(21), minlength=ORD_BINS).max()) > ORD_BUCKET_MAX:
        return ATT_CROWDED
    return ATT_ACCEPTED


def _exact(u, K, cap):
    """(how, level, positions of the keys <= bound) of the multi-level selection."""
    n = u.size
    keys = (u.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    live = keys           # the keys that match the prefix fixed so far
    below = 0
    prefix = 0
    for lv in range(6):
        sh, nb = SHIFTS[lv], 1 << WIDTHS[lv]
        digit = ((live >> np.uint64(sh)) & np.uint64(nb - 1)).astype(np.int64)
        hist = np.bincount(digit, minlength=nb)
        incl = np.cumsum(hist)
        target = K - 1 - below
        b = int(np.searchsorted(incl, target, side="right"))
        binbelow, bincnt = int(incl[b] - hist[b]), int(hist[b])
        below += binbelow
        prefix |= b << sh
        bound = prefix | ((1 << sh) - 1)
        if below + bincnt <= cap:
            sel = np.nonzero(keys <= np.uint64(bound))[0]
            assert sel.size == below + bincnt
            if lv == 0 and int(hist[:b + 1].max()) <= ORD_BUCKET_MAX:
                return HOW_BUCKETS0, 0, sel
            return HOW_NET0 + lv, lv, sel
        live = live[digit == b]
    raise AssertionError("the last level's bins hold one key each: the selection ends there at the latest")


def classify(h32, S, launch_max_kmers, mat):
    """h32: the strand's k2-mer hashes in position order (int32 or uint32); launch_max_kmers: the k2-mers of the launch's longest read."""
    u = np.ascontiguousarray(h32).view(np.uint32) ^ np.uint32(0x80000000)
    n = int(u.size)
    if n < 1:
        return Path(0, True, np.zeros(0, np.int64), None)
    cap, K = cap_of(S), min(S, n)
    wide = launch_max_kmers > WIDE_KMERS
    if n <= cap:
        return Path(make_code(ATT_NONE, HOW_ALL, wide, mat), True, np.arange(n), None)
    cut = one_pass_cut(n, S)
    att, stable = ATT_NONE, True
    if cut is not None:
        att = _attempt(u, cut, K, cap)
        for c in (max(0, cut - CUT_MARGIN), min(0xFFFFFFFF, cut + CUT_MARGIN)):   # (the staged set and its largest bin only grow with the cut)
            stable = stable and _attempt(u, c, K, cap) == att
        if att == ATT_ACCEPTED:
            return Path(make_code(att, HOW_ONEPASS, wide, mat), stable, np.nonzero(u < np.uint32(cut))[0], None)
    how, lv, sel = _exact(u, K, cap)
    return Path(make_code(att, how, wide, mat), stable, sel, lv)


def parse_witness(stderr_text):
    """The [ordered paths] lines of a run: dicts first / count / cap / S / codes (list of ints)."""
    out = []
    for ln in stderr_text.splitlines():
        m = WITNESS_RE.match(ln)
        if m:
            codes = [int(x, 16) for x in m[5].split()]
            assert len(codes) == int(m[2]), ln
            out.append(dict(first=int(m[1]), count=int(m[2]), cap=int(m[3]), S=int(m[4]), codes=codes))
    return out


def strand_is_mat(seq, k, k2, fused_env=True):
    """Whether the library stores the strand's hashes in memory (MHAP_RD_MAT): raw-byte reads (a character outside ACGT, either case),
    k != 16 / k2 != 12, MHAP_FUSED_HASH=0, or more 16-mers than the weight kernel's LDS path holds."""
    if not fused_env or k != 16 or k2 != 12:
        return True
    if set(seq.upper()) - set("ACGT"):
        return True
    return len(seq) - k + 1 > CODES_MAX_KMERS


# ---- the corpus of tests/test_ordered_paths_{cpu,gpu}.py ------------------------------------------------------------------------
def _rand(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _sprinkle_n(rnd, s, count=5):
    b = list(s)
    for i in rnd.sample(range(len(b)), count):
        b[i] = "N"
    return "".join(b)


# Three 12-mers whose hashes share the top 22 bits and are the smallest of the read they sit in (found once by hashing the 12-mers of 3 x 10^7 random bases
# 12-mers with oracle_lib.kmer_hashes32 and keeping the lowest hash prefix with three members): at S = 1 and S = 2 the exact selection of
# LEVEL2_READ's forward strand passes levels 0 and 1 with more than cap keys in the chosen bin and ends at level 2.
LEVEL2_KMERS = ("TTTGCAAATTAC", "ACACCGTAGCTG", "AGATTGAGTAGG")


def corpus():
    """name -> read.  Random reads come from one fixed seed, in this order."""
    import random
    rnd = random.Random(20261)
    c = {}
    for n in (2000, 2059, 2060, 5000, 30000):           # n = 1 989, 2 048 (= cap at S = 1536), 2 049, ...
        c[f"r{n}"] = _rand(rnd, n)
    for n in (2058, 4107, 4108):                        # trip edges: 2 047, 4 096, 4 097 k2-mers (2 048 and 2 049: r2059, r2060)
        c[f"r{n}"] = _rand(rnd, n)
    for n in (2048, 2049, 2063, 2064, 2065, 4095, 4096, 4097, 4111, 4112, 4113):   # lengths = 0, 1, 15 (mod 16) next to the trip edges
        c[f"r{n}"] = _rand(rnd, n)
    for n in (74, 75, 76, 310, 311, 312, 410, 411, 412):   # n = S - 1, S, S + 1 at S = 64, 300, 400
        c[f"r{n}"] = _rand(rnd, n)
    c["polyA"] = "A" * 3000
    c["polyC"] = "C" * 3000
    c["polyG"] = "G" * 3000
    c["acgttgca"] = "ACGTTGCA" * 400
    c["r3000+polyA"] = _rand(rnd, 3000) + "A" * 3000
    c["tandem40x60"] = _rand(rnd, 2000) + _rand(rnd, 40) * 60 + _rand(rnd, 2000)
    half = _rand(rnd, 2500)
    c["dup2500x2"] = half + half
    c["level2"] = _rand(rnd, 900) + "".join(LEVEL2_KMERS) + _rand(rnd, 900)
    for name in ("r2060", "r5000", "r4108", "r3000+polyA", "tandem40x60"):     # raw-byte reads: MHAP_RD_MAT next to packed strands
        c[name + "+N"] = _sprinkle_n(rnd, c[name])
    return c


def wide_corpus():
    """A launch whose longest read has more than 65 535 k2-mers: every strand of it stages 32-bit positions."""
    import random
    c = corpus()
    out = {k: c[k] for k in ("r5000", "r2060", "polyC", "r3000+polyA", "acgttgca", "r5000+N")}
    out["r70000"] = _rand(random.Random(70000), 70000)
    return out


def predict(reads, S, k=16, k2=12, fused_env=True):
    """The Path of every strand (2 i = read i forward, 2 i + 1 = its reverse strand) of one sketch() call over `reads` (name -> read)."""
    import oracle_lib as O
    seqs = list(reads.values())
    launch_max = max(len(s) for s in seqs) - k2 + 1
    out = []
    for s in seqs:
        mat = strand_is_mat(s, k, k2, fused_env)
        for t in (s, O.rc(s)):
            out.append(classify(O.kmer_hashes32(t, k2), S, launch_max, mat))
    return out


# The classes the corpus has to reach: (attempt, how) -> (corpus, S, strand names "read/0" forward, "read/1" reverse) that take it.
TABLE = {
    (ATT_NONE, HOW_ALL): ("main", 1536, ("r2000/0", "r2059/0", "r2059/1")),
    (ATT_ACCEPTED, HOW_ONEPASS): ("main", 1536, ("r2060/0", "r5000/0", "r30000/1", "dup2500x2/0")),
    (ATT_SHORT, HOW_BUCKETS0): ("main", 1536, ("r3000+polyA/0", "r3000+polyA/1")),
    (ATT_SHORT, HOW_NET0 + 4): ("main", 1536, ("polyA/0", "polyA/1", "polyC/1", "polyG/0")),
    (ATT_SHORT, HOW_NET0 + 5): ("main", 300, ("polyA/0", "polyA/1")),
    (ATT_OVER, HOW_NET0 + 4): ("main", 1536, ("polyC/0", "polyG/1")),
    (ATT_CROWDED, HOW_NET0): ("main", 1536, ("acgttgca/0", "tandem40x60/0", "tandem40x60/1")),
    (ATT_NONE, HOW_BUCKETS0): ("main", 400, ("r2000/0", "r30000/0", "r5000/1")),
    (ATT_NONE, HOW_NET0 + 1): ("main", 2048, ("r30000/0", "r30000/1", "r5000/1")),
    (ATT_NONE, HOW_NET0 + 2): ("main", 1, ("level2/0",)),
    (ATT_NONE, HOW_NET0 + 4): ("main", 2048, ("polyA/0", "polyC/0")),
    (ATT_NONE, HOW_NET0 + 5): ("main", 400, ("polyA/0", "acgttgca/0")),
}
# ... and the same under a launch that stages 32-bit positions
WIDE_TABLE = {
    (ATT_ACCEPTED, HOW_ONEPASS): ("wide", 1536, ("r5000/0", "r5000/1", "r2060/0")),
    (ATT_SHORT, HOW_BUCKETS0): ("wide", 1536, ("r3000+polyA/0",)),
    (ATT_OVER, HOW_NET0 + 4): ("wide", 1536, ("polyC/0",)),
    (ATT_CROWDED, HOW_NET0): ("wide", 1536, ("r70000/0", "r70000/1", "acgttgca/0")),
}
MAIN_S = (1536, 300, 400, 100, 2048, 64, 1, 2)
WIDE_S = (1536,)


def strand_index(reads, name):
    read, strand = name.rsplit("/", 1)
    return 2 * list(reads).index(read) + int(strand)
