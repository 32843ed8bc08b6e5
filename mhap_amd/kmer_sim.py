"""KmerStatSimulator (J/main/KmerStatSimulator.java; docs/source/utilities.rst): simulated reads, and the k-mer similarity of
overlapping and of random read pairs, with the pair statistics computed on the GPU (mhap_amd.pair_kmer_stats).

    python -m mhap_amd.kmer_sim <#trials> <kmer size> <seq length> <overlap length> <insertion> <del> <subst>
                                [only one sequence error] [reference genome] [kmers to ignore]          (Usage 1: pair statistics)
    python -m mhap_amd.kmer_sim <#trials> <seq length> <insertion> <del> <subst> [reference genome]     (Usage 2: reads as FASTA)

takes the Java program's positional arguments, dispatches on their count as `main` does (:72-117) and writes its stdout and stderr.
The project's own options, removed before dispatch: --rng java|device (default java), --seed S (the stream's seed, default 0 = Java's
static seed) and --device N.

The trials are generated on the host by mhap_ksim_next (host_util.cpp), a replay of Java's single java.util.Random stream; chunks of
trials go to the GPU while the next chunk is generated.  Column 4 is BottomOverlapSketch.jaccardToIdentity through the C library's
log / exp (DESIGN.md §1 lists HotSpot's intrinsics as a hazard for bit parity).  Values print as Double.toString per the JDK 19+
specification (shortest round-tripping decimal; a one-digit shortest takes the closest decimal of one or two digits): JDK 8's occasional
extra digit is not reproduced.  Deliberate deviations:
  - where Java would loop forever (a reference without a record of at least 4L bases; an error mix in which every draw inserts) KsimError
    names the loop; where Java throws, KsimError carries Java's exception text and the CLI exits 1 as the uncaught exception would;
  - k = 0 and lengths below 1 are refused (Java counts empty k-mers / divides by zero); a k above L + 1 is refused before the first trial
    rather than after it (BottomSketch's NegativeArraySizeException);
  - the generated reads are all the same length, so compareKmers and compareMinHash see exactly what Java's do.
--rng device generates the trials on the GPU instead (mhap_ksim_dev_trials; its header comment documents the counter-based RNG and
its keying): Java's rules per base, pick and trim, but not Java's stream, so it matches Java in distribution only.  A trial's reads
depend only on (seed, trial index), never on the chunking.
"""
import concurrent.futures
import ctypes as C
import math
import sys
from decimal import ROUND_HALF_EVEN, Context, Decimal, localcontext

import numpy as np

from . import api, roc

BOTTOM_K = 1256     # compareMinHash: new BottomSketch(s, k, 1256, true) (:171-176)
FASTA_LINE_LENGTH = 60


class KsimError(RuntimeError):
    """What KmerStatSimulator would have thrown, exited with, or looped forever on."""


# ---- Double.toString (JDK 19+ specification) ---------------------------------------------------------------------------------
def _digits(r):
    """repr of a positive finite double -> (significant digits without trailing zeros, decimal exponent of the first digit)."""
    m, e = (r.split("e") + ["0"])[:2]
    ip, fp = (m.split(".") + [""])[:2]
    ds = ip + fp
    z = len(ds) - len(ds.lstrip("0"))
    return ds.strip("0") or "0", len(ip) - 1 + int(e) - z


def _two_digits(a, e10):
    """The decimal of one or two digits that rounds to a and is closest to it (ties: even last digit)."""
    with localcontext(Context(prec=1000)):
        X = Decimal(a)
        q = Decimal(1).scaleb(e10 - 1)
        c0 = X.quantize(q, rounding=ROUND_HALF_EVEN)
        d1 = Decimal(int(_digits(repr(a))[0])).scaleb(e10)
        cands = [c for c in (c0 - q, c0, c0 + q, d1) if c > 0 and float(c) == a]
        best = min(cands, key=lambda c: (abs(c - X), int(c.scaleb(1 - e10).to_integral_value()) & 1))
        t = best.normalize().as_tuple()
        ds = "".join(map(str, t.digits))
        return ds.rstrip("0") or "0", t.exponent + len(t.digits) - 1


def java_double(x):
    """Double.toString(x)."""
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    sign = "-" if x < 0 else ""
    a = -x if x < 0 else x
    if 1.0 <= a < 1e7 and a == int(a):
        return f"{sign}{int(a)}.0"
    ds, e10 = _digits(repr(a))
    if len(ds) == 1:
        ds, e10 = _two_digits(a, e10)
    if 1e-3 <= a < 1e7:
        if e10 >= 0:
            ip = ds[:e10 + 1].ljust(e10 + 1, "0")
            return f"{sign}{ip}.{ds[e10 + 1:] or '0'}"
        return f"{sign}0.{'0' * (-e10 - 1)}{ds}"
    return f"{sign}{ds[0]}.{ds[1:] or '0'}E{e10}"


# ---- Java arithmetic -----------------------------------------------------------------------------------------------------
def _jdiv(a, b):
    """IEEE division as Java does it (x / 0.0 is +-Infinity or NaN, never an exception)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def jaccard_to_identity(score, k):
    """BottomOverlapSketch.jaccardToIdentity (J/sketch/BottomOverlapSketch.java:391-395)."""
    s = float(score)
    v = 2.0 * s / (1.0 + s)
    lg = -math.inf if v == 0.0 else (math.nan if v != v or v < 0 else math.log(v))
    d = -1.0 / float(k) * lg
    return math.exp(-d) if d == d else math.nan


def output_stats(values):
    """outputStats (:278-299): the mean summed in trial order, the variance divided by N - 1 -> (mean, stdev)."""
    n, s = 0, 0.0
    for d in values:
        n += 1
        s += d
    mean = _jdiv(s, n)
    var = 0.0
    for d in values:
        var += (d - mean) * (d - mean)
    var = _jdiv(var, n - 1)
    return mean, (math.sqrt(var) if var >= 0 else math.nan)


def convert_to_fasta(s):
    """Utils.convertToFasta for a string without white space: 60 characters per line."""
    out, i = [], 0
    while i + FASTA_LINE_LENGTH < len(s):
        out.append(s[i:i + FASTA_LINE_LENGTH])
        i += FASTA_LINE_LENGTH
    out.append(s[i:])
    return "\n".join(out)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def load_skip_mers(path):
    """loadSkipMers (:143-152): the first white-space token of each line; a line without a second (integer) token throws."""
    mers = {}
    with open(path, "r", encoding="latin-1") as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            split = roc.java_split(line)
            if len(split) < 2:
                raise KsimError(f"java.lang.ArrayIndexOutOfBoundsException: Index 1 out of bounds for length {len(split)}")
            try:
                mers[split[0].strip()] = roc.parse_int(split[1])
            except ValueError as e:
                raise KsimError(f"java.lang.NumberFormatException: {e}") from None
    return mers


def load_reference(path):
    """The reference's records as `simulate` holds them (:339-347): FastaData order and rules, upper-cased, N removed."""
    fa = api.FastaData.from_file(path)
    b = fa.bases.tobytes()
    return [b[o:o + n].replace(b"N", b"") for o, n in zip(fa.offsets.tolist(), fa.lengths.tolist())]


def _as_records(reference):
    if reference is None:
        return None
    if isinstance(reference, str):
        return load_reference(reference)
    return [(r.encode("latin-1") if isinstance(r, str) else bytes(r)).upper().replace(b"N", b"") for r in reference]


# ---- the Java stream (mhap_ksim_*) --------------------------------------------------------------------------------------------
class _JavaTrials:
    """mhap_ksim_create / _next / _destroy: the trials of one java.util.Random stream, chunk after chunk."""

    def __init__(self, seed, L, offset, err, pi, pd, ps, one_sided, sim_only, records):
        self.lib = api.load_library()
        self.L, self.sim_only = L, sim_only
        self.roles = 1 if sim_only else 3
        recs = records or []
        self._b = np.frombuffer(b"".join(recs) or b"\0", dtype=np.uint8)
        self._len = np.array([len(r) for r in recs] or [0], dtype=np.int32)
        self._off = np.zeros(len(self._len), dtype=np.int64)
        self._off[1:] = np.cumsum(self._len[:-1], dtype=np.int64)
        flags = (1 if one_sided else 0) | (2 if sim_only else 0)   # MHAP_KSIM_ONE_SIDED, MHAP_KSIM_SIM_ONLY
        self.h = self.lib.mhap_ksim_create(int(seed), L, offset, err, pi, pd, ps, flags, api._ptr(self._b), api._ptr(self._off),
                                           api._ptr(self._len), len(recs))
        if not self.h:
            raise KsimError("mhap_ksim_create rejected its arguments")

    def next(self, n, reads=None):
        """(reads (n, roles, L) uint8, meta (n, 5) int32, trials completed, (exception text, role) or None)."""
        if reads is None:
            reads = np.zeros((n, self.roles, self.L), dtype=np.uint8)
        meta = np.zeros((max(n, 1), 5), dtype=np.int32)
        done = self.lib.mhap_ksim_next(self.h, n, reads.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p))
        if done < 0:
            raise KsimError(f"mhap_ksim_next failed ({done})")
        err = None
        if done < n:
            role = C.c_int32(-1)
            err = (self.lib.mhap_ksim_error(self.h, C.byref(role)).decode(), role.value)
        return reads, meta[:n], done, err

    def close(self):
        if self.h:
            self.lib.mhap_ksim_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _check_rng(rng):
    if rng not in ("java", "device"):
        raise KsimError(f"unknown --rng {rng!r}: 'java' (java.util.Random replayed on the host) or 'device' (generated on the GPU)")


def _ref_arrays(records):
    if not records:
        return None, None, None
    b = np.frombuffer(b"".join(records) or b"\0", dtype=np.uint8)
    ln = np.array([len(r) for r in records], dtype=np.int32)
    off = np.zeros(len(ln), dtype=np.int64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.int64)
    return b, off, ln


def _device_chunk(L, roles):
    return max(1, (256 << 20) // (roles * L))


def _dev_call(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except api.MhapError as e:
        raise KsimError(e.args[0]) from None


def _rates(ins, dele, sub):
    """simulate's error rate and percentages (:326-335); KsimError for a rate outside [0, 1] (Java's message) or a mix that never ends."""
    err = ins + dele + sub
    pi, pd, ps = _jdiv(ins, err), _jdiv(dele, err), _jdiv(sub, err)
    if err < 0 or err > 1:
        raise KsimError("Error rate must be between 0 and 1")
    return err, pi, pd, ps


def _check_terminates(err, pi, ps):
    # every base errs (nextDouble() < 1 always), no draw substitutes and every draw inserts: the ListIterator walk never advances
    if err >= 1.0 and not ps > 0.0 and pi + ps >= 1.0:
        raise KsimError("every draw is an insertion at error rate 1: getSequence would never finish (Java loops forever)")


def _check_reference(records, L):
    if records is None:
        return
    if not records:
        raise KsimError("java.lang.IllegalArgumentException: bound must be positive")
    if not any(len(r) >= 4 * L for r in records):
        raise KsimError(f"no reference record has at least 4 * {L} bases: simulate would draw seqID forever (Java loops forever)")


def _java_int(x):
    """(int) of a double: truncation, NaN -> 0, saturating."""
    if x != x:
        return 0
    if x >= 2 ** 31 - 1:
        return 2 ** 31 - 1
    if x <= -2 ** 31:
        return -2 ** 31
    return int(x)


def simulate_reads(n, length, ins, dele, sub, reference=None, rng="java", seed=0, device=0, chunk=None, _progress=None):
    """Usage 2: n reads of int(length) bases, each a window of the reference (or of a fresh random sequence) with Java's errors.
    Returns (reads: uint8 array (n, L), ids: int64 array (n, 2) of (seqID, firstPos + L) as the FASTA headers print them).
    reference: a FASTA path or a list of records.  rng="java": host only; rng="device": generated on the GPU."""
    _check_rng(rng)
    err, pi, pd, ps = _rates(ins, dele, sub)
    records = _as_records(reference)
    L = _java_int(length)
    if n <= 0:
        return np.zeros((0, max(L, 0)), np.uint8), np.zeros((0, 2), np.int64)
    if L < 1:
        raise KsimError(f"sequence length {L} < 1 is not supported")
    _check_reference(records, L)
    _check_terminates(err, pi, ps)
    if rng == "device":
        reads = np.zeros((n, 1, L), dtype=np.uint8)
        meta = np.zeros((n, 5), dtype=np.int32)
        with api.KsimDevice(device) as d:
            step = chunk or _device_chunk(L, 1)
            for c0 in range(0, n, step):
                m = min(n - c0, step)
                _, r, mt, _ = _dev_call(d.trials, seed, c0, m, L, 0, err, pi, pd, ps, 2, _ref_arrays(records), 1, BOTTOM_K, [], want_reads=True)
                reads[c0:c0 + m], meta[c0:c0 + m] = r, mt
        done, e = n, None
    else:
        gen = _JavaTrials(seed, L, 0, err, pi, pd, ps, False, True, records)
        try:
            reads, meta, done, e = gen.next(n)
        finally:
            gen.close()
    ids = np.stack([meta[:, 0].astype(np.int64), meta[:, 1].astype(np.int64) + L], axis=1)
    if _progress is not None:
        _progress(reads[:done, 0], ids[:done], done, e)
    if e is not None:
        raise KsimError(e[0])
    return reads[:, 0], ids


COLUMNS = ("shared_mer_count", "shared_jaccard", "shared_minhash", "shared_identity", "random_mer_count", "random_jaccard", "random_minhash")


def _columns(st, L, k):
    """The seven output columns of trials from the (shared, total, intersect) counts of their (first, shared) and (first, random) pairs."""
    nw = max(L - k + 1, 0)
    kk = float(min(BOTTOM_K, nw))
    sh, rn = st[0::2].astype(np.float64), st[1::2].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.stack([sh[:, 0], sh[:, 0] / sh[:, 1], sh[:, 2] / kk, np.zeros(len(sh)), rn[:, 0], rn[:, 0] / rn[:, 1], rn[:, 2] / kk], axis=1)
    out[:, 3] = [jaccard_to_identity(v, k) for v in out[:, 2]]
    return out


def simulate_pairs(trials, k, length, overlap, ins, dele, sub, one_sided=False, reference=None, skip_kmers=None, rng="java", seed=0,
                   device=0, chunk=None, return_reads=False, session=None, _progress=None):
    """Usage 1 with k >= 1: a float64 array (trials, 7) of COLUMNS, the per-trial line of the Java program.  length is requestedLength
    (a double, as Java parses it); reference: a FASTA path or a list of records; skip_kmers: an iterable of k-mers (or loadSkipMers'
    dict).  rng="java": generation runs on the host in chunks while the GPU computes the previous chunk's statistics; rng="device": the
    trials are generated on the GPU and compared where they were written.  return_reads=True (rng="device", test hook): returns
    (columns, reads (trials, 3, L) uint8, meta (trials, 5), events (trials, 3, 4) = insertions, deletions, substitutions, visits of each
    walk).  session: an api.KsimDevice to reuse (its buffers and handle)."""
    _check_rng(rng)
    if k < 1:
        raise KsimError(f"k-mer size {k} is not supported by the pair statistics (k < 0 only simulates reads; k = 0 is refused)")
    if overlap > length:
        raise KsimError("Cannot have overlap > sequence length")
    err, pi, pd, ps = _rates(ins, dele, sub)
    records = _as_records(reference)
    L = _java_int(length)
    if trials <= 0:
        return np.zeros((0, 7))
    if L < 1:
        raise KsimError(f"sequence length {L} < 1 is not supported")
    _check_reference(records, L)
    _check_terminates(err, pi, ps)
    if L - k + 1 < 0:
        raise KsimError(f"java.lang.NegativeArraySizeException: {L - k + 1}")
    skip = sorted(skip_kmers) if skip_kmers is not None else []
    offset = _java_int(length * 2 - overlap)
    if rng == "device":
        if length != L:
            if _progress is not None:
                _progress(0, 0, ("", 0))
            raise KsimError(f"Error wrong length first: {L} second: {L} requested {java_double(length)}")
        return _simulate_pairs_device(trials, k, L, offset, err, pi, pd, ps, one_sided, records, skip, seed, device, chunk, return_reads,
                                      session, _progress)
    if length != L:   # Java's length check after trial 0's second read (:389), unless one of those two reads threw first
        g0 = _JavaTrials(seed, L, offset, err, pi, pd, ps, one_sided, False, records)
        _, _, done, e = g0.next(1)
        g0.close()
        if _progress is not None:
            _progress(0, 0, ("", 0))
        if e is not None and e[1] < 2:
            raise KsimError(e[0])
        raise KsimError(f"Error wrong length first: {L} second: {L} requested {java_double(length)}")
    gen = _JavaTrials(seed, L, offset, err, pi, pd, ps, one_sided, False, records)
    if chunk is None:
        chunk = max(1, min(trials, (64 << 20) // (3 * L)))
    import torch
    bufs = [torch.empty(chunk * 3 * L, dtype=torch.uint8).pin_memory().numpy().reshape(chunk, 3, L) for _ in range(2)]
    pair_rows = np.zeros((2 * chunk, 4), dtype=np.int64)
    t = np.arange(chunk, dtype=np.int64) * 3 * L
    pair_rows[0::2, 0] = t; pair_rows[0::2, 2] = t + L
    pair_rows[1::2, 0] = t; pair_rows[1::2, 2] = t + 2 * L
    pair_rows[:, 1] = L; pair_rows[:, 3] = L
    out = np.zeros((trials, 7))
    ses = session or api.KsimDevice(device)
    pool = concurrent.futures.ThreadPoolExecutor(1)
    try:
        pending, c0, b = None, 0, 0
        while c0 < trials:
            m = min(chunk, trials - c0)
            reads, meta, done, e = gen.next(m, bufs[b][:m])
            if _progress is not None:
                _progress(c0, done, e)
            if e is not None:
                raise KsimError(e[0])
            if pending is not None:
                pc0, pm, f = pending
                out[pc0:pc0 + pm] = _columns(f.result(), L, k)
            f = pool.submit(ses.pair_stats, bufs[b].reshape(-1)[:m * 3 * L], pair_rows[:2 * m], k, BOTTOM_K, skip)
            pending = (c0, m, f)
            c0 += m
            b ^= 1
        if pending is not None:
            pc0, pm, f = pending
            out[pc0:pc0 + pm] = _columns(f.result(), L, k)
    finally:
        pool.shutdown(wait=True)
        if session is None:
            ses.close()
        gen.close()
    return out


def _simulate_pairs_device(trials, k, L, offset, err, pi, pd, ps, one_sided, records, skip, seed, device, chunk, return_reads, session,
                           _progress):
    chunk = chunk or _device_chunk(L, 3)
    out = np.zeros((trials, 7))
    reads = np.zeros((trials, 3, L), dtype=np.uint8) if return_reads else None
    meta = np.zeros((trials, 5), dtype=np.int32)
    events = np.zeros((trials, 3, 4), dtype=np.int32)
    ref = _ref_arrays(records)
    ses = session or api.KsimDevice(device)
    try:
        for c0 in range(0, trials, chunk):
            m = min(chunk, trials - c0)
            if _progress is not None:
                _progress(c0, m, None)
            st, r, mt, ev = _dev_call(ses.trials, seed, c0, m, L, offset, err, pi, pd, ps, 1 if one_sided else 0, ref, k, BOTTOM_K, skip,
                                      want_reads=return_reads)
            out[c0:c0 + m] = _columns(st.reshape(2 * m, 3), L, k)
            meta[c0:c0 + m], events[c0:c0 + m] = mt, ev
            if return_reads:
                reads[c0:c0 + m] = r
    finally:
        if session is None:
            ses.close()
    return (out, reads, meta, events) if return_reads else out


# ---- the command line --------------------------------------------------------------------------------------------------------
USAGE = ("Example usage: simulateSharedKmers <#trials> <kmer size> <seq length> <overlap length> <insertion> <del> <subst> "
         "[only one sequence error] [reference genome] [kmers to ignore]\n"
         "Usage 2: simulateSharedKmers <#trials> <seq length> <insertion> <del> <subst> [reference genome]\n")
STAT_NAMES = ("Shared mer counts", "Shared jaccard", "Shared MinHash jaccard", "Random mer counts", "Random jaccard", "Random MinHash jaccard")
_STAT_COLUMNS = (0, 1, 2, 4, 5, 6)


def format_lines(cols):
    """stdout of Usage 1: the per-trial lines and the six stats lines."""
    lines = ["\t".join(java_double(v) for v in row) for row in cols.tolist()]
    for name, c in zip(STAT_NAMES, _STAT_COLUMNS):
        mean, sd = output_stats(cols[:, c].tolist())
        lines.append(f"{name} stats: {java_double(mean)}\t{java_double(sd)}")
    return "".join(x + "\n" for x in lines)


def _own_options(argv):
    opts, rest, i = {"rng": "java", "seed": 0, "device": 0}, [], 0
    while i < len(argv):
        a = argv[i]
        name = next((o for o in ("rng", "seed", "device") if a == "--" + o or a.startswith(f"--{o}=")), None)
        if name is None:
            rest.append(a)
            i += 1
            continue
        if "=" in a:
            v = a.split("=", 1)[1]
            i += 1
        else:
            if i + 1 >= len(argv):
                raise KsimError(f"--{name} needs a value")
            v = argv[i + 1]
            i += 2
        opts[name] = v if name == "rng" else int(v)
    return opts, rest


def main(argv=None, out=None, err=None):
    out = out or sys.stdout
    err = err or sys.stderr
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        opts, args = _own_options(argv)
        _check_rng(opts["rng"])
    except (KsimError, ValueError) as e:
        err.write(f"error: {e}\n")
        return 2
    n = len(args)
    if 5 <= n <= 6:
        usage1 = False
    elif n >= 7:
        usage1 = True
    else:
        err.write(USAGE)
        return 1
    try:
        trials = roc.parse_int(args[0])
        k, overlap, one_sided, reference, skip = -1, 100, False, None, None
        if usage1:
            length = roc.parse_double(args[2])
            k = roc.parse_int(args[1])
            overlap = roc.parse_int(args[3])
            if n > 7:
                one_sided = args[7].lower() == "true"
            if n > 8:
                reference = args[8]
            if overlap > length:
                err.write("Cannot have overlap > sequence length\n")
                return 1
            if n > 9:
                skip = load_skip_mers(args[9])
            ins, dele, sub = (roc.parse_double(a) for a in args[4:7])
        else:
            length = roc.parse_double(args[1])
            if n > 5:
                reference = args[5]
            ins, dele, sub = (roc.parse_double(a) for a in args[2:5])
    except ValueError as e:
        err.write(f'Exception in thread "main" java.lang.NumberFormatException: {e}\n')
        return 1
    except KsimError as e:
        err.write(f'Exception in thread "main" {e}\n')
        return 1
    if k == 0:
        err.write("error: a k-mer size of 0 is not supported (Java would count empty k-mers)\n")
        return 1
    try:
        _rates(ins, dele, sub)
    except KsimError as e:
        err.write(f"{e}\n")
        return 1
    err.write("Started...\n")
    try:
        records = load_reference(reference) if reference is not None else None
    except api.MhapError as e:
        err.write(f'Exception in thread "main" {e}\n')
        return 1
    err.write("Loaded reference\n")
    done_lines = lambda lo, hi: err.write("".join(f"Done {i}/{trials}\n" for i in range(lo, hi) if i % 100 == 0))   # noqa: E731
    try:
        if k < 0:
            def show(reads, ids, done, e):
                done_lines(0, done + (1 if e is not None else 0))
                out.write("".join(f">s{i} {ids[i, 0]} {ids[i, 1]}\n{convert_to_fasta(reads[i].tobytes().decode('latin-1'))}\n"
                                  for i in range(done)))
            simulate_reads(trials, length, ins, dele, sub, reference=records, rng=opts["rng"], seed=opts["seed"], device=opts["device"],
                           _progress=show)
            return 0

        def progress(c0, done, e):
            done_lines(c0, c0 + done + (1 if e is not None else 0))
        cols = simulate_pairs(trials, k, length, overlap, ins, dele, sub, one_sided=one_sided, reference=records, skip_kmers=skip,
                              rng=opts["rng"], seed=opts["seed"], device=opts["device"], _progress=progress)
        if len(cols):
            out.write(format_lines(cols))
    except KsimError as e:
        text = str(e)
        if text.startswith("Error wrong length") or text.startswith("Error rate") or text.startswith("Cannot have"):
            err.write(text + "\n")
        else:
            err.write(f'Exception in thread "main" {text}\n')
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
