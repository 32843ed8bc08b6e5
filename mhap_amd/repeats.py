"""Mark repeats from the pile-up of a file of MHAP overlaps on the GPU and drop the overlaps that lie in nothing but repeat:
`python -m mhap_amd.repeats overlaps.txt reads.fasta [--band W] [--min-identity X] [--factor PCT] [--max-cov N] [--min-run N]
[--min-unique N] [--penalty N] [--table t.tsv] [-o kept_overlaps.txt]` marks what `mhap-hip --realign --repeat-filter --repeat-table t.tsv`
marks for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does; the records that tool would drop (no alignment, or an
identity below --min-identity) take no part.  Every other record is first cut to the best stretch of its alignment (the trimming's
refinement, --penalty): the local alignment runs on through unrelated flank, which would hand a false overlap an anchor it does not
have.  The refined intervals are piled up per read, the typical depth D is the lower median of the covered positions, and the
stretches of at least --min-run positions deeper than D * --factor / 100 (or than --max-cov) are a read's repeat intervals
(api.RepeatSession; the contract is the "repeat marking" section of include/mhap_hip.h).  An overlap is kept when at least
--min-unique of its aligned bases lie outside the intervals on both of its reads.  -o writes the kept overlaps, as realigned (default:
stdout); --table writes one line per interval: `read_id begin end`, tab-separated.  One line on stderr gives the counts, D and the
threshold.
Not done: a two-copy repeat at ordinary depth is not reliably found; intervals are neither padded nor merged; one round.
"""
import argparse
import sys

import numpy as np

from . import api
from .correct import select_paths
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned per call


def format_table(ids, offsets, intervals):
    """One line per interval: read_id, begin, end, tab-separated, in the order of the reads."""
    per_read = np.diff(np.asarray(offsets))
    who = np.repeat(np.asarray(ids), per_read)
    return "".join(f"{i}\t{b}\t{e}\n" for i, (b, e) in zip(who.tolist(), np.asarray(intervals).tolist()))


def refined_overlaps(recs, fasta, ms, band=0, min_identity=0.0, batch=BATCH, penalty=api.TRIM_PENALTY):
    """(realigned, refined): the records `python -m mhap_amd.realign` keeps, as realigned and cut to the best stretch of their
    paths (penalty 0: the same records twice)."""
    plain, cut = [np.zeros(0, api.RECORD_DTYPE)], [np.zeros(0, api.RECORD_DTYPE)]
    for q0 in range(0, len(recs), batch):
        out, _, op_offsets, ops = api.realign_records_paths(recs[q0:q0 + batch], fasta, band=band, handle=ms)
        rows = kept_rows(out, min_identity)
        plain.append(out[rows])
        cut.append(api.trim_refine(out[rows], *select_paths(op_offsets, ops, rows), penalty=penalty, handle=ms) if penalty > 0 else out[rows])
    return np.concatenate(plain), np.concatenate(cut)


def mark_records(refined, ids, lengths, ms, **params):
    """Pile `refined` up, mark and judge them: a dict of counts, rows, flags, offsets, intervals, hist, keep and unique.  The
    session's device arrays are freed before this returns."""
    with api.RepeatSession(ids, lengths, handle=ms, **params) as rs:
        rs.add(refined)
        counts = rs.finish()
        rows, flags, offsets, intervals = rs.table()
        keep, unique = rs.apply(refined)
        return dict(counts=counts, rows=rows, flags=flags, offsets=offsets, intervals=intervals, hist=rs.histogram(), keep=keep, unique=unique)


def repeat_overlaps(recs, fasta, band=0, max_shift=0.2, min_identity=0.0, device=0, batch=BATCH, handle=None, penalty=api.TRIM_PENALTY, **params):
    """Realign, refine, mark and judge: mark_records' dict with realigned and refined (the records judged, in the same order)."""
    ms = handle or api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device))
    try:
        plain, cut = refined_overlaps(recs, fasta, ms, band=band, min_identity=min_identity, batch=batch, penalty=penalty)
        res = mark_records(cut, fasta.ids, fasta.lengths, ms, **params)
        res.update(realigned=plain, refined=cut)
        return res
    finally:
        if handle is None:
            ms.close()


def add_arguments(ap, prefix=""):
    """The stage's parameters as --{prefix}factor ... (the graph and trim tools take them as --repeat-...)."""
    d = api.REPEAT_DEFAULTS
    ap.add_argument(f"--{prefix}factor", type=int, default=d["factor_pct"], help="a position is repeat when its depth exceeds the typical depth times this, in percent")
    ap.add_argument(f"--{prefix}max-cov", type=int, default=d["max_cov"], help="the depth above which a position is repeat; 0: derive it from the typical depth")
    ap.add_argument(f"--{prefix}min-run", type=int, default=d["min_run"], help="the shortest stretch of repeat positions that is marked")
    ap.add_argument(f"--{prefix}min-unique", type=int, default=d["min_unique"], help="the aligned bases outside repeats an overlap needs on both reads")


def parameters(a, prefix=""):
    """The dict of RepeatSession's parameters from parsed arguments, or a message."""
    g = lambda k: getattr(a, (prefix + k).replace("-", "_"))
    p = dict(factor_pct=g("factor"), max_cov=g("max-cov"), min_run=g("min-run"), min_unique=g("min-unique"))
    if p["factor_pct"] < 100 or p["max_cov"] < 0 or p["min_run"] < 1 or p["min_unique"] < 0:
        return None, f"--{prefix}factor must be >= 100, --{prefix}max-cov >= 0, --{prefix}min-run >= 1 and --{prefix}min-unique >= 0"
    return p, None


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.repeats", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("--band", type=int, default=0, help="half-width of the realignment band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0, help="overlaps realigned below this identity take no part")
    add_arguments(ap)
    ap.add_argument("--penalty", type=int, default=api.TRIM_PENALTY,
                    help="the cost of an error column next to +1 for a match when every overlap is cut to the best stretch of its alignment; 0: overlaps as realigned")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default=None, help="the file of the kept overlaps (default: stdout)")
    ap.add_argument("--table", default=None, help="also write one line per repeat interval: read_id begin end")
    a = ap.parse_args(argv)
    p, message = parameters(a)
    if message:
        ap.error(message)
    if a.band < 0 or a.penalty < 0:
        ap.error("--band and --penalty must be >= 0")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    res = repeat_overlaps(recs, fasta, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity, device=a.device, penalty=a.penalty, **p)
    text = "".join(l + "\n" for l in api.records_to_lines(res["realigned"][res["keep"] != 0]))
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if a.table:
        with open(a.table, "w") as fh:
            fh.write(format_table(fasta.ids, res["offsets"], res["intervals"]))
    print(api.repeat_counts_line([res["counts"][k] for k in api.REPEAT_COUNTS]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
