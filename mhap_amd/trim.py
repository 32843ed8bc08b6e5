"""Trim reads and split chimeras on the GPU from a file of MHAP overlaps: `python -m mhap_amd.trim overlaps.txt reads.fasta [--band W]
[--min-identity X] [--min-cov N] [--end-clip N] [--min-span N] [--penalty N] [--repeat-filter [--repeat-factor PCT] [--repeat-max-cov N]
[--repeat-min-run N] [--repeat-min-unique N]] -o trimmed.fasta [--table t.tsv] [--records trimmed.txt]` writes what
`mhap-hip --realign --trim --trim-fasta trimmed.fasta --trim-table t.tsv` writes for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does; the records that tool would drop (no alignment, or an
identity below --min-identity) take no part.  Every other record is first cut to the best stretch of its alignment under +1 per match
and --penalty per error column, so that an overlap which the aligner ran through a chimeric junction ends there.  Its two aligned intervals, shrunk by --end-clip at both ends, are piled
up on their reads, and a read keeps the longest stretch that --min-cov of them cover, widened again by --end-clip (api.TrimSession;
the contract is the "read trimming" section of include/mhap_hip.h).  A chimeric read falls into two stretches at its junction and
keeps the longer.  Output is FASTA, one unwrapped line per surviving read: `>ID len=<trimmed length> begin=<first base kept>
end=<one past the last> runs=<stretches>`, the ids numeric as the records print them; --table writes one line per read, deleted ones
included: `id length begin end runs covered flags`, tab-separated; --records writes the overlaps rewritten onto the trimmed reads, the
void ones left out.  One line on stderr gives the counts.
With --repeat-filter the refined overlaps that lie in nothing but repeat are set aside first and count as no support (`python -m
mhap_amd.repeats`; "repeat marking" in the same header, with its two-copy limit); one more line on stderr, in front.
Not done: a second round on the trimmed overlaps; no selection of best overlaps in front of the trimming (python -m mhap_amd.best_overlaps
selects for the read correction only).
"""
import argparse
import sys

import numpy as np

from . import api, repeats
from .correct import select_paths
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned and piled up per call


def format_fasta(fasta, rows, flags):
    """The trimmed reads as FASTA text; `fasta` holds the untrimmed reads in the order of `rows`."""
    out = []
    for r, (row, f) in enumerate(zip(np.asarray(rows).tolist(), np.asarray(flags).tolist())):
        if f & api.TRIM_DELETED:
            continue
        o = int(fasta.offsets[r])
        out.append(f">{int(fasta.ids[r])} len={row[1] - row[0]} begin={row[0]} end={row[1]} runs={row[2]}\n"
                   f"{fasta.bases[o + row[0]:o + row[1]].tobytes().decode('latin-1')}\n")
    return "".join(out)


def format_table(ids, lengths, rows, flags):
    """One line per read: id, length, begin, end, runs, covered, flags, tab-separated."""
    return "".join(f"{i}\t{n}\t{row[0]}\t{row[1]}\t{row[2]}\t{row[3]}\t{f}\n"
                   for i, n, row, f in zip(np.asarray(ids).tolist(), np.asarray(lengths).tolist(), np.asarray(rows).tolist(),
                                           np.asarray(flags).tolist()))


def trim_overlaps(recs, fasta, band=0, max_shift=0.2, min_identity=0.0, device=0, batch=BATCH, handle=None, penalty=api.TRIM_PENALTY, repeat=None,
                  **params):
    """Realign `recs` in batches with their paths, cut every kept record to the best stretch of its path (penalty 0: not at all) and
    trim: a dict of rows, flags, counts, records (the kept realigned records, refined, untrimmed), applied
    (those rewritten onto the trimmed reads, void ones left out) and reads (the surviving reads, a FastaData over fasta's bases).
    repeat: None, or a dict of RepeatSession's parameters: the refined records go through the repeat stage first ("repeat marking"
    in include/mhap_hip.h), only its survivors are piled up and are `records`, and its dict is the key `repeat`."""
    ms = handle or api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device))
    try:
        if repeat is not None:   # the repeat session has freed its device arrays before the trim session allocates its own
            from .repeats import mark_records, refined_overlaps
            _, cut = refined_overlaps(recs, fasta, ms, band=band, min_identity=min_identity, batch=batch, penalty=penalty)
            marked = mark_records(cut, fasta.ids, fasta.lengths, ms, **repeat)
            kept = cut[marked["keep"] != 0]
            with api.TrimSession(fasta.ids, fasta.lengths, handle=ms, **params) as ts:
                ts.add(kept)
                counts = ts.finish()
                rows, flags = ts.table()
                out, keep = ts.apply(kept)
                return dict(rows=rows, flags=flags, counts=counts, records=kept, applied=out[keep != 0], reads=ts.trimmed(fasta), repeat=marked)
        with api.TrimSession(fasta.ids, fasta.lengths, handle=ms, **params) as ts:
            kept = []
            for q0 in range(0, len(recs), batch):
                out, _, op_offsets, ops = api.realign_records_paths(recs[q0:q0 + batch], fasta, band=band, handle=ms)
                rows = kept_rows(out, min_identity)
                if penalty > 0:
                    out = api.trim_refine(out[rows], *select_paths(op_offsets, ops, rows), penalty=penalty, handle=ms)
                else:
                    out = out[rows]
                ts.add(out)
                kept.append(out)
            counts = ts.finish()
            rows, flags = ts.table()
            kept = np.concatenate(kept) if kept else np.zeros(0, api.RECORD_DTYPE)
            out, keep = ts.apply(kept)
            return dict(rows=rows, flags=flags, counts=counts, records=kept, applied=out[keep != 0], reads=ts.trimmed(fasta))
    finally:
        if handle is None:
            ms.close()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.trim", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("--band", type=int, default=0, help="half-width of the realignment band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0, help="overlaps realigned below this identity take no part")
    ap.add_argument("--min-cov", type=int, default=3, help="the shrunk overlaps a position needs to be kept")
    ap.add_argument("--end-clip", type=int, default=500, help="the bases every aligned interval is shrunk by at both ends")
    ap.add_argument("--min-span", type=int, default=2000, help="the shortest aligned interval that counts")
    ap.add_argument("--penalty", type=int, default=api.TRIM_PENALTY,
                    help="the cost of an error column next to +1 for a match when every overlap is cut to the best stretch of its alignment; 0: overlaps as realigned")
    ap.add_argument("--repeat-filter", action="store_true", help="set aside the overlaps that lie in nothing but repeat before the pile-up")
    repeats.add_arguments(ap, "repeat-")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default=None, help="the FASTA file of the trimmed reads (default: stdout)")
    ap.add_argument("--table", default=None, help="also write one line per read: id length begin end runs covered flags")
    ap.add_argument("--records", default=None, help="also write the overlaps rewritten onto the trimmed reads")
    a = ap.parse_args(argv)
    if a.band < 0:
        ap.error("--band must be >= 0")
    if a.min_cov < 1 or a.end_clip < 0 or a.min_span < 0 or a.penalty < 0:
        ap.error("--min-cov must be >= 1, --end-clip, --min-span and --penalty >= 0")
    rp, message = repeats.parameters(a, "repeat-")
    if message:
        ap.error(message)
    if rp != {k: v for k, v in api.REPEAT_DEFAULTS.items() if k in rp} and not a.repeat_filter:
        ap.error("--repeat-factor, --repeat-max-cov, --repeat-min-run and --repeat-min-unique need --repeat-filter")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    res = trim_overlaps(recs, fasta, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity, device=a.device, min_cov=a.min_cov,
                        end_clip=a.end_clip, min_span=a.min_span, penalty=a.penalty, repeat=rp if a.repeat_filter else None)
    text = format_fasta(fasta, res["rows"], res["flags"])
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if a.table:
        with open(a.table, "w") as fh:
            fh.write(format_table(fasta.ids, fasta.lengths, res["rows"], res["flags"]))
    if a.records:
        with open(a.records, "w") as fh:
            fh.write("".join(l + "\n" for l in api.records_to_lines(res["applied"])))
    if a.repeat_filter:
        print(api.repeat_counts_line([res["repeat"]["counts"][k] for k in api.REPEAT_COUNTS]), file=sys.stderr)
    print(api.trim_counts_line([res["counts"][k] for k in api.TRIM_COUNTS]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
