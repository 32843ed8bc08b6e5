"""Select each read's best overlaps on the GPU: `python -m mhap_amd.best_overlaps overlaps.txt reads.fasta [queries.fasta] [-n N]
[--min-span S] [--min-identity X] [--band W] [--table t.tsv] [-o kept.txt]` realigns the overlaps as `python -m mhap_amd.realign` does,
gives every view of a record (the record as seen from its first and from its second read) a key, the counted matches on that read, and
keeps for every read the N views with the greatest keys, ties at the last place included (api.SelectSession; the contract is the
"overlap selection" section of include/mhap_hip.h).

Output: the realigned records that keep at least one view, 12 columns each, in the input's order.  --table writes one line per read,
`read_id entries kept threshold`; one line on stderr gives the counts.  --min-identity drops realigned records below it before the
selection, as the other tools do.
"""
import argparse
import sys

from . import api
from .realign import keep, read_overlaps


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.best_overlaps", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("queries", nargs="?")
    ap.add_argument("-n", "--best-overlaps", type=int, default=api.SELECT_DEFAULTS["best_n"], metavar="N", help="views a read keeps (40)")
    ap.add_argument("--min-span", type=int, default=api.SELECT_DEFAULTS["min_span"], metavar="S", help="a view shorter than this is no evidence (500)")
    ap.add_argument("--min-identity", type=float, default=0.0)
    ap.add_argument("--band", type=int, default=0, help="half-width of the band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--query-id-offset", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--table", default=None, help="write one line per read: read_id entries kept threshold")
    ap.add_argument("-o", "--output", default=None, help="the file of kept records to write (default: stdout)")
    a = ap.parse_args(argv)
    if a.best_overlaps < 1:
        ap.error("-n must be >= 1")
    if a.min_span < 0:
        ap.error("--min-span must be >= 0")
    if a.band < 0:
        ap.error("--band must be >= 0")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    queries = api.FastaData.from_file(a.queries, len(fasta) if a.query_id_offset is None else a.query_id_offset) if a.queries else None
    with api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=a.max_shift, device=a.device)) as ms:
        out, _ = api.realign_records(recs, fasta, band=a.band, handle=ms, query_fasta=queries)
        kept = keep(out, a.min_identity)
        views, rows, counts, ids = api.select_overlaps(kept, fasta, best_n=a.best_overlaps, min_span=a.min_span, query_fasta=queries, handle=ms)
    text = "".join(line + "\n" for line in api.records_to_lines(kept[views != 0]))
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if a.table:
        with open(a.table, "w") as fh:
            fh.write(api.select_table_text(ids, rows))
    print(api.select_counts_line([counts[k] for k in api.SELECT_COUNTS]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
