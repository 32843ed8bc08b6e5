"""Mark variant sites from the pile-up of a file of MHAP overlaps on the GPU and set aside the overlaps whose reads disagree across them:
`python -m mhap_amd.variants overlaps.txt reads.fasta [--band W] [--min-identity X] [--min-depth N] [--min-minor N] [--min-pct PCT]
[--max-del-pct PCT] [--min-diff N] [--diff-pct PCT] [--table sites.tsv] [--judged judged.tsv] [-o kept_overlaps.txt]` marks what
`mhap-hip --realign --variant-filter --variant-table sites.tsv` marks for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does; the records that tool would drop (no alignment, or an
identity below --min-identity) take no part.  Every other record votes column by column on both of its reads (A, C, G, T, deletion;
no insertions, every vote 1).  A position is a site when it is at least --min-depth deep, its second allele has at least --min-minor
votes and --min-pct percent of the depth, and deletions are at most --max-del-pct percent of it.  Every overlap is then walked again:
a column on a site of either read whose two bases are the site's two alleles agrees or disagrees, and an overlap with at least
--min-diff disagreeing columns that are at least --diff-pct percent of the two together is set aside (api.VariantSession; the
contract is the "variant sites" section of include/mhap_hip.h).  -o writes the kept overlaps, as realigned (default: stdout); --table
writes one line per site: `read_id pos major minor n_major n_minor depth`, tab-separated, pos 0-based, the bases as letters; --judged
writes one line per realigned overlap: its two ids, informative, agree, disagree, other and the keep flag.  One line on stderr
gives the counts.
Not done: quality-weighted votes, indel variants, phasing, haplotype-aware correction and consensus.
"""
import argparse
import sys

import numpy as np

from . import api
from .correct import select_paths
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned per call
PARAMETERS = ("min-depth", "min-minor", "min-pct", "max-del-pct", "min-diff", "diff-pct")


def format_table(ids, offsets, sites):
    """One line per site: read_id, pos, major, minor (letters), n_major, n_minor, depth, tab-separated, in the order of the reads."""
    per_read = np.diff(np.asarray(offsets))
    who = np.repeat(np.asarray(ids), per_read)
    return "".join(f"{i}\t{p}\t{'ACGT'[a]}\t{'ACGT'[b]}\t{na}\t{nb}\t{d}\n" for i, (p, a, b, na, nb, d) in zip(who.tolist(), np.asarray(sites).tolist()))


def format_judged(records, tallies, keep):
    """One line per judged overlap: from_id, to_id, informative, agree, disagree, other, keep, tab-separated."""
    return "".join(f"{int(r['from_id'])}\t{int(r['to_id'])}\t{t[0]}\t{t[1]}\t{t[2]}\t{t[3]}\t{int(k)}\n"
                   for r, t, k in zip(records, np.asarray(tallies).tolist(), np.asarray(keep).tolist()))


def realigned_paths(recs, fasta, ms, band=0, min_identity=0.0, batch=BATCH):
    """Per batch of `recs`: (the rows of recs that `python -m mhap_amd.realign` keeps, those records as realigned, their run offsets,
    their runs)."""
    for q0 in range(0, len(recs), batch):
        out, _, op_offsets, ops = api.realign_records_paths(recs[q0:q0 + batch], fasta, band=band, handle=ms)
        rows = kept_rows(out, min_identity)
        yield (rows + q0, out[rows]) + select_paths(op_offsets, ops, rows)


def variant_overlaps(recs, fasta, band=0, max_shift=0.2, min_identity=0.0, device=0, batch=BATCH, handle=None, **params):
    """Realign, vote, mark and judge: a dict of counts, rows, offsets, sites, realigned (the records judged), found_rows (their rows in
    `recs`), keep and tallies.  The paths of every batch wait on the host between the vote and the judgement; the driver realigns a
    second time instead."""
    ms = handle or api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device))
    try:
        with api.VariantSession(fasta, handle=ms, **params) as vs:
            batches = list(realigned_paths(recs, fasta, ms, band=band, min_identity=min_identity, batch=batch))
            for _, out, op_offsets, ops in batches:
                vs.add(out, op_offsets, ops)
            counts = vs.finish()
            rows, offsets, sites = vs.table()
            judged = [vs.apply(out, op_offsets, ops) for _, out, op_offsets, ops in batches]
        cat = lambda parts, empty: np.concatenate(parts) if parts else empty   # noqa: E731
        return dict(counts=counts, rows=rows, offsets=offsets, sites=sites,
                    found_rows=cat([b[0] for b in batches], np.zeros(0, np.int64)), realigned=cat([b[1] for b in batches], np.zeros(0, api.RECORD_DTYPE)),
                    keep=cat([j[0] for j in judged], np.zeros(0, np.uint8)), tallies=cat([j[1] for j in judged], np.zeros((0, 4), np.int32)))
    finally:
        if handle is None:
            ms.close()


def add_arguments(ap, prefix=""):
    """The stage's parameters as --{prefix}min-depth ... (the graph tool takes them as --variant-...)."""
    d = api.VARIANT_DEFAULTS
    says = {"min-depth": "the depth, own base included, a position needs to be a site",
            "min-minor": "the votes the second allele of a site needs",
            "min-pct": "the share of the depth the second allele of a site needs, in percent",
            "max-del-pct": "the greatest share of deletions in the depth of a site, in percent",
            "min-diff": "the disagreeing site columns an overlap needs to be set aside",
            "diff-pct": "the share of disagreeing among the agreeing and disagreeing site columns an overlap needs to be set aside, in percent"}
    for k in PARAMETERS:
        ap.add_argument(f"--{prefix}{k}", type=int, default=d[k.replace("-", "_")], help=says[k])


def parameters(a, prefix=""):
    """The dict of VariantSession's parameters from parsed arguments, or a message."""
    p = {k.replace("-", "_"): getattr(a, (prefix + k).replace("-", "_")) for k in PARAMETERS}
    if min(p["min_depth"], p["min_minor"], p["min_diff"]) < 1 or not all(0 <= p[k] <= 100 for k in ("min_pct", "max_del_pct", "diff_pct")):
        return None, (f"--{prefix}min-depth, --{prefix}min-minor and --{prefix}min-diff must be >= 1 and --{prefix}min-pct, --{prefix}max-del-pct and "
                      f"--{prefix}diff-pct in 0 .. 100")
    return p, None


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.variants", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("--band", type=int, default=0, help="half-width of the realignment band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0, help="overlaps realigned below this identity take no part")
    add_arguments(ap)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default=None, help="the file of the kept overlaps (default: stdout)")
    ap.add_argument("--table", default=None, help="also write one line per site: read_id pos major minor n_major n_minor depth")
    ap.add_argument("--judged", default=None, help="also write one line per realigned overlap: its two ids, informative, agree, disagree, other, keep")
    a = ap.parse_args(argv)
    p, message = parameters(a)
    if message:
        ap.error(message)
    if a.band < 0:
        ap.error("--band must be >= 0")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    res = variant_overlaps(recs, fasta, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity, device=a.device, **p)
    text = "".join(l + "\n" for l in api.records_to_lines(res["realigned"][res["keep"] != 0]))
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if a.table:
        with open(a.table, "w") as fh:
            fh.write(format_table(fasta.ids, res["offsets"], res["sites"]))
    if a.judged:
        with open(a.judged, "w") as fh:
            fh.write(format_judged(res["realigned"], res["tallies"], res["keep"]))
    print(api.variant_counts_line([res["counts"][k] for k in api.VARIANT_COUNTS], int((res["keep"] == 0).sum()), len(res["keep"])), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
