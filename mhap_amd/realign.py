"""Realign a file of MHAP overlaps on the GPU: `python -m mhap_amd.realign overlaps.txt reads.fasta [queries.fasta] [--band W]
[--min-identity X] [--paf]` prints what `mhap-hip --realign` prints for the same overlaps (with --paf: what `--realign --realign-paf`
prints, one PAF line per overlap with the alignment's path as a cg:Z CIGAR).

Every record's interval is an estimate made from the shared k-mers of two sketches; this tool aligns the two reads inside a band around
the diagonal that interval implies (mhap_realign_records) and prints the record with the alignment's ends and 1 - identity in column 3.
The ids must be the numeric ones MHAP assigns (the 1-based position of a read in reads.fasta; the reads of queries.fasta follow, offset
by --query-id-offset, by default the number of reads in reads.fasta, which is what the driver assigns when every read is long enough
to be sketched).  Named ids (--store-full-id) are not supported.
"""
import argparse
import sys

import numpy as np

from . import api
from .roc import java_split, parse_double, parse_int


def read_overlaps(path):
    """The 12-column MHAP records of a file (ours or Java MHAP's) as a RECORD_DTYPE array; blank lines are skipped."""
    rows = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            sp = java_split(line)
            if sp == [""]:
                continue
            if len(sp) != 12:
                raise api.MhapError(f"{path}:{no}: an MHAP overlap has 12 columns, this line has {len(sp)}")
            try:
                ids = (parse_int(sp[0]), parse_int(sp[1]))
            except ValueError:
                raise api.MhapError(f"{path}:{no}: ids must be numeric; overlaps written with --store-full-id (named ids) are not "
                                    "supported") from None
            try:
                err, raw = parse_double(sp[2]), parse_double(sp[3])
                a_rc, a1, a2, alen, b_rc, b1, b2, blen = (parse_int(x) for x in sp[4:])
            except ValueError as e:
                raise api.MhapError(f"{path}:{no}: {e}") from None
            if a_rc != 0:
                raise api.MhapError(f"{path}:{no}: column 5 (the first read's strand) must be 0")
            rows.append((ids[0], ids[1], 1.0 - err, raw, a1, a2, alen, b1, b2, blen, 1 if b_rc else 0, 0))
    return np.array(rows, dtype=api.RECORD_DTYPE) if rows else np.zeros(0, api.RECORD_DTYPE)


def kept_rows(records, min_identity=0.0):
    """The driver's rule: a record without an alignment, or with an identity below min_identity, is dropped.  The rows that stay."""
    none = (records["score"] == 0.0) & (records["a1"] == 0) & (records["a2"] == 0) & (records["b1"] == 0) & (records["b2"] == 0)
    return np.nonzero(~none & ~(records["score"] < min_identity))[0]


def keep(records, min_identity=0.0):
    """The records that kept_rows keeps."""
    return records[kept_rows(records, min_identity)]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.realign", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("queries", nargs="?")
    ap.add_argument("--band", type=int, default=0, help="half-width of the band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0)
    ap.add_argument("--query-id-offset", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--paf", action="store_true", help="print PAF lines with the alignment's path (cg:Z) instead of the 12 columns")
    a = ap.parse_args(argv)
    if a.band < 0:
        ap.error("--band must be >= 0")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    queries = api.FastaData.from_file(a.queries, len(fasta) if a.query_id_offset is None else a.query_id_offset) if a.queries else None
    if a.paf:
        out, detail, op_offsets, ops = api.realign_records_paths(recs, fasta, band=a.band, max_shift=a.max_shift, device=a.device,
                                                                 query_fasta=queries)
        kept = keep(out, a.min_identity)
        sys.stdout.write("".join(api.format_paf(out[q], detail[q], ops[op_offsets[q]:op_offsets[q + 1]]) + "\n"
                                 for q in kept_rows(out, a.min_identity).tolist()))
    else:
        out, _ = api.realign_records(recs, fasta, band=a.band, max_shift=a.max_shift, device=a.device, query_fasta=queries)
        kept = keep(out, a.min_identity)
        sys.stdout.write("".join(line + "\n" for line in api.records_to_lines(kept)))
    print(f"Realigned {len(recs)} overlaps: {len(kept)} kept, {len(recs) - len(kept)} dropped (no alignment or identity below "
          f"{a.min_identity:g})", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
