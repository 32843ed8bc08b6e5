"""Correct reads on the GPU from a file of MHAP overlaps: `python -m mhap_amd.correct overlaps.txt reads.fasta [queries.fasta] [--band W]
[--min-identity X] [--min-coverage N] [--best-overlaps N [--best-min-span S]] [-o out.fasta] [--fastq out.fastq [--quality-per-vote N]
[--quality-cap N]] [--weigh-qualities [--weight-q-lo Q] [--weight-q-hi Q]]` writes what `mhap-hip --realign --correct out.fasta` (with the same --best-overlaps flags, and --correct-fastq)
writes for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does, with every alignment's path; the records that tool would
drop (no alignment, or an identity below --min-identity) cast no vote.  Every other record votes column by column on both of its reads
(api.CorrectSession; the contract is the "read correction" section of include/mhap_hip.h) and each read position takes the majority.
Output is FASTA, one unwrapped line per read: `>ID len=<corrected length> sub=<substitutions> del=<deletions> ins=<insertions>
low=<positions below --min-coverage>`, the ids numeric as the records print them; one line on stderr gives the totals.
--fastq also writes the corrected reads as FASTQ, the same header fields behind `@`, with one quality per base from the votes that
decided it ("base qualities" of include/mhap_hip.h; Phred+33), and one more stderr line counts them.

--weigh-qualities, on FASTQ reads, lets every vote weigh the base quality of the read it comes from ("quality-weighted votes" of
include/mhap_hip.h; `mhap-hip --weigh-qualities`), and one more stderr line counts the reads' bases per weight class.

--best-overlaps N makes two passes ("overlap selection" of include/mhap_hip.h): the first realigns without paths and selects each
read's N best views over the records that would vote (api.SelectSession), the second realigns only the records that keep a view, with
paths, and votes the selected views.
"""
import argparse
import sys

import numpy as np

from . import api, fastq
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned and voted per call


def select_paths(op_offsets, ops, rows):
    """(op_offsets, ops) of the pairs `rows` of a paths result, in that order."""
    rows = np.asarray(rows, dtype=np.int64)
    lens = (op_offsets[rows + 1] - op_offsets[rows]) if len(rows) else np.zeros(0, np.int64)
    out = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=out[1:])
    parts = [ops[op_offsets[q]:op_offsets[q + 1]] for q in rows.tolist()]
    return out, (np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32))


def header_fields(names, stats):
    """What follows `>` (FASTA) or `@` (FASTQ) per read: `NAME len= sub= del= ins= low=`."""
    return [f"{name} len={st[1]} sub={st[2]} del={st[3]} ins={st[4]} low={st[5]}" for name, st in zip(names, np.asarray(stats).tolist())]


def format_fasta(names, seqs, stats):
    """The corrected reads as FASTA text: `>NAME len= sub= del= ins= low=` and the bases on one line, per read."""
    return "".join(f">{h}\n{bytes(seq).decode('latin-1')}\n" for h, seq in zip(header_fields(names, stats), seqs))


def totals_line(stats, skipped_views):
    """The one stderr line of a correction (the driver prints the same)."""
    t = np.asarray(stats, dtype=np.int64).reshape(-1, 6).sum(axis=0).tolist()
    return (f"Corrected {len(stats)} reads: {t[0]} bases in, {t[1]} out; {t[2]} substitutions, {t[3]} deletions, {t[4]} insertions, "
            f"{t[5]} positions of low coverage; skipped_views = {skipped_views}")


def select_pass(recs, fasta, queries, ms, band, min_identity, best_n, best_min_span, batch):
    """The first pass of --best-overlaps: (the rows of `recs` that keep a view, their view bytes, SelectSession.finish's rows and
    counts, the ids of the rows)."""
    _, ids, _, lengths = api._all_reads(fasta, queries)
    with api.SelectSession(ids, lengths, best_n=best_n, min_span=best_min_span, handle=ms) as ss:
        held = []   # per batch: the rows of recs that would vote, and their realigned records
        for q0 in range(0, len(recs), batch):
            out, _ = api.realign_records(recs[q0:q0 + batch], fasta, band=band, handle=ms, query_fasta=queries)
            rows = kept_rows(out, min_identity)
            ss.add(out[rows])
            held.append((q0 + rows, out[rows]))
        table, counts = ss.finish()
        which, views = [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)]
        for rows, out in held:
            v = ss.apply(out)
            which.append(rows[v != 0])
            views.append(v[v != 0])
    return np.concatenate(which), np.concatenate(views), table, counts, np.asarray(ids, np.int64)


def correct_overlaps(recs, fasta, queries=None, band=0, max_shift=0.2, min_identity=0.0, min_cov=4, device=0, batch=BATCH, best_n=0,
                     best_min_span=500, selection=None, quality=None, weights=None):
    """Realign `recs` with paths in batches and vote: (seqs, stats, skipped_views, records that voted).  best_n > 0: only each read's
    best_n best views vote; `selection` (a dict) then takes the selection's rows, counts and ids.  quality: None, or a dict of per_vote and
    cap, which then takes `quals` (a uint8 array per read) and `hist` of CorrectSession.quality.  weights: None, or (q_lo, q_hi): the votes
    weigh the reads' own qualities (api.all_qualities: FASTQ reads), "quality-weighted votes" of include/mhap_hip.h."""
    wkw = {} if weights is None else dict(qualities=api.all_qualities(fasta, queries), weights=api.WeightParams(*weights))
    voted = 0
    with api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device)) as ms:
        views = None
        if best_n > 0:
            which, views, table, counts, sel_ids = select_pass(recs, fasta, queries, ms, band, min_identity, best_n, best_min_span, batch)
            recs = recs[which]
            if selection is not None:
                selection.update(rows=table, counts=counts, ids=sel_ids)
        with api.CorrectSession(fasta, query_fasta=queries, handle=ms, **wkw) as cs:
            for q0 in range(0, len(recs), batch):
                out, _, op_offsets, ops = api.realign_records_paths(recs[q0:q0 + batch], fasta, band=band, handle=ms, query_fasta=queries)
                rows = kept_rows(out, min_identity)
                ko, kops = select_paths(op_offsets, ops, rows)
                cs.add(out[rows], ko, kops, views=None if views is None else views[q0:q0 + batch][rows])
                voted += len(rows)
            seqs, stats, skipped = cs.finish(min_cov)
            if quality is not None:
                quality["quals"], quality["hist"] = cs.quality(quality.get("per_vote", 15), quality.get("cap", 60))
            ids = cs.ids.tolist()
    return ids, seqs, stats, skipped, voted


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.correct", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("queries", nargs="?")
    ap.add_argument("--band", type=int, default=0, help="half-width of the band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0, help="overlaps realigned below this identity cast no vote")
    ap.add_argument("--min-coverage", type=int, default=4, help="votes a position needs before it is changed (min_cov)")
    ap.add_argument("--best-overlaps", type=int, default=0, metavar="N", help="only each read's N best views vote; 0: every view")
    ap.add_argument("--best-min-span", type=int, default=None, metavar="S", help="a view shorter than this is no evidence (500)")
    ap.add_argument("--query-id-offset", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default=None, help="the FASTA file to write (default: stdout)")
    ap.add_argument("--fastq", default=None, help="also write the corrected reads with base qualities to this FASTQ file")
    fastq.add_arguments(ap)
    fastq.add_weight_arguments(ap)
    a = ap.parse_args(argv)
    quality, message = fastq.parameters(a, a.fastq is not None, "--fastq")
    if message:
        ap.error(message)
    weights, message = fastq.weight_parameters(a, True, "a correction")
    if message:
        ap.error(message)
    if a.best_overlaps < 0:
        ap.error("--best-overlaps must be >= 0")
    if a.best_min_span is not None and a.best_overlaps == 0:
        ap.error("--best-min-span needs --best-overlaps")
    if a.best_min_span is not None and a.best_min_span < 0:
        ap.error("--best-min-span must be >= 0")
    if a.band < 0:
        ap.error("--band must be >= 0")
    if a.min_coverage < 1:
        ap.error("--min-coverage must be >= 1")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    queries = api.FastaData.from_file(a.queries, len(fasta) if a.query_id_offset is None else a.query_id_offset) if a.queries else None
    if weights is not None:
        for path, f in ((a.reads, fasta), (a.queries, queries)):
            if f is not None and f.qualities is None:
                print(f"--weigh-qualities needs the base qualities of FASTQ reads: {path} is FASTA.")
                return 1
        bases, _, _, _ = api._all_reads(fasta, queries)
        print(api.weight_classes_line(bases, api.all_qualities(fasta, queries), api.WeightParams(*weights)), file=sys.stderr)
    selection = {}
    ids, seqs, stats, skipped, voted = correct_overlaps(recs, fasta, queries, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity,
                                                        min_cov=a.min_coverage, device=a.device, best_n=a.best_overlaps,
                                                        best_min_span=500 if a.best_min_span is None else a.best_min_span,
                                                        selection=selection, quality=quality if a.fastq else None, weights=weights)
    text = format_fasta(ids, seqs, stats)
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    print(f"Realigned {len(recs)} overlaps: {voted} voted, {len(recs) - voted} dropped (no alignment or identity below {a.min_identity:g})",
          file=sys.stderr)
    if selection:
        print(api.select_counts_line([selection["counts"][k] for k in api.SELECT_COUNTS]), file=sys.stderr)
    print(totals_line(stats, skipped), file=sys.stderr)
    if a.fastq:
        with open(a.fastq, "w") as fh:
            fh.write(fastq.format_fastq(header_fields(ids, stats), seqs, quality["quals"]))
        print(api.quality_counts_line(quality["hist"]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
