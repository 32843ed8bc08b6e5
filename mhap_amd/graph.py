"""The string graph of a file of MHAP overlaps, on the GPU: `python -m mhap_amd.graph overlaps.txt reads.fasta [--band W]
[--min-identity X] [--max-hang N] [--int-frac F] [--min-overlap N] [--fuzz N] -o out.gfa [--unitigs utg.gfa]` writes what
`mhap-hip --realign --gfa out.gfa [--gfa-unitigs utg.gfa]` writes for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does; the records that tool would drop (no alignment, or an
identity below --min-identity) take no part.  Every other record is classed (internal match, containment, too short, dovetail), reads
that some record contains are set aside, the dovetails become the arcs of a bidirected graph and the arcs that a two-arc path
explains are reduced (api.GraphSession; the contract is the "string graph" section of include/mhap_hip.h).  Output is GFA 1: an S line
per read that is not contained, without its sequence, and an L line per final arc; the ids are numeric, as the records print them.
With --unitigs the final arcs are compacted into unitigs on the GPU as well and a second GFA 1 file is written: an S line with
the sequence per unitig, an `a` line per read of it, an L line per arc between unitigs ("unitigs" in the same section).
Not done: read trimming, chimera detection, tip and bubble removal.  One line on stderr gives the counts (two with --unitigs).
"""
import argparse
import sys

from . import api
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned and classed per call


def counts_line(c):
    """The one stderr line of a graph (the driver prints the same)."""
    return (f"String graph of {c['records']} overlaps: {c['none']} none, {c['internal']} internal, {c['a_contained']} contained (from), "
            f"{c['b_contained']} contained (to), {c['short']} short, {c['dovetail']} dovetail; {c['contained_reads']} contained reads, "
            f"{c['arcs']} arcs, {c['reduced']} reduced, {c['final']} final")


def graph_overlaps(recs, fasta, band=0, max_shift=0.2, min_identity=0.0, device=0, batch=BATCH, unitigs=False, **params):
    """Realign `recs` in batches and build the graph: (gfa text, arcs, counts, contained); with unitigs=True two more: the GFA text
    of the unitig graph and the dict of GraphSession.unitigs()."""
    with api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device)) as ms:
        with api.GraphSession(fasta.ids, fasta.lengths, handle=ms, **params) as gs:
            for q0 in range(0, len(recs), batch):
                out, _ = api.realign_records(recs[q0:q0 + batch], fasta, band=band, handle=ms)
                gs.add(out[kept_rows(out, min_identity)])
            arcs, counts = gs.finish()
            if unitigs:
                utext = gs.unitig_gfa(fasta)
                return gs.gfa(), arcs, counts, gs.contained(), utext, gs.unitigs_table
            return gs.gfa(), arcs, counts, gs.contained()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mhap_amd.graph", description=__doc__.split("\n\n")[0])
    ap.add_argument("overlaps")
    ap.add_argument("reads")
    ap.add_argument("--band", type=int, default=0, help="half-width of the realignment band in bases; 0: the overlap's length times --max-shift")
    ap.add_argument("--max-shift", type=float, default=0.2)
    ap.add_argument("--min-identity", type=float, default=0.0, help="overlaps realigned below this identity take no part")
    ap.add_argument("--max-hang", type=int, default=1000, help="the longest unaligned end on both reads before an overlap is an internal match")
    ap.add_argument("--int-frac", type=float, default=0.8, help="the aligned share of an overlap and its hangs below which it is an internal match")
    ap.add_argument("--min-overlap", type=int, default=2000, help="the shortest overlap that becomes an arc")
    ap.add_argument("--fuzz", type=int, default=1000, help="the slack of the transitive reduction in bases")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default=None, help="the GFA file to write (default: stdout)")
    ap.add_argument("--unitigs", default=None, help="also compact the final arcs into unitigs and write their GFA, with sequences, to this file")
    a = ap.parse_args(argv)
    if a.band < 0:
        ap.error("--band must be >= 0")
    if a.max_hang < 0 or a.min_overlap < 0 or a.fuzz < 0 or not 0.0 <= a.int_frac <= 1.0:
        ap.error("--max-hang, --min-overlap and --fuzz must be >= 0 and --int-frac in [0, 1]")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    res = graph_overlaps(recs, fasta, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity, device=a.device, unitigs=bool(a.unitigs),
                         max_hang=a.max_hang, int_frac_permille=int(round(a.int_frac * 1000)), min_ovlp=a.min_overlap, fuzz=a.fuzz)
    text, counts = res[0], res[2]
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    print(counts_line(counts), file=sys.stderr)
    if a.unitigs:
        with open(a.unitigs, "w") as fh:
            fh.write(res[4])
        print(api.unitig_counts_line([res[5]["counts"][k] for k in api.UNITIG_COUNTS]), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
