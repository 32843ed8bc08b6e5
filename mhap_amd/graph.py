"""The string graph of a file of MHAP overlaps, on the GPU: `python -m mhap_amd.graph overlaps.txt reads.fasta [--band W]
[--min-identity X] [--max-hang N] [--int-frac F] [--min-overlap N] [--fuzz N] -o out.gfa [--unitigs utg.gfa] [--clean [--tip-reads N]
[--bubble-bases N] [--clean-rounds N]] [--consensus [--consensus-fasta F] [--consensus-fastq F [--quality-per-vote N] [--quality-cap N]]
[--consensus-min-cov N]] [--repeat-filter ...] [--variant-filter ...]` writes what `mhap-hip --realign
--gfa out.gfa [--gfa-unitigs utg.gfa] [--gfa-clean ...]` writes for the same overlaps.

The overlaps are parsed and realigned as `python -m mhap_amd.realign` does; the records that tool would drop (no alignment, or an
identity below --min-identity) take no part.  Every other record is classed (internal match, containment, too short, dovetail), reads
that some record contains are set aside, the dovetails become the arcs of a bidirected graph and the arcs that a two-arc path
explains are reduced (api.GraphSession; the contract is the "string graph" section of include/mhap_hip.h).  Output is GFA 1: an S line
per read that is not contained, without its sequence, and an L line per final arc; the ids are numeric, as the records print them.
With --unitigs the final arcs are compacted into unitigs on the GPU as well and a second GFA 1 file is written: an S line with
the sequence per unitig, an `a` line per read of it, an L line per arc between unitigs ("unitigs" in the same section).
With --clean the graph is cleaned on the GPU before either file is written: tips of at most --tip-reads reads are clipped and simple
bubbles whose lesser branch has at most --bubble-bases bases are popped, in at most --clean-rounds rounds ("graph cleaning" in the same
section); the -o file is then the cleaned read graph and the --unitigs file the cleaned unitig graph.
With --consensus (which needs --unitigs) every read is placed on a unitig, aligned to it and votes, and the --unitigs file carries the
consensus sequences, their lengths and `a` offsets mapped into them ("unitig consensus" in the same header); --consensus-fasta also
writes them as FASTA, and --consensus-fastq as FASTQ with one quality per base from the votes that decided it ("base qualities" in
the same header; Phred+33), with one more stderr line that counts them.  With --weigh-qualities [--weight-q-lo Q] [--weight-q-hi Q], on
FASTQ reads, every vote of the consensus weighs the base quality of the read it comes from ("quality-weighted votes" in the same
header; with --trim the trimmed reads' qualities are the matching slices), and one more stderr line counts the bases per weight class.
With --trim [--trim-min-cov N] [--trim-end-clip N] [--trim-min-span N] [--trim-penalty N] the reads are trimmed and chimeras split on the GPU first
("read trimming" in the same header; `python -m mhap_amd.trim` writes the trimmed reads themselves): every output is then built on
the surviving reads, their trimmed lengths and the overlaps rewritten onto them.
With --repeat-filter [--repeat-factor PCT] [--repeat-max-cov N] [--repeat-min-run N] [--repeat-min-unique N] repeats are marked from the
overlap pile-up first ("repeat marking" in the same header; `python -m mhap_amd.repeats` writes the intervals) and the overlaps that
lie in nothing but repeat reach neither the trimming nor the graph; a two-copy repeat at ordinary depth is not reliably found.
With --variant-filter [--variant-min-depth N] [--variant-min-minor N] [--variant-min-pct PCT] [--variant-max-del-pct PCT]
[--variant-min-diff N] [--variant-diff-pct PCT] variant sites are marked from the pile-up votes in front of all of that ("variant sites"
in the same header; `python -m mhap_amd.variants` writes the sites) and the overlaps whose reads disagree across them reach neither
the repeat marking nor the trimming nor the graph.
Not done: bubbles that are not simple, a second trimming round.  One line on stderr gives the counts (one more with --variant-filter,
one more with --repeat-filter and one more with --trim, in front; one more with --clean, one more with --unitigs, one more with --consensus).
"""
import argparse
import sys

from . import api, fastq, repeats, variants
from .realign import kept_rows, read_overlaps

BATCH = 1 << 16   # records realigned and classed per call


def counts_line(c):
    """The one stderr line of a graph (the driver prints the same)."""
    return (f"String graph of {c['records']} overlaps: {c['none']} none, {c['internal']} internal, {c['a_contained']} contained (from), "
            f"{c['b_contained']} contained (to), {c['short']} short, {c['dovetail']} dovetail; {c['contained_reads']} contained reads, "
            f"{c['arcs']} arcs, {c['reduced']} reduced, {c['final']} final")


def consensus_names(circular):
    """`utg%06d{l|c}` per unitig, as the GFA names them."""
    return [f"utg{k + 1:06d}{'c' if c else 'l'}" for k, c in enumerate(circular)]


def consensus_fasta(seqs, circular):
    """The FASTA text of consensus sequences: `>utg%06d{l|c}` as the GFA names them, one line per sequence."""
    return "".join(f">{name}\n{s.decode('latin-1')}\n" for name, s in zip(consensus_names(circular), seqs))


def graph_overlaps(recs, fasta, band=0, max_shift=0.2, min_identity=0.0, device=0, batch=BATCH, unitigs=False, clean=None, consensus=None,
                   trim=None, repeat=None, quality=None, weights=None, variant=None, **params):
    """Realign `recs` in batches and build the graph: (gfa text, arcs, counts, contained); with unitigs=True two more: the GFA text
    of the unitig graph and the dict of GraphSession.unitigs().  clean: None, or a dict of GraphSession.clean's parameters: the graph
    is cleaned first, both texts and the dict are those of the cleaned graph, and the dict of CLEAN_COUNTS comes last.
    consensus: None, or a dict of ConsensusSession's parameters (min_cov, band), with unitigs=True: the unitig text carries the consensus,
    and the result is a dict instead: gfa, arcs, counts, contained, unitig_gfa, unitigs, clean_counts (or None), consensus_counts,
    consensus_seqs.  quality: None, or with consensus a dict of per_vote and cap: the result dict then has consensus_quals (a uint8
    array per unitig) and quality_hist of ConsensusSession.quality.
    trim: None, or a dict of TrimSession's parameters (min_cov, end_clip, min_span): the reads are trimmed first ("read trimming" in
    the same header) and everything above is built on the surviving reads, their trimmed lengths and the records rewritten onto
    them; the dict of TRIM_COUNTS then comes last of all (key trim_counts of the dict).
    repeat: None, or a dict of RepeatSession's parameters and `penalty`: every kept record is judged on its refined copy ("repeat
    marking" in the same header) and the void ones reach neither the trimming nor the graph; without trim the graph takes the
    survivors as realigned.  The dict of REPEAT_COUNTS then comes behind the trimming's (key repeat_counts of the dict).
    variant: None, or a dict of VariantSession's parameters: the records are judged across the variant sites first ("variant sites"
    in the same header) and everything above is built from the ones that stay; the dict then carries `counts` (VARIANT_COUNTS),
    `set_aside` and `judged`, which graph_overlaps fills in.
    weights: None, or with consensus (q_lo, q_hi): the consensus votes weigh the reads' own qualities (FASTQ reads; with trim, the
    trimmed reads' are the matching slices), "quality-weighted votes" in the same header."""
    with api.MinHashSearch(api.MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device)) as ms:
        tcounts = ()
        if variant is not None:   # the survivors, as they were found: realigned again below, they give the same alignments
            v = variants.variant_overlaps(recs, fasta, band=band, max_shift=max_shift, min_identity=min_identity, batch=batch, handle=ms,
                                          **{k: variant[k] for k in api.VARIANT_DEFAULTS if k in variant})
            recs = recs[v["found_rows"][v["keep"] != 0]]
            variant.update(counts=v["counts"], set_aside=int((v["keep"] == 0).sum()), judged=len(v["keep"]))
        if repeat is not None:
            repeat = dict(repeat)
            rpenalty = repeat.pop("penalty", api.TRIM_PENALTY)
        if trim is not None:   # every record is realigned and held, the reads are cut, and the graph sees the rewritten records only
            from .trim import trim_overlaps
            t = trim_overlaps(recs, fasta, band=band, max_shift=max_shift, min_identity=min_identity, batch=batch, handle=ms, repeat=repeat, **trim)
            fasta, tcounts = t["reads"], (t["counts"],) + (() if repeat is None else (t["repeat"]["counts"],))
            batches = (t["applied"][q0:q0 + batch] for q0 in range(0, len(t["applied"]), batch))
        elif repeat is not None:
            from .repeats import repeat_overlaps
            t = repeat_overlaps(recs, fasta, band=band, max_shift=max_shift, min_identity=min_identity, batch=batch, handle=ms, penalty=rpenalty, **repeat)
            survivors, tcounts = t["realigned"][t["keep"] != 0], (t["counts"],)
            batches = (survivors[q0:q0 + batch] for q0 in range(0, len(survivors), batch))
        else:
            batches = (api.realign_records(recs[q0:q0 + batch], fasta, band=band, handle=ms)[0] for q0 in range(0, len(recs), batch))
        with api.GraphSession(fasta.ids, fasta.lengths, handle=ms, **params) as gs:
            kept = []
            for out in batches:
                if trim is None and repeat is None:
                    out = out[kept_rows(out, min_identity)]
                gs.add(out)
                if consensus is not None:
                    kept.append(out)       # held until the graph is finished, then fed to the consensus
            arcs, counts = gs.finish()
            tail = () if clean is None else (gs.clean(**clean),)
            text = gs.gfa(cleaned=clean is not None)
            if consensus is not None:
                if not unitigs:
                    raise api.MhapError("graph_overlaps: consensus needs unitigs=True")
                if clean is None:
                    gs.unitigs()
                wkw = {} if weights is None else dict(qualities=api.all_qualities(fasta), weights=api.WeightParams(*weights))
                with api.ConsensusSession(gs, fasta, **consensus, **wkw) as cs:
                    for out in kept:
                        cs.add(out)
                    ccounts = cs.run()
                    quals, qhist = cs.quality(**quality) if quality is not None else (None, None)
                    return dict(consensus_quals=quals, quality_hist=qhist, gfa=text, arcs=arcs, counts=counts, contained=gs.contained(), unitig_gfa=cs.gfa(), unitigs=gs.unitigs_table,
                                clean_counts=tail[0] if tail else None, consensus_counts=ccounts, consensus_seqs=cs.sequences(),
                                trim_counts=tcounts[0] if trim is not None else None, repeat_counts=tcounts[-1] if repeat is not None else None)
            if unitigs:
                utext = gs.unitig_gfa(fasta)
                return (text, arcs, counts, gs.contained(), utext, gs.unitigs_table) + tail + tcounts
            return (text, arcs, counts, gs.contained()) + tail + tcounts


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
    ap.add_argument("--clean", action="store_true", help="clip tips and pop simple bubbles on the GPU before the files are written")
    ap.add_argument("--tip-reads", type=int, default=4, help="with --clean, the most reads a tip may have")
    ap.add_argument("--bubble-bases", type=int, default=50000, help="with --clean, the most bases a popped branch may have")
    ap.add_argument("--clean-rounds", type=int, default=16, help="with --clean, the most rounds")
    ap.add_argument("--consensus", action="store_true", help="with --unitigs, write the consensus of every unitig's reads instead of its raw spelling")
    ap.add_argument("--consensus-fasta", default=None, help="with --consensus, also write the consensus sequences to this FASTA file")
    ap.add_argument("--consensus-min-cov", type=int, default=4, help="with --consensus, the depth below which a position keeps the draft's base")
    ap.add_argument("--trim", action="store_true", help="trim the reads and split chimeras on the GPU first; every output is built on the trimmed reads")
    ap.add_argument("--trim-min-cov", type=int, default=3, help="with --trim, the shrunk overlaps a position needs to be kept")
    ap.add_argument("--trim-end-clip", type=int, default=500, help="with --trim, the bases every aligned interval is shrunk by at both ends")
    ap.add_argument("--trim-min-span", type=int, default=2000, help="with --trim, the shortest aligned interval that counts")
    ap.add_argument("--trim-penalty", type=int, default=api.TRIM_PENALTY, help="with --trim, the cost of an error column when overlaps are cut to their best stretch; 0: not cut")
    ap.add_argument("--repeat-filter", action="store_true", help="mark repeats from the overlap pile-up first and drop the overlaps that lie in nothing but repeat")
    ap.add_argument("--consensus-fastq", default=None, help="with --consensus, also write the consensus sequences with base qualities to this FASTQ file")
    fastq.add_arguments(ap)
    fastq.add_weight_arguments(ap)
    repeats.add_arguments(ap, "repeat-")
    ap.add_argument("--variant-filter", action="store_true", help="mark variant sites from the pile-up votes first and drop the overlaps whose reads disagree across them")
    variants.add_arguments(ap, "variant-")
    a = ap.parse_args(argv)
    quality, message = fastq.parameters(a, a.consensus_fastq is not None, "--consensus-fastq")
    if message:
        ap.error(message)
    if a.weigh_qualities and not a.consensus:
        print("--weigh-qualities weighs the votes of --consensus: give --consensus too.")
        return 1
    weights, message = fastq.weight_parameters(a, True, "--consensus")
    if message:
        ap.error(message)
    rp, message = repeats.parameters(a, "repeat-")
    if message:
        ap.error(message)
    if rp != {k: v for k, v in api.REPEAT_DEFAULTS.items() if k in rp} and not a.repeat_filter:
        ap.error("--repeat-factor, --repeat-max-cov, --repeat-min-run and --repeat-min-unique need --repeat-filter")
    vp, message = variants.parameters(a, "variant-")
    if message:
        ap.error(message)
    if vp != api.VARIANT_DEFAULTS and not a.variant_filter:
        ap.error("--variant-min-depth, --variant-min-minor, --variant-min-pct, --variant-max-del-pct, --variant-min-diff and --variant-diff-pct need --variant-filter")
    vp = dict(vp) if a.variant_filter else None
    if (a.trim_min_cov != 3 or a.trim_end_clip != 500 or a.trim_min_span != 2000) and not a.trim:
        ap.error("--trim-min-cov, --trim-end-clip and --trim-min-span need --trim")
    if a.trim_penalty != api.TRIM_PENALTY and not (a.trim or a.repeat_filter):
        ap.error("--trim-penalty needs --trim or --repeat-filter")
    if a.trim_min_cov < 1 or a.trim_end_clip < 0 or a.trim_min_span < 0 or a.trim_penalty < 0:
        ap.error("--trim-min-cov must be >= 1, --trim-end-clip, --trim-min-span and --trim-penalty >= 0")
    if a.consensus and not a.unitigs:
        ap.error("--consensus needs --unitigs")
    if (a.consensus_fasta or a.consensus_fastq or a.consensus_min_cov != 4) and not a.consensus:
        ap.error("--consensus-fasta, --consensus-fastq and --consensus-min-cov need --consensus")
    if a.consensus_min_cov < 1:
        ap.error("--consensus-min-cov must be >= 1")
    if a.tip_reads < 0 or a.bubble_bases < 0 or a.clean_rounds < 1:
        ap.error("--tip-reads and --bubble-bases must be >= 0 and --clean-rounds >= 1")
    if a.band < 0:
        ap.error("--band must be >= 0")
    if a.max_hang < 0 or a.min_overlap < 0 or a.fuzz < 0 or not 0.0 <= a.int_frac <= 1.0:
        ap.error("--max-hang, --min-overlap and --fuzz must be >= 0 and --int-frac in [0, 1]")
    recs = read_overlaps(a.overlaps)
    fasta = api.FastaData.from_file(a.reads)
    if weights is not None:
        if fasta.qualities is None:
            print(f"--weigh-qualities needs the base qualities of FASTQ reads: {a.reads} is FASTA.")
            return 1
        print(api.weight_classes_line(fasta.bases, fasta.qualities, api.WeightParams(*weights)), file=sys.stderr)
    res = graph_overlaps(recs, fasta, band=a.band, max_shift=a.max_shift, min_identity=a.min_identity, device=a.device, unitigs=bool(a.unitigs),
                         clean=dict(tip_reads=a.tip_reads, bubble_bases=a.bubble_bases, max_rounds=a.clean_rounds) if a.clean else None,
                         consensus=dict(min_cov=a.consensus_min_cov) if a.consensus else None,
                         trim=dict(min_cov=a.trim_min_cov, end_clip=a.trim_end_clip, min_span=a.trim_min_span, penalty=a.trim_penalty) if a.trim else None,
                         repeat=dict(rp, penalty=a.trim_penalty) if a.repeat_filter else None,
                         quality=quality if a.consensus_fastq else None, weights=weights, variant=vp,
                         max_hang=a.max_hang, int_frac_permille=int(round(a.int_frac * 1000)), min_ovlp=a.min_overlap, fuzz=a.fuzz)
    tcounts = rcounts = None
    if a.repeat_filter:
        rcounts = res["repeat_counts"] if a.consensus else res[-1]
        res = res if a.consensus else res[:-1]
    if a.trim:
        tcounts = res["trim_counts"] if a.consensus else res[-1]
        res = res if a.consensus else res[:-1]
    if a.consensus:
        quals, qhist = res["consensus_quals"], res["quality_hist"]
        res = (res["gfa"], res["arcs"], res["counts"], res["contained"], res["unitig_gfa"], res["unitigs"], res["consensus_counts"],
               res["consensus_seqs"]) + ((res["clean_counts"],) if a.clean else ())
    text, counts = res[0], res[2]
    if a.output:
        with open(a.output, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)
    if a.variant_filter:
        print(api.variant_counts_line([vp["counts"][k] for k in api.VARIANT_COUNTS], vp["set_aside"], vp["judged"]), file=sys.stderr)
    if a.repeat_filter:
        print(api.repeat_counts_line([rcounts[k] for k in api.REPEAT_COUNTS]), file=sys.stderr)
    if a.trim:
        print(api.trim_counts_line([tcounts[k] for k in api.TRIM_COUNTS]), file=sys.stderr)
    print(counts_line(counts), file=sys.stderr)
    if a.clean:
        print(api.clean_counts_line([res[-1][k] for k in api.CLEAN_COUNTS]), file=sys.stderr)
    if a.unitigs:
        with open(a.unitigs, "w") as fh:
            fh.write(res[4])
        print(api.unitig_counts_line([res[5]["counts"][k] for k in api.UNITIG_COUNTS]), file=sys.stderr)
    if a.consensus:
        print(api.consensus_counts_line([res[6][k] for k in api.CONSENSUS_COUNTS]), file=sys.stderr)
        if a.consensus_fasta:
            with open(a.consensus_fasta, "w") as fh:
                fh.write(consensus_fasta(res[7], res[5]["circular"].tolist()))
        if a.consensus_fastq:
            with open(a.consensus_fastq, "w") as fh:
                fh.write(fastq.format_fastq(consensus_names(res[5]["circular"].tolist()), res[7], quals))
            print(api.quality_counts_line(qhist), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
