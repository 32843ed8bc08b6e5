"""FASTQ text for sequences with base qualities ("base qualities" of include/mhap_hip.h): the one formatter that
`python -m mhap_amd.correct --fastq` and `python -m mhap_amd.graph --consensus-fastq` share.  Writing only: FASTQ is not read."""
import numpy as np

PHRED_OFFSET = 33
PHRED_MAX = 93   # '~'


def quality_string(quals):
    """The Phred+33 string of quality values 0 .. 93."""
    q = np.asarray(quals, dtype=np.int64)
    if len(q) and (int(q.min()) < 0 or int(q.max()) > PHRED_MAX):
        raise ValueError(f"a quality outside 0 .. {PHRED_MAX}")
    return (q + PHRED_OFFSET).astype(np.uint8).tobytes().decode("ascii")


def format_record(header, seq, quals):
    """`@header`, the sequence, `+`, the qualities: four lines; header is what follows `>` on the FASTA line."""
    if len(seq) != len(quals):
        raise ValueError(f"{len(seq)} bases and {len(quals)} qualities")
    return f"@{header}\n{bytes(seq).decode('latin-1')}\n+\n{quality_string(quals)}\n"


def format_fastq(headers, seqs, quals):
    """The FASTQ text of several sequences."""
    return "".join(format_record(h, s, q) for h, s, q in zip(headers, seqs, quals))


def add_arguments(ap):
    """--quality-per-vote and --quality-cap, which both tools take next to their FASTQ flag."""
    ap.add_argument("--quality-per-vote", type=int, default=None, metavar="N", help="tenths of a Phred unit per net vote, 1 .. 1000 (15)")
    ap.add_argument("--quality-cap", type=int, default=None, metavar="N", help="the highest quality written, 1 .. 93 (60)")


def parameters(a, owner_given, owner):
    """(dict(per_vote, cap), None) from the parsed arguments, or (None, the error message)."""
    if (a.quality_per_vote is not None or a.quality_cap is not None) and not owner_given:
        return None, f"--quality-per-vote and --quality-cap need {owner}"
    per_vote = 15 if a.quality_per_vote is None else a.quality_per_vote
    cap = 60 if a.quality_cap is None else a.quality_cap
    if not 1 <= per_vote <= 1000:
        return None, "--quality-per-vote must be 1 .. 1000"
    if not 1 <= cap <= PHRED_MAX:
        return None, "--quality-cap must be 1 .. 93"
    return dict(per_vote=per_vote, cap=cap), None


def add_weight_arguments(ap):
    """--weigh-qualities, --weight-q-lo and --weight-q-hi, which both tools take for their votes ("quality-weighted votes" of
    include/mhap_hip.h)."""
    ap.add_argument("--weigh-qualities", action="store_true", help="every vote weighs the base quality of the FASTQ read it comes from")
    ap.add_argument("--weight-q-lo", type=int, default=None, metavar="Q", help="with --weigh-qualities, a base below this Phred value votes with weight 1 (7)")
    ap.add_argument("--weight-q-hi", type=int, default=None, metavar="Q", help="with --weigh-qualities, a base from this Phred value on votes with weight 3 (20)")


def weight_parameters(a, stage_given, stage):
    """((q_lo, q_hi) or None without --weigh-qualities, None) from the parsed arguments, or (None, the error message).  A threshold
    that was not given is None: the library's default."""
    if (a.weight_q_lo is not None or a.weight_q_hi is not None) and not a.weigh_qualities:
        return None, "--weight-q-lo and --weight-q-hi need --weigh-qualities"
    if not a.weigh_qualities:
        return None, None
    if not stage_given:
        return None, f"--weigh-qualities needs {stage}"
    lo, hi = 7 if a.weight_q_lo is None else a.weight_q_lo, 20 if a.weight_q_hi is None else a.weight_q_hi
    if not 0 <= lo <= hi <= PHRED_MAX:
        return None, "--weight-q-lo and --weight-q-hi must be 0 <= --weight-q-lo <= --weight-q-hi <= 93"
    return (lo, hi), None
