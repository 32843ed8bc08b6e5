"""mhap_amd — MI355X-native MinHash overlap engine (the hot path of marbl/MHAP).

The compute lives in libmhaphip.so (hand-written HIP for gfx950 behind the C ABI in
include/mhap_hip.h).  This package is the Python host-side mirror of the reference's operator
interface (MinHashSearch / SequenceSketchStreamer / FastaData / MatchResult) over that C ABI.
There is no CPU fallback: without the built extension and a HIP device the compute calls raise.
"""
from .api import (  # noqa: F401
    MhapError,
    MhapParams,
    MinHashSearch,
    MinHashSearchGroup,
    FastaData,
    FastaScan,
    FrequencyCounts,
    KmerCounts,
    count_kmers,
    KmerSet,
    KmerEval,
    kmer_histogram_valley,
    MatchResult,
    format_record,
    synth_reads,
    synth_reads_from_genome,
    synth_truth,
    align_pairs,
    align_pairs_banded,
    realign_plan,
    realign_records,
    align_pairs_banded_paths,
    realign_records_paths,
    cigar_string,
    format_paf,
    CorrectSession,
    correct_reads,
    WeightParams,
    all_qualities,
    weight_classes_line,
    GraphSession,
    string_graph,
    format_gfa,
    format_gfa_link,
    unitigs,
    format_unitig_gfa,
    format_gfa_unitig_link,
    ConsensusSession,
    format_consensus_gfa,
    consensus_counts_line,
    TrimSession,
    trim_counts_line,
    trim_clip_record,
    trim_refine,
    trim_refine_record,
    RepeatSession,
    repeat_counts_line,
    repeat_judge_record,
    VariantSession,
    variant_counts_line,
    SelectSession,
    select_overlaps,
    select_counts_line,
    select_judge_record,
    pair_kmer_stats,
    records_to_lines,
    load_library,
    KERNEL_NAMES,
)


def __getattr__(name):
    # KmerStatSimulator's API, imported on first use so that `python -m mhap_amd.kmer_sim` runs a module not yet imported
    if name in ("simulate_pairs", "simulate_reads"):
        from . import kmer_sim
        return getattr(kmer_sim, name)
    if name in ("hpc", "HpcReads"):   # homopolymer compression, the same way (`python -m mhap_amd.hpc`): hpc.compress, hpc.HpcReads
        import importlib
        hpc = importlib.import_module(".hpc", __name__)
        return hpc if name == "hpc" else hpc.HpcReads
    if name == "assess":   # sequence assessment, the same way (`python -m mhap_amd.kmer_qv`)
        from . import kmer_qv
        return kmer_qv.assess
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
