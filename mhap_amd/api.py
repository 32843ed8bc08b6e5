"""Host-side mirror of MHAP's operator interface over the libmhaphip C ABI (include/mhap_hip.h).

Names follow the reference (J/ = src/main/java/edu/umd/marbl/mhap/):
  MinHashSearch   <- J/impl/MinHashSearch.java + J/impl/AbstractMatchSearch.java (addData/findMatches)
  FastaData       <- J/impl/FastaData.java
  FrequencyCounts <- J/sketch/FrequencyCounts.java (file parsing; the table is applied on the GPU)
  MatchResult     <- J/impl/MatchResult.java (record + text format)
Error behaviour: every failure raises MhapError (the MhapRuntimeException analogue).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("MHAP_LIB_PATH") or os.path.join(_HERE, "lib", "libmhaphip.so")   # MHAP_LIB_PATH: A/B builds of the kernels
_lib = None

KERNEL_NAMES = ["hash_kmers", "kmer_weight", "minhash", "ordered", "candidate", "overlap", "index_build", "index_query"]


class MhapError(RuntimeError):
    """MhapRuntimeException analogue (J/impl/MhapRuntimeException.java:32)."""


class _Params(C.Structure):
    _fields_ = [("kmer_size", C.c_int32), ("num_hashes", C.c_int32), ("ordered_kmer_size", C.c_int32),
                ("ordered_sketch_size", C.c_int32), ("num_min_matches", C.c_int32), ("min_store_length", C.c_int32),
                ("min_olap_length", C.c_int32), ("device", C.c_int32), ("threshold", C.c_double),
                ("max_shift", C.c_double), ("repeat_weight", C.c_double)]


class _Stats(C.Structure):
    _fields_ = [("strands_indexed", C.c_int64), ("queries_searched", C.c_int64), ("candidates_compared", C.c_int64),
                ("matches_found", C.c_int64), ("slot_compares", C.c_int64), ("table_elements", C.c_int64),
                ("slow_pairs", C.c_int64), ("index_splits", C.c_int64)]


class _KTimes(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("launches", C.c_int64 * 8)]


class _Fasta(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("lengths", C.c_void_p), ("ids", C.c_void_p),
                ("n", C.c_int64), ("total_bases", C.c_int64), ("headers", C.c_void_p), ("headers_bytes", C.c_int64)]


RECORD_DTYPE = np.dtype([("from_id", "<i8"), ("to_id", "<i8"), ("score", "<f8"), ("raw", "<f8"), ("a1", "<i4"),
                         ("a2", "<i4"), ("alen", "<i4"), ("b1", "<i4"), ("b2", "<i4"), ("blen", "<i4"),
                         ("to_rc", "<i4"), ("pad", "<i4")])
_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p)
_GATE = C.CFUNCTYPE(C.c_int, C.c_void_p)

# Every symbol include/mhap_hip.h declares, with its prototype as the header has it: "result:parameters", one letter per type.
# Result: v void, i int, q int64_t, s const char*, p another pointer.  Parameters: p a pointer of any kind (a callback too),
# i int or int32_t, I uint32_t, q int64_t, Q uint64_t, z size_t, d double.  load_library declares all of them, so that a bare Python int
# goes down as the 64-bit value the callee reads, and a library without one of the symbols is refused there.
_CTYPES = {"v": None, "i": C.c_int32, "I": C.c_uint32, "q": C.c_int64, "Q": C.c_uint64, "z": C.c_size_t, "d": C.c_double, "p": C.c_void_p,
           "s": C.c_char_p}
_PROTOTYPES = {
    "mhap_create": "i:pppz",
    "mhap_destroy": "v:p",
    "mhap_last_error": "s:p",
    "mhap_default_params": "v:p",
    "mhap_set_filter": "i:pppqdddi",
    "mhap_index_add_reads": "i:pppppq",
    "mhap_sketch_batch": "i:ppppqpppp",
    "mhap_index_add_sketches": "i:ppppppppq",
    "mhap_index_size": "i:pp",
    "mhap_index_export": "i:pqqpppppppp",
    "mhap_index_clear": "i:p",
    "mhap_index_prepare": "i:p",
    "mhap_sketch_reads_device": "i:ppppqppp",
    "mhap_index_set_device": "i:ppppppq",
    "mhap_find_matches_self": "i:pqqpp",
    "mhap_find_matches_reads": "i:pppppqpp",
    "mhap_get_stats": "i:pp",
    "mhap_get_kernel_times": "i:pp",
    "mhap_reset_kernel_times": "i:p",
    "mhap_set_stream": "i:pp",
    "mhap_synchronize": "i:p",
    "mhap_format_record": "i:ppz",
    "mhap_fasta_read": "i:pqppz",
    "mhap_fasta_free": "v:p",
    "mhap_synth_reads": "i:Qqiddp",
    "mhap_hash_kmer": "i:piip",
    "mhap_selftest_hash_windows": "i:piiipp",
    "mhap_selftest_overlap_lane": "i:piipiidip",
    "mhap_stage_reads": "i:pppppq",
    "mhap_index_add_staged": "i:p",
    "mhap_sketch_staged_device": "i:pppp",
    "mhap_find_matches_self_shard": "i:pqqpp",
    "mhap_synth_reads_shard": "i:Qqiddqqp",
    "mhap_selftest_transpose32": "i:p",
    "mhap_selftest_pass_min": "i:iidpp",
    "mhap_selftest_sketch_plan": "i:Qqppqiiippppp",
    "mhap_selftest_ordered_schedule": "i:qqqqip",
    "mhap_selftest_xorshift_jump": "i:Qip",
    "mhap_selftest_xorshift_unjump": "i:Qip",
    "mhap_find_matches_sketches": "i:pppppppqpp",
    "mhap_synth_reads_repeats": "i:Qqiddqqiidp",
    "mhap_synth_reads_genome": "i:Qpqqppdp",
    "mhap_find_matches_device": "i:pppppqipp",
    "mhap_set_filter_whitelist": "i:ppqqi",
    "mhap_set_filter_file": "i:ppddiidipz",
    "mhap_selftest_bloom": "i:pqqpqpp",
    "mhap_set_second_stage_gate": "i:ppp",
    "mhap_dist_unique_id": "i:pz",
    "mhap_dist_init": "i:piip",
    "mhap_dist_finalize": "i:p",
    "mhap_dist_find_matches_self": "i:ppp",
    "mhap_dist_find_matches_reads": "i:pppppqpp",
    "mhap_dist_last_timing": "i:pp",
    "mhap_dist_exchange_timing": "i:pp",
    "mhap_dist_info": "i:pppz",
    "mhap_dist_selftest": "i:pzp",
    "mhap_dist_set_eager": "i:pi",
    "mhap_dist_eager_searches": "q:p",
    "mhap_group_create": "i:ppippz",
    "mhap_group_destroy": "v:p",
    "mhap_group_size": "i:p",
    "mhap_group_rank": "p:pi",
    "mhap_group_last_error": "s:p",
    "mhap_group_add_reads": "i:pppppq",
    "mhap_group_clear": "i:p",
    "mhap_group_find_matches_self": "i:ppp",
    "mhap_group_find_matches_reads": "i:pppppqpp",
    "mhap_group_get_stats": "i:pp",
    "mhap_abi_version": "i:",
    "mhap_abi_sizes": "i:p",
    "mhap_index_reserve": "i:pq",
    "mhap_fasta_scan_open": "i:pqppz",
    "mhap_fasta_scan_free": "v:p",
    "mhap_fasta_scan_reads": "q:p",
    "mhap_fasta_scan_bases": "q:p",
    "mhap_fasta_scan_info": "i:ppppp",
    "mhap_index_add_scan": "i:pp",
    "mhap_find_matches_scan": "i:pppp",
    "mhap_group_add_scan": "i:pp",
    "mhap_kmer_count_begin": "i:pii",
    "mhap_kmer_count_add_reads": "i:ppppq",
    "mhap_kmer_count_add_scan": "i:pp",
    "mhap_kmer_count_finish": "i:pdp",
    "mhap_kmer_counts_info": "i:ppppp",
    "mhap_kmer_counts_lines": "i:ppp",
    "mhap_kmer_counts_write": "i:pp",
    "mhap_kmer_counts_free": "v:p",
    "mhap_selftest_kmer_windows": "i:piiipp",
    "mhap_kmer_count_finish_flags": "i:pdIp",
    "mhap_kmer_counts_histogram_size": "i:pp",
    "mhap_kmer_counts_histogram": "i:ppp",
    "mhap_kmer_counts_write_histogram": "i:pp",
    "mhap_kmer_histogram_valley": "i:ppqp",
    "mhap_kmer_qv": "i:qqipp",
    "mhap_kmer_count_finish_set": "i:pQp",
    "mhap_kmer_set_free": "v:p",
    "mhap_kmer_set_info": "i:ppppppp",
    "mhap_kmer_set_contains": "i:pppqp",
    "mhap_kmer_set_compare": "i:pppppp",
    "mhap_kmer_eval_reads": "i:pppppqp",
    "mhap_kmer_eval_scan": "i:pppp",
    "mhap_kmer_eval_free": "v:p",
    "mhap_kmer_eval_info": "i:ppppp",
    "mhap_kmer_eval_rows": "i:pp",
    "mhap_kmer_eval_intervals": "i:pp",
    "mhap_kmer_eval_write_table": "i:ppp",
    "mhap_kmer_eval_write_bed": "i:ppp",
    "mhap_kmer_eval_summary": "i:pppqpz",
    "mhap_selftest_kmer_eval": "i:piiippp",
    "mhap_histogram_stats": "i:ppqdppp",
    "mhap_synth_truth": "i:Qqidqpdqqpppppp",
    "mhap_align_pairs": "i:ppqpqp",
    "mhap_align_pairs_banded": "i:ppqpqp",
    "mhap_realign_plan": "i:pqpppqdip",
    "mhap_realign_plan_error": "s:",
    "mhap_realign_records": "i:ppqpppqpqipp",
    "mhap_align_pairs_banded_paths": "i:ppqpqpp",
    "mhap_realign_records_paths": "i:ppqpppqpqippp",
    "mhap_align_paths_info": "i:ppp",
    "mhap_align_paths_copy": "i:ppp",
    "mhap_align_paths_free": "v:p",
    "mhap_format_paf": "i:pppqpppz",
    "mhap_align_paths_from_runs": "i:pqpp",
    "mhap_correct_begin": "i:ppqpppqp",
    "mhap_correct_add": "i:ppqp",
    "mhap_correct_finish": "i:pippp",
    "mhap_correct_copy": "i:pp",
    "mhap_correct_votes": "i:pqp",
    "mhap_correct_free": "v:p",
    "mhap_graph_default_params": "v:p",
    "mhap_graph_begin": "i:pppqpp",
    "mhap_graph_add": "i:ppq",
    "mhap_graph_finish": "i:pp",
    "mhap_graph_info": "i:pppp",
    "mhap_graph_copy_arcs": "i:pp",
    "mhap_graph_copy_classes": "i:pp",
    "mhap_graph_copy_read_flags": "i:pp",
    "mhap_graph_free": "v:p",
    "mhap_format_gfa_link": "i:pppz",
    "mhap_graph_unitigs": "i:pp",
    "mhap_graph_unitigs_info": "i:ppppp",
    "mhap_graph_copy_unitigs": "i:pppp",
    "mhap_graph_copy_layout": "i:pppp",
    "mhap_graph_copy_links": "i:pp",
    "mhap_graph_spell": "i:ppqpp",
    "mhap_graph_spell_device": "i:ppqpp",
    "mhap_format_gfa_unitig_link": "i:ppz",
    "mhap_graph_default_clean_params": "v:p",
    "mhap_graph_clean": "i:ppp",
    "mhap_graph_copy_dropped": "i:pp",
    "mhap_graph_copy_removed": "i:pp",
    "mhap_graph_unitigs_counts": "i:pp",
    "mhap_consensus_default_params": "v:p",
    "mhap_consensus_begin": "i:ppqppp",
    "mhap_consensus_add": "i:ppq",
    "mhap_consensus_run": "i:pp",
    "mhap_consensus_info": "i:ppppp",
    "mhap_consensus_copy": "i:pppp",
    "mhap_consensus_copy_placements": "i:pp",
    "mhap_consensus_copy_map": "i:pp",
    "mhap_consensus_votes": "i:pqp",
    "mhap_consensus_times": "i:pp",
    "mhap_consensus_free": "v:p",
    "mhap_trim_default_params": "v:p",
    "mhap_trim_begin": "i:pppqpp",
    "mhap_trim_add": "i:ppq",
    "mhap_trim_finish": "i:pp",
    "mhap_trim_copy": "i:ppp",
    "mhap_trim_coverage": "i:pqp",
    "mhap_trim_apply": "i:ppqpp",
    "mhap_trim_clip_record": "i:ppppp",
    "mhap_trim_free": "v:p",
    "mhap_trim_refine": "i:ppqpip",
    "mhap_trim_refine_record": "i:ppqip",
    "mhap_repeat_default_params": "v:p",
    "mhap_repeat_begin": "i:pppqpp",
    "mhap_repeat_add": "i:ppq",
    "mhap_repeat_finish": "i:pp",
    "mhap_repeat_copy": "i:ppppp",
    "mhap_repeat_histogram": "i:pp",
    "mhap_repeat_apply": "i:ppqpp",
    "mhap_repeat_judge_record": "i:ppqpqpp",
    "mhap_repeat_free": "v:p",
    "mhap_select_default_params": "v:p",
    "mhap_select_begin": "i:pppqpp",
    "mhap_select_add": "i:ppq",
    "mhap_select_finish": "i:pp",
    "mhap_select_copy": "i:pp",
    "mhap_select_apply": "i:ppqp",
    "mhap_select_judge_record": "i:ppp",
    "mhap_select_free": "v:p",
    "mhap_hpc_compress": "i:ppqpppqqp",
    "mhap_hpc_info": "i:pp",
    "mhap_hpc_copy": "i:ppppp",
    "mhap_hpc_expand_records": "i:pppqp",
    "mhap_hpc_expand_record": "i:ppipip",
    "mhap_hpc_times": "i:pp",
    "mhap_hpc_free": "v:p",
    "mhap_correct_add_views": "i:ppqpp",
    "mhap_pair_kmer_stats": "i:ppqpqiipqpp",
    "mhap_pair_kmer_stats_paths": "i:pqiqip",
    "mhap_ksim_create": "p:qiiddddipppq",
    "mhap_ksim_next": "q:pqpp",
    "mhap_ksim_error": "s:pp",
    "mhap_ksim_destroy": "v:p",
    "mhap_ksim_dev_create": "p:p",
    "mhap_ksim_dev_destroy": "v:p",
    "mhap_ksim_dev_pair_stats": "i:ppqpqiipqpp",
    "mhap_ksim_dev_trials": "i:pQqqiiddddipppqiipqppppp",
    "mhap_quality_default_params": "v:p",
    "mhap_correct_quality": "i:pppp",
    "mhap_consensus_quality": "i:pppp",
    "mhap_fasta_read_qualities": "i:pqpppz",
    "mhap_qualities_free": "v:p",
    "mhap_fasta_scan_has_qualities": "i:p",
    "mhap_fasta_scan_qualities": "i:pp",
    "mhap_weight_default_params": "v:p",
    "mhap_correct_begin_weighted": "i:pppqpppqpp",
    "mhap_consensus_begin_weighted": "i:pppqpppp",
    "mhap_variant_default_params": "v:p",
    "mhap_variant_begin": "i:ppqpppqpp",
    "mhap_variant_add": "i:ppqp",
    "mhap_variant_votes": "i:pqp",
    "mhap_variant_finish": "i:pp",
    "mhap_variant_copy": "i:pppp",
    "mhap_variant_apply": "i:ppqppp",
    "mhap_variant_free": "v:p",
}
EXPORTED_SYMBOLS = list(_PROTOTYPES)
MHAP_KMER_HISTOGRAM = 1   # mhap_kmer_count_finish_flags
MHAP_KMER_KEEP_OPEN = 2   # (the count stays open: mhap_kmer_count_finish_set may follow)
ABI_VERSION = 4   # MHAP_ABI_VERSION of include/mhap_hip.h this binding was written against


def load_library(build_if_missing=True):
    """Load libmhaphip.so (building it in-tree with hipcc if absent). Fails loudly: no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        if not build_if_missing:
            raise MhapError(f"{_LIB_PATH} is missing: run `python -m mhap_amd.build`")
        from . import build as _b
        _b.build()
    try:
        # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Importing torch first makes the
        # process use ONE HIP/HSA runtime; loading ours first and torch later leaves the second runtime without devices.
        import torch  # noqa: F401
    except Exception:
        pass
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as e:
        raise MhapError(f"cannot load the HIP extension {_LIB_PATH}: {e}") from e
    for name, proto in _PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        result, params = proto.split(":")
        fn.restype, fn.argtypes = _CTYPES[result], [_CTYPES[c] for c in params]
    # a stale library next to newer host code (or the reverse) must not get as far as a struct copy
    sizes = (C.c_int32 * 4)()
    lib.mhap_abi_sizes(sizes)
    want = [C.sizeof(_Params), RECORD_DTYPE.itemsize, C.sizeof(_Stats), C.sizeof(_KTimes)]
    if lib.mhap_abi_version() != ABI_VERSION or list(sizes) != want:
        raise MhapError(f"{_LIB_PATH} was built from another include/mhap_hip.h (ABI {lib.mhap_abi_version()}, struct sizes {list(sizes)}; "
                        f"this binding: ABI {ABI_VERSION}, {want}): rebuild it with `python -m mhap_amd.build`")
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _opt(a):
    """The pointer of an array that may be empty: an empty one goes down as NULL."""
    return _ptr(a) if len(a) else None


class MhapParams:
    """Flag table of J/main/MhapMain.java:67-125 (defaults identical)."""

    def __init__(self, kmer_size=16, num_hashes=512, ordered_kmer_size=12, ordered_sketch_size=1536, num_min_matches=3,
                 min_store_length=0, min_olap_length=116, threshold=0.78, max_shift=0.2, repeat_weight=0.9, device=-1):
        self.kmer_size = kmer_size
        self.num_hashes = num_hashes
        self.ordered_kmer_size = ordered_kmer_size
        self.ordered_sketch_size = ordered_sketch_size
        self.num_min_matches = num_min_matches
        self.min_store_length = min_store_length
        self.min_olap_length = min_olap_length
        self.threshold = threshold
        self.max_shift = max_shift
        self.repeat_weight = repeat_weight
        self.device = device

    def _c(self):
        return _Params(self.kmer_size, self.num_hashes, self.ordered_kmer_size, self.ordered_sketch_size,
                       self.num_min_matches, self.min_store_length, self.min_olap_length, self.device,
                       self.threshold, self.max_shift, self.repeat_weight)


class FastaData:
    """Reads (upper-cased, concatenated) + 1-based ids, as J/impl/FastaData.java:125-204 produces them."""

    def __init__(self, bases, offsets, lengths, ids, qualities=None):
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        # one Phred value (0 .. 93) per base, parallel to `bases`: what a FASTQ file brought ("FASTQ input" in include/mhap_hip.h); else None
        self.qualities = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8)

    def __len__(self):
        return int(self.lengths.shape[0])

    @classmethod
    def from_file(cls, path, id_offset=0):
        lib = load_library()
        f = _Fasta()
        err = C.create_string_buffer(512)
        qp = C.c_void_p()
        rc = lib.mhap_fasta_read_qualities(path.encode(), C.c_int64(id_offset), C.byref(f), C.byref(qp), err, C.c_size_t(512))
        if rc != 0:
            raise MhapError(err.value.decode() or f"mhap_fasta_read failed ({rc})")
        quals = None
        try:
            n, tb = f.n, f.total_bases
            if qp:
                quals = np.ctypeslib.as_array(C.cast(qp, C.POINTER(C.c_uint8)), shape=(max(tb, 1),))[:tb].copy()
                lib.mhap_qualities_free(qp)
            bases = np.ctypeslib.as_array(C.cast(f.bases, C.POINTER(C.c_uint8)), shape=(max(tb, 1),))[:tb].copy()
            offsets = np.ctypeslib.as_array(C.cast(f.offsets, C.POINTER(C.c_int64)), shape=(max(n, 1),))[:n].copy()
            lengths = np.ctypeslib.as_array(C.cast(f.lengths, C.POINTER(C.c_int32)), shape=(max(n, 1),))[:n].copy()
            ids = np.ctypeslib.as_array(C.cast(f.ids, C.POINTER(C.c_int64)), shape=(max(n, 1),))[:n].copy()
        finally:
            lib.mhap_fasta_free(C.byref(f))
        return cls(bases, offsets, lengths, ids, quals)

    @classmethod
    def from_strings(cls, seqs, id_offset=0):
        """Ids count only non-empty records, 1-based (FastaData.java:180-181)."""
        seqs = [s.upper() for s in seqs if len(s) > 0]
        lengths = np.array([len(s) for s in seqs], dtype=np.int32)
        offsets = np.zeros(len(seqs), dtype=np.int64)
        if len(seqs):
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        bases = np.frombuffer("".join(seqs).encode("latin-1"), dtype=np.uint8).copy() if seqs else np.zeros(0, np.uint8)
        ids = np.arange(1, len(seqs) + 1, dtype=np.int64) + id_offset
        return cls(bases, offsets, lengths, ids)

    def sequence(self, i):
        o, n = int(self.offsets[i]), int(self.lengths[i])
        return self.bases[o:o + n].tobytes().decode("latin-1")

    def subset(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        lengths = self.lengths[idx]
        offsets = np.zeros(len(idx), dtype=np.int64)
        if len(idx):
            offsets[1:] = np.cumsum(lengths[:-1], dtype=np.int64)
        bases = np.empty(int(lengths.sum()), dtype=np.uint8)
        quals = None if self.qualities is None else np.empty(len(bases), dtype=np.uint8)
        for j, i in enumerate(idx):
            bases[offsets[j]:offsets[j] + lengths[j]] = self.bases[self.offsets[i]:self.offsets[i] + self.lengths[i]]
            if quals is not None:
                quals[offsets[j]:offsets[j] + lengths[j]] = self.qualities[self.offsets[i]:self.offsets[i] + self.lengths[i]]
        return FastaData(bases, offsets, lengths, self.ids[idx], quals)


def synth_reads(n, length, seed=0x4D484150, coverage=30.0, error_rate=0.15, shard=0, nshards=1, repeats=None):
    """Deterministic synthetic PacBio-style reads as a FastaData.

    With nshards > 1 only reads shard, shard+nshards, ... of the same n-read data set are generated (ids kept).
    repeats = (element length, spacing, divergence) plants a repeat family in the genome (BASELINE configs[4])."""
    lib = load_library()
    idx = np.arange(shard, n, nshards, dtype=np.int64)
    m = len(idx)
    bases = np.empty(max(m * length, 1), dtype=np.uint8)
    rl, rs, rd = repeats if repeats else (0, 0, 0.0)
    rc = lib.mhap_synth_reads_repeats(C.c_uint64(seed), C.c_int64(n), C.c_int32(length), C.c_double(coverage),
                                      C.c_double(error_rate), C.c_int64(shard), C.c_int64(nshards), C.c_int32(rl), C.c_int32(rs),
                                      C.c_double(rd), _ptr(bases))
    if rc != 0:
        raise MhapError(f"mhap_synth_reads failed ({rc})")
    offsets = np.arange(m, dtype=np.int64) * length
    lengths = np.full(m, length, dtype=np.int32)
    return FastaData(bases[:m * length], offsets, lengths, idx + 1)


def synth_reads_from_genome(genome, lengths, seed=0x4D484150, error_rate=0.15):
    """Reads of the given lengths drawn from a supplied circular genome (uint8 codes 0..3): mhap_synth_reads_genome."""
    lib = load_library()
    genome = np.ascontiguousarray(genome, dtype=np.uint8)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    n = len(lengths)
    offsets = np.zeros(n, dtype=np.int64)
    if n > 1:
        np.cumsum(lengths[:-1].astype(np.int64), out=offsets[1:])
    bases = np.empty(max(int(lengths.astype(np.int64).sum()), 1), dtype=np.uint8)
    rc = lib.mhap_synth_reads_genome(C.c_uint64(seed), _ptr(genome), C.c_int64(len(genome)), C.c_int64(n), _ptr(lengths), _ptr(offsets),
                                     C.c_double(error_rate), _ptr(bases))
    if rc != 0:
        raise MhapError(f"mhap_synth_reads_genome failed ({rc})")
    return FastaData(bases, offsets, lengths, np.arange(1, n + 1, dtype=np.int64))


SYNTH_TRUTH_DTYPE = np.dtype([("start", "<i8"), ("span", "<i8"), ("strand", "i1"), ("ins", "<i4"), ("dels", "<i4"), ("subs", "<i4"),
                              ("length", "<i4")])


def synth_truth(n, length=None, seed=0x4D484150, coverage=30.0, error_rate=0.15, shard=0, nshards=1, lengths=None, genome_len=None):
    """Where the reads of synth_reads (length=..., coverage=..., shard/nshards) or of synth_reads_from_genome (lengths=..., genome_len=...)
    came from: mhap_synth_truth.  One SYNTH_TRUTH_DTYPE row per read: genome start, genome bases consumed (span; may wrap past the end
    of the circular genome), strand (1 = reverse complement), inserted / deleted / substituted bases, and the read's length.
    Returns (rows, genome length)."""
    lib = load_library()
    if lengths is not None:
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        if genome_len is None or len(lengths) != n:
            raise MhapError("synth_truth: the genome form needs genome_len and n == len(lengths)")
        m, G = n, int(genome_len)
    else:
        if length is None:
            raise MhapError("synth_truth: give length (synth_reads) or lengths + genome_len (synth_reads_from_genome)")
        m = len(range(shard, n, nshards))
        G = max(int(float(n) * float(length) / coverage), length + 1)   # mhap_synth_reads_repeats' genome length
    start, span = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
    strand = np.zeros(max(m, 1), np.int8)
    ins, dels, subs = (np.zeros(max(m, 1), np.int32) for _ in range(3))
    rc = lib.mhap_synth_truth(C.c_uint64(seed), C.c_int64(n), C.c_int32(length or 0), C.c_double(coverage), C.c_int64(G if lengths is not None else 0),
                              _ptr(lengths), C.c_double(error_rate), C.c_int64(shard), C.c_int64(nshards), _ptr(start), _ptr(span),
                              _ptr(strand), _ptr(ins), _ptr(dels), _ptr(subs))
    if rc != 0:
        raise MhapError(f"mhap_synth_truth failed ({rc})")
    out = np.zeros(m, SYNTH_TRUTH_DTYPE)
    out["start"], out["span"], out["strand"] = start[:m], span[:m], strand[:m]
    out["ins"], out["dels"], out["subs"] = ins[:m], dels[:m], subs[:m]
    out["length"] = lengths if lengths is not None else length
    return out, G


def align_pairs(bases, pairs, device=0, handle=None):
    """Local alignments of many segment pairs on the GPU (mhap_align_pairs; its header comment is the contract).  bases: uint8 array
    (FastaData.bases); pairs: int64 array (n, 5) of (a_off, a_len, b_off, b_len, b_rc).  Returns an int32 array (n, 7) of
    (score, read_begin, read_end, ref_begin, ref_end, columns, errors).  handle: a MinHashSearch whose device to use (else one is made)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 5))
    out = np.zeros((len(pairs), 7), dtype=np.int32)
    if len(pairs) == 0:
        return out
    own = handle is None
    ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) if own else handle
    try:
        ms._chk(ms._lib.mhap_align_pairs(ms._h, _ptr(bases), C.c_int64(len(bases)), _ptr(pairs), C.c_int64(len(pairs)), _ptr(out)))
    finally:
        if own:
            ms.close()
    return out


def align_pairs_banded(bases, pairs7, device=0, handle=None):
    """align_pairs inside a band (mhap_align_pairs_banded; its header comment is the contract).  pairs7: int64 array (n, 7) of
    (a_off, a_len, b_off, b_len, b_rc, diag, band): cell (i, j) is in the band iff |j - i - diag| <= band.  Returns the (n, 7) int32
    rows of align_pairs."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs7 = np.ascontiguousarray(np.asarray(pairs7, dtype=np.int64).reshape(-1, 7))
    out = np.zeros((len(pairs7), 7), dtype=np.int32)
    if len(pairs7) == 0:
        return out
    own = handle is None
    ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) if own else handle
    try:
        ms._chk(ms._lib.mhap_align_pairs_banded(ms._h, _ptr(bases), C.c_int64(len(bases)), _ptr(pairs7), C.c_int64(len(pairs7)), _ptr(out)))
    finally:
        if own:
            ms.close()
    return out


def _all_reads(fasta, query_fasta):
    """(bases, ids, offsets, lengths) of the indexed reads followed by the -q reads, as one array of bases."""
    if query_fasta is None or len(query_fasta) == 0:
        return fasta.bases, fasta.ids, fasta.offsets, fasta.lengths
    return (np.concatenate([fasta.bases, query_fasta.bases]), np.concatenate([fasta.ids, query_fasta.ids]),
            np.concatenate([fasta.offsets, query_fasta.offsets + len(fasta.bases)]), np.concatenate([fasta.lengths, query_fasta.lengths]))


def all_qualities(fasta, query_fasta=None):
    """The Phred bytes of the indexed reads followed by those of the -q reads, parallel to _all_reads' bases: what a weighted
    CorrectSession or ConsensusSession takes.  MhapError when a file brought none (it was FASTA)."""
    parts = [fasta] if query_fasta is None or len(query_fasta) == 0 else [fasta, query_fasta]
    if any(getattr(p, "qualities", None) is None for p in parts):
        raise MhapError("the reads have no base qualities (a FASTQ file brings them)")
    return parts[0].qualities if len(parts) == 1 else np.concatenate([p.qualities for p in parts])


WEIGHTED_VIEW_CAP = 21845   # MHAP_WEIGHTED_VIEW_CAP: accepted views per target of a weighted session (65 535 / 3)


class WeightParams(C.Structure):
    """mhap_weight_params: a base of Phred q votes with weight 1 (q < q_lo), 2 (q_lo <= q < q_hi) or 3 (q >= q_hi); 0 <= q_lo <= q_hi
    <= 93.  None for either takes the library's default ("quality-weighted votes" in include/mhap_hip.h)."""
    _fields_ = [("q_lo", C.c_int32), ("q_hi", C.c_int32)]

    def __init__(self, q_lo=None, q_hi=None):
        d = WeightParams.__new__(WeightParams)
        load_library().mhap_weight_default_params(C.byref(d))
        super().__init__(d.q_lo if q_lo is None else int(q_lo), d.q_hi if q_hi is None else int(q_hi))


def weight_classes_line(bases, qualities, weights=None):
    """The one stderr line of a weighted run (the driver prints the same): the A, C, G, T bases of the reads per weight class."""
    w = weights or WeightParams()
    b, q = np.asarray(bases, np.uint8), np.asarray(qualities, np.uint8)
    q = q[(b == 65) | (b == 67) | (b == 71) | (b == 84)]
    n1, n3 = int((q < w.q_lo).sum()), int((q >= w.q_hi).sum())
    return (f"Weights: q_lo = {w.q_lo}, q_hi = {w.q_hi}; {n1} bases of weight 1, {len(q) - n1 - n3} of weight 2, {n3} of weight 3")


def _weighted_args(bases, qualities, weights):
    """(the qualities as a checked array, the weight parameters) of a weighted begin; (None, None) without qualities."""
    if qualities is None:
        if weights is not None:
            raise MhapError("weights without qualities")
        return None, None
    q = np.ascontiguousarray(qualities, np.uint8)
    if q.shape != (len(bases),):
        raise MhapError(f"{len(bases)} bases need {len(bases)} quality bytes, not {q.shape}")
    return q, weights or WeightParams()


def realign_plan(records, fasta, band=0, max_shift=0.2, query_fasta=None):
    """The banded pairs of overlap records (mhap_realign_plan, no GPU): an int64 array (n, 7) for align_pairs_banded over the bases of
    `fasta` followed by those of `query_fasta`."""
    lib = load_library()
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
    ids, offsets = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(offsets, np.int64)
    lengths = np.ascontiguousarray(lengths, np.int32)
    pairs = np.zeros((len(records), 7), np.int64)
    rc = lib.mhap_realign_plan(_ptr(records), C.c_int64(len(records)), _ptr(ids), _ptr(offsets), _ptr(lengths), C.c_int64(len(ids)),
                               C.c_double(max_shift), C.c_int32(band), _ptr(pairs))
    if rc != 0:
        raise MhapError(f"{lib.mhap_realign_plan_error().decode()} (code {rc})")
    return pairs


def realign_records(records, fasta, band=0, max_shift=0.2, device=0, handle=None, query_fasta=None):
    """Realign overlap records on the GPU (mhap_realign_records): every record's interval and identity are replaced by those of the
    banded local alignment of its two reads around the diagonal the record implies.  records: RECORD_DTYPE array (a search's
    output); fasta: the FastaData the ids refer to (query_fasta: the -q reads, whose ids follow).  band = 0: the automatic band,
    max(1, int(max(a2 - a1, b2 - b1) * max_shift)) — with a `handle`, the max_shift of that handle's parameters is the one used.
    Returns (records, detail): detail is an int32 array (n, 3) of (score, columns, errors); a record without an alignment has score 0,
    positions 0 and a zero detail row."""
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    out = np.zeros(len(records), dtype=RECORD_DTYPE)
    detail = np.zeros((len(records), 3), dtype=np.int32)
    if len(records) == 0:
        return out, detail
    bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
    bases = np.ascontiguousarray(bases, np.uint8)
    ids, offsets = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(offsets, np.int64)
    lengths = np.ascontiguousarray(lengths, np.int32)
    own = handle is None
    ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device)) if own else handle
    try:
        ms._chk(ms._lib.mhap_realign_records(ms._h, _ptr(bases), C.c_int64(len(bases)), _ptr(ids), _ptr(offsets), _ptr(lengths),
                                             C.c_int64(len(ids)), _ptr(records), C.c_int64(len(records)), C.c_int32(band), _ptr(out),
                                             _ptr(detail)))
    finally:
        if own:
            ms.close()
    return out, detail


def _take_paths(lib, obj):
    """(op_offsets, ops) of a mhap_align_paths object, which is freed."""
    try:
        n, n_ops = C.c_int64(0), C.c_int64(0)
        lib.mhap_align_paths_info(obj, C.byref(n), C.byref(n_ops))
        op_offsets = np.zeros(n.value + 1, np.int64)
        ops = np.zeros(n_ops.value, np.uint32)
        if lib.mhap_align_paths_copy(obj, _ptr(op_offsets), _ptr(ops) if n_ops.value else None) != 0:
            raise MhapError("mhap_align_paths_copy failed")
        return op_offsets, ops
    finally:
        lib.mhap_align_paths_free(obj)


def align_pairs_banded_paths(bases, pairs7, handle=None, device=0):
    """align_pairs_banded and every alignment's path (mhap_align_pairs_banded_paths; the path contract is in its header comment).
    Returns (results, op_offsets, ops): results as align_pairs_banded returns them; pair q's runs are the uint32 values
    ops[op_offsets[q]:op_offsets[q + 1]], each len << 4 | code with code 7 '=', 8 'X', 1 'I', 2 'D', from the begin cell to the end
    cell (cigar_string writes them out)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    pairs7 = np.ascontiguousarray(np.asarray(pairs7, dtype=np.int64).reshape(-1, 7))
    out = np.zeros((len(pairs7), 7), dtype=np.int32)
    if len(pairs7) == 0:
        return out, np.zeros(1, np.int64), np.zeros(0, np.uint32)
    own = handle is None
    ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) if own else handle
    try:
        obj = C.c_void_p()
        ms._chk(ms._lib.mhap_align_pairs_banded_paths(ms._h, _ptr(bases), C.c_int64(len(bases)), _ptr(pairs7), C.c_int64(len(pairs7)),
                                                      _ptr(out), C.byref(obj)))
        op_offsets, ops = _take_paths(ms._lib, obj)
    finally:
        if own:
            ms.close()
    return out, op_offsets, ops


def realign_records_paths(records, fasta, band=0, max_shift=0.2, handle=None, device=0, query_fasta=None):
    """realign_records and every alignment's path (mhap_realign_records_paths).  Returns (records, detail, op_offsets, ops): the first
    two as realign_records returns them, the runs as align_pairs_banded_paths returns them for the pairs of realign_plan — on a
    to_rc record they run along the reverse complement of the `to` read (format_paf turns them round)."""
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    out = np.zeros(len(records), dtype=RECORD_DTYPE)
    detail = np.zeros((len(records), 3), dtype=np.int32)
    if len(records) == 0:
        return out, detail, np.zeros(1, np.int64), np.zeros(0, np.uint32)
    bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
    bases = np.ascontiguousarray(bases, np.uint8)
    ids, offsets = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(offsets, np.int64)
    lengths = np.ascontiguousarray(lengths, np.int32)
    own = handle is None
    ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, max_shift=max_shift, device=device)) if own else handle
    try:
        obj = C.c_void_p()
        ms._chk(ms._lib.mhap_realign_records_paths(ms._h, _ptr(bases), C.c_int64(len(bases)), _ptr(ids), _ptr(offsets), _ptr(lengths),
                                                   C.c_int64(len(ids)), _ptr(records), C.c_int64(len(records)), C.c_int32(band),
                                                   _ptr(out), _ptr(detail), C.byref(obj)))
        op_offsets, ops = _take_paths(ms._lib, obj)
    finally:
        if own:
            ms.close()
    return out, detail, op_offsets, ops


_CIGAR_LETTERS = "MIDNSHP=X???????"   # BAM's codes; the aligner writes 7, 8, 1 and 2


def cigar_string(ops, reverse=False):
    """The runs of one path (uint32, len << 4 | code) as a CIGAR with = X I D; reverse=True: in reverse order, which is the CIGAR of
    the same alignment with both sequences reverse-complemented."""
    ops = [int(x) for x in np.asarray(ops, dtype=np.uint32).reshape(-1).tolist()]
    return "".join(f"{op >> 4}{_CIGAR_LETTERS[op & 15]}" for op in (reversed(ops) if reverse else ops))


def format_paf(record, detail, ops, qname=None, tname=None):
    """One PAF line of a realigned record (mhap_format_paf): record and detail as realign_records_paths returns them, ops the
    record's runs.  The names default to the two ids, which is what columns 1 and 2 of the 12-column line hold."""
    lib = load_library()
    arr = np.zeros(1, dtype=RECORD_DTYPE)
    for k in RECORD_DTYPE.names:
        if k != "pad":
            arr[0][k] = record[k] if not isinstance(record, MatchResult) else getattr(record, k)
    detail = np.ascontiguousarray(detail, dtype=np.int32).reshape(3)
    ops = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1)
    qname = str(int(arr[0]["from_id"]) if qname is None else qname).encode()
    tname = str(int(arr[0]["to_id"]) if tname is None else tname).encode()
    cap = 256 + len(qname) + len(tname) + 12 * len(ops)
    buf = C.create_string_buffer(cap)
    n = lib.mhap_format_paf(_ptr(arr), _ptr(detail), _opt(ops), C.c_int64(len(ops)), qname, tname, buf, C.c_size_t(cap))
    if n < 0 or n >= cap:
        raise MhapError("mhap_format_paf failed")
    return buf.value.decode()


CORRECT_STATS = ("len_in", "len_out", "n_sub", "n_del", "n_ins", "n_low")   # the six counts per read of a correction
CORRECT_COUNTERS = 24   # per position: base A C G T, del, span, ins[k][A C G T] for k = 0 .. 3, two spare


class _Session:
    """What every session class shares: the MinHashSearch whose device and stream it uses, the caller's (handle=...) or one made here
    and closed with the session; the C session in `_s`; close(), `with` and the close of a session that is dropped.  A subclass names
    the prefix of its C entry points in `_prefix`: close() calls `<prefix>_free`."""

    _prefix = None

    def __init__(self, handle, device, begin):
        """begin(): the C begin, which fills `_s`.  Whatever it raises closes a handle made here."""
        self._own = handle is None
        self._ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) if self._own else handle
        self._lib = self._ms._lib
        self._s = C.c_void_p()
        try:
            begin()
        except Exception:
            if self._own:
                self._ms.close()
            raise

    def _c(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def close(self):
        if self._s:
            self._c("free")(self._s)
            self._s = C.c_void_p()
            if self._own:
                self._ms.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ReadsSession(_Session):
    """A session over a table of reads: (read_ids, lengths) and a struct of parameters go to `<prefix>_begin`, records to
    `<prefix>_add`, and `<prefix>_finish` fills the counts that `_counts` names."""

    _counts = ()

    def __init__(self, read_ids, lengths, params, handle, device):
        self.ids = np.ascontiguousarray(read_ids, np.int64)
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        super().__init__(handle, device, lambda: self._begin(params))

    def _begin(self, params):
        if len(self.ids) != len(self.lengths):
            raise MhapError(f"{type(self).__name__}: {len(self.ids)} ids and {len(self.lengths)} lengths")
        self._ms._chk(self._c("begin")(self._ms._h, _opt(self.ids), _opt(self.lengths), len(self.ids), C.byref(params), C.byref(self._s)))

    def add(self, records):
        """Take realigned records: piled up, classed or entered, as the session does (nothing waits for the device)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        self._ms._chk(self._c("add")(self._s, _opt(records), len(records)))

    def _finish(self):
        """`<prefix>_finish`: the dict of `_counts`."""
        counts = np.zeros(len(self._counts), np.int64)
        self._ms._chk(self._c("finish")(self._s, _ptr(counts)))
        return dict(zip(self._counts, counts.tolist()))


QUALITY_BINS = 94   # MHAP_QUALITY_BINS: Phred 0 .. 93


class QualityParams(C.Structure):
    """mhap_quality_params: per_vote, tenths of a Phred unit per net vote (1 .. 1000), and cap (1 .. 93)."""
    _fields_ = [("per_vote", C.c_int32), ("cap", C.c_int32)]

    def __init__(self, per_vote=15, cap=60):
        super().__init__(int(per_vote), int(cap))


def quality_counts_line(hist):
    """The one stderr line of a run that was asked for qualities (the driver prints the same), from the histogram."""
    h = [int(x) for x in hist]
    n = sum(h)
    mean = f"{sum(q * c for q, c in enumerate(h)) / n:.1f}" if n else "0.0"
    return f"Qualities: {n} bytes, {sum(h[:10])} below Q10, {sum(h[:20])} below Q20, mean {mean}"


def _qualities(ms, call, session, params, offsets):
    """What both quality() methods do: (one uint8 array per sequence of `offsets`, the histogram)."""
    flat, hist = np.zeros(int(offsets[-1]), np.uint8), np.zeros(QUALITY_BINS, np.int64)
    ms._chk(call(session, C.byref(params), _opt(flat), _ptr(hist)))
    return [flat[int(offsets[k]):int(offsets[k + 1])] for k in range(len(offsets) - 1)], hist


class CorrectSession(_Session):
    """Read correction on the GPU (mhap_correct_begin / _add / _finish / _votes; the contract is the "read correction" section of
    include/mhap_hip.h): every realigned overlap votes column by column on both of its reads, and each position takes the majority.
    The vote table (48 bytes per base) stays on the device from begin to close.

        with CorrectSession(fasta) as cs:
            cs.add(records, op_offsets, ops)          # what realign_records_paths returned; any number of times
            seqs, stats, skipped = cs.finish(min_cov=4)

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix = "mhap_correct"

    def __init__(self, fasta, query_fasta=None, handle=None, device=0, qualities=None, weights=None):
        """qualities: one Phred byte per base of the reads (all_qualities(fasta, query_fasta)) makes the session a weighted one
        (mhap_correct_begin_weighted; "quality-weighted votes" in include/mhap_hip.h), weights its WeightParams (None: the defaults)."""
        bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
        self._bases = np.ascontiguousarray(bases, np.uint8)
        self.ids, self._offsets = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(offsets, np.int64)
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        self._quals, self.weights = _weighted_args(self._bases, qualities, weights)
        if self._quals is None:
            begin = lambda: self._lib.mhap_correct_begin(   # noqa: E731
                self._ms._h, _ptr(self._bases), len(self._bases), _ptr(self.ids), _ptr(self._offsets), _ptr(self.lengths), len(self.ids),
                C.byref(self._s))
        else:   # (an empty array has no bytes to point at, and NULL would mean "unweighted")
            begin = lambda: self._lib.mhap_correct_begin_weighted(   # noqa: E731
                self._ms._h, _ptr(self._bases), _ptr(self._quals if len(self._quals) else np.zeros(1, np.uint8)), len(self._bases), _ptr(self.ids),
                _ptr(self._offsets), _ptr(self.lengths), len(self.ids), C.byref(self.weights), C.byref(self._s))
        super().__init__(handle, device, lambda: self._ms._chk(begin()))

    @classmethod
    def begin(cls, fasta, query_fasta=None, handle=None, device=0, qualities=None, weights=None):
        """The constructor under the C entry point's name: the bases go up and the vote table is zeroed."""
        return cls(fasta, query_fasta=query_fasta, handle=handle, device=device, qualities=qualities, weights=weights)

    def add(self, records, op_offsets, ops, views=None):
        """The votes of realigned records and their runs (pair q's are ops[op_offsets[q]:op_offsets[q + 1]]).  views: one byte per
        record, bit 0 view A votes, bit 1 view B (SelectSession.apply makes them); None: both views of every record."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        if views is not None:
            views = np.ascontiguousarray(views, dtype=np.uint8)
            if views.shape != (len(records),):
                raise MhapError(f"CorrectSession.add: {len(records)} records need {len(records)} view bytes, not {views.shape}")
        op_offsets = np.ascontiguousarray(op_offsets, dtype=np.int64)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        if len(op_offsets) != len(records) + 1:
            raise MhapError(f"CorrectSession.add: {len(records)} records need {len(records) + 1} run offsets, not {len(op_offsets)}")
        obj = C.c_void_p()
        if self._lib.mhap_align_paths_from_runs(_ptr(op_offsets), C.c_int64(len(records)), _opt(ops), C.byref(obj)) != 0:
            raise MhapError("CorrectSession.add: op_offsets is not a list of run offsets over ops")
        try:
            recs = _opt(records)
            if views is None:
                self._ms._chk(self._lib.mhap_correct_add(self._s, recs, C.c_int64(len(records)), obj))
            else:   # (an empty array has no bytes to point at, and NULL would mean "both")
                self._ms._chk(self._lib.mhap_correct_add_views(self._s, recs, C.c_int64(len(records)), obj,
                                                               _ptr(views if len(views) else np.zeros(1, np.uint8))))
        finally:
            self._lib.mhap_align_paths_free(obj)

    def finish(self, min_cov=4):
        """(seqs, stats, skipped_views): the corrected bytes of every read, an int32 array (n, 6) of CORRECT_STATS, and the views the
        65 535-per-target cap has skipped so far.  `offsets` and `bytes` keep the flat form: read r is bytes[offsets[r]:offsets[r + 1]]."""
        n = len(self.ids)
        self.offsets = np.zeros(n + 1, np.int64)
        stats = np.zeros((n, 6), np.int32)
        skipped = C.c_int64(0)
        self._ms._chk(self._lib.mhap_correct_finish(self._s, C.c_int32(min_cov), _ptr(self.offsets), _ptr(stats) if n else None, C.byref(skipped)))
        self.bytes = np.zeros(int(self.offsets[n]), np.uint8)
        self._ms._chk(self._lib.mhap_correct_copy(self._s, _opt(self.bytes)))
        raw = self.bytes.tobytes()
        return [raw[int(self.offsets[r]):int(self.offsets[r + 1])] for r in range(n)], stats, int(skipped.value)

    def votes(self, read_index):
        """The raw counters of one read: a uint16 array (length, CORRECT_COUNTERS)."""
        if not 0 <= read_index < len(self.ids):
            raise MhapError(f"CorrectSession.votes: read {read_index} is not among the {len(self.ids)} reads")
        out = np.zeros((int(self.lengths[read_index]), CORRECT_COUNTERS), np.uint16)
        self._ms._chk(self._lib.mhap_correct_votes(self._s, C.c_int64(read_index), _opt(out)))
        return out

    def quality(self, per_vote=15, cap=60):
        """(quals, hist) of the last finish (mhap_correct_quality; "base qualities" in include/mhap_hip.h): a uint8 array per read, as
        long as its corrected bytes, and the int64 histogram of QUALITY_BINS bins over all of them."""
        off = getattr(self, "offsets", np.zeros(1, np.int64))   # (no finish yet: the library refuses)
        return _qualities(self._ms, self._lib.mhap_correct_quality, self._s, QualityParams(per_vote, cap), off)

    def table_bytes(self):
        return 48 * int(self.lengths.astype(np.int64).sum())


def correct_reads(records, fasta, op_offsets, ops, min_cov=4, query_fasta=None, handle=None, device=0):
    """Correct every read of `fasta` (and `query_fasta`) from realigned records and their runs, as realign_records_paths returned them:
    (seqs, stats, skipped_views) of CorrectSession.finish."""
    with CorrectSession(fasta, query_fasta=query_fasta, handle=handle, device=device) as cs:
        cs.add(records, op_offsets, ops)
        return cs.finish(min_cov)


GRAPH_CLASSES = ("none", "internal", "a_contained", "b_contained", "short", "dovetail")   # the class codes 0 .. 5 of a record
GRAPH_COUNTS = ("records",) + GRAPH_CLASSES + ("contained_reads", "arcs", "reduced", "final")   # mhap_graph_finish's counts, in order
GRAPH_ARC_FIELDS = ("u", "v", "len", "ol", "q", "reduced", "final")


UNITIG_COUNTS = ("unitigs", "circular", "members", "joined_arcs", "links", "longest_bases", "total_bases")   # mhap_graph_unitigs' counts
UNITIG_LINK_FIELDS = ("from_unitig", "from_orient", "to_unitig", "to_orient", "ol", "arc")


CLEAN_COUNTS = ("rounds", "tip_unitigs", "tip_reads", "bubble_unitigs", "bubble_reads", "arcs_removed")   # mhap_graph_clean's counts


class _CleanParams(C.Structure):
    _fields_ = [("tip_reads", C.c_int32), ("bubble_bases", C.c_int32), ("max_rounds", C.c_int32)]


class _GraphParams(C.Structure):
    _fields_ = [("max_hang", C.c_int32), ("int_frac_permille", C.c_int32), ("min_ovlp", C.c_int32), ("fuzz", C.c_int32),
                ("min_identity", C.c_double)]


def format_gfa_link(row, read_ids):
    """The GFA L line of one arc row (mhap_format_gfa_link, no GPU), without the newline."""
    lib = load_library()
    row = np.ascontiguousarray(row, dtype=np.int32).reshape(7)
    read_ids = np.ascontiguousarray(read_ids, dtype=np.int64)
    buf = C.create_string_buffer(96)
    n = lib.mhap_format_gfa_link(_ptr(row), _ptr(read_ids), buf, C.c_size_t(96))
    if n < 0 or n >= 96:
        raise MhapError("mhap_format_gfa_link failed")
    return buf.value.decode()


def format_gfa(read_ids, lengths, contained, arcs, dropped=None, removed=None):
    """GFA 1 text of a string graph: the header, an S line per read that is not contained (in read_ids order), an L line per final
    arc (in list order).  The "string graph" section of include/mhap_hip.h has the format.  With the `dropped` and `removed` bytes
    of a cleaning, the text of the cleaned graph: no S line for a dropped read, no L line for a removed arc."""
    arcs = np.ascontiguousarray(arcs, dtype=np.int32).reshape(-1, 7)
    gone = np.asarray(contained) != 0
    keep = arcs[:, 6] != 0
    if dropped is not None:
        gone = gone | (np.asarray(dropped) != 0)
        keep = keep & (np.asarray(removed) == 0)
    out = ["H\tVN:Z:1.0\n"]
    out += [f"S\t{i}\t*\tLN:i:{n}\n" for i, n, c in zip(np.asarray(read_ids).tolist(), np.asarray(lengths).tolist(), gone.tolist()) if not c]
    out += [format_gfa_link(r, read_ids) + "\n" for r in arcs[keep]]
    return "".join(out)


def format_gfa_unitig_link(row):
    """The GFA L line of one link row of the unitig graph (mhap_format_gfa_unitig_link, no GPU), without the newline."""
    lib = load_library()
    row = np.ascontiguousarray(row, dtype=np.int32).reshape(6)
    buf = C.create_string_buffer(96)
    n = lib.mhap_format_gfa_unitig_link(_ptr(row), buf, C.c_size_t(96))
    if n < 0 or n >= 96:
        raise MhapError("mhap_format_gfa_unitig_link failed")
    return buf.value.decode()


def unitig_counts_line(counts):
    """The one stderr line of the unitigs (the driver prints the same); counts: the MHAP_UNITIG_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Unitigs: {c[0]} unitigs ({c[1]} circular) of {c[2]} reads, {c[3]} joined arcs, {c[4]} links; longest {c[5]} bases, "
            f"{c[6]} bases in all")


def clean_counts_line(counts):
    """The one stderr line of a graph cleaning (the driver prints the same); counts: the MHAP_CLEAN_COUNTS values in order."""
    c = [int(x) for x in counts]
    return f"Cleaned in {c[0]} rounds: {c[1]} tips ({c[2]} reads), {c[3]} bubbles ({c[4]} reads), {c[5]} arcs removed"


def format_unitig_gfa(read_ids, unitigs, sequences):
    """GFA 1 text of the unitig graph: the header, per unitig its S line and an `a` line per member, then an L line per link.
    unitigs: the dict of GraphSession.unitigs(); sequences: a list of bytes, one per unitig.  The "unitigs" part of the string-graph
    section of include/mhap_hip.h has the format."""
    ids = np.asarray(read_ids).tolist()
    start, ulen, circ = unitigs["unitig_start"].tolist(), unitigs["unitig_len"].tolist(), unitigs["circular"].tolist()
    vertex, offset, span = unitigs["vertex"].tolist(), unitigs["offset"].tolist(), unitigs["span"].tolist()
    out = ["H\tVN:Z:1.0\n"]
    for k, seq in enumerate(sequences):
        name = f"utg{k + 1:06d}{'c' if circ[k] else 'l'}"
        out.append(f"S\t{name}\t{seq.decode('latin-1')}\tLN:i:{ulen[k]}\tnr:i:{start[k + 1] - start[k]}\n")
        out += [f"a\t{name}\t{offset[m]}\t{ids[vertex[m] >> 1]}:1-{span[m]}\t{'-' if vertex[m] & 1 else '+'}\t{span[m]}\n"
                for m in range(start[k], start[k + 1])]
    out += [format_gfa_unitig_link(r) + "\n" for r in np.ascontiguousarray(unitigs["links"], dtype=np.int32).reshape(-1, 6)]
    return "".join(out)


class GraphSession(_ReadsSession):
    """The string graph of realigned overlaps on the GPU (mhap_graph_begin / _add / _finish / _copy_*; the contract is the "string
    graph" section of include/mhap_hip.h): every record is classed, contained reads are set aside, the dovetails become arcs and
    the arcs a two-arc path explains are reduced.

        with GraphSession(fasta.ids, fasta.lengths) as gs:
            gs.add(records)                       # what realign_records returned; any number of times
            arcs, counts = gs.finish()            # int32 (n, 7) of GRAPH_ARC_FIELDS, a dict of GRAPH_COUNTS
            text = gs.gfa()
            u = gs.unitigs()                      # the final arcs compacted into chains: a dict of arrays
            seqs = gs.unitig_sequences(fasta)     # their sequences, a list of bytes; gs.unitig_gfa(fasta) is the GFA text
            gs.clean()                            # tips and simple bubbles removed in rounds: a dict of CLEAN_COUNTS; after it
                                                  # gs.cleaned_unitigs(), gs.gfa(cleaned=True), and the two calls above follow it

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix, _counts = "mhap_graph", GRAPH_COUNTS

    def __init__(self, read_ids, lengths, max_hang=1000, int_frac_permille=800, min_ovlp=2000, fuzz=1000, min_identity=0.0, handle=None,
                 device=0):
        self.arcs = np.zeros((0, 7), np.int32)
        self.unitigs_table = None
        self.cleaned_table = None
        super().__init__(read_ids, lengths, _GraphParams(max_hang, int_frac_permille, min_ovlp, fuzz, min_identity), handle, device)

    def finish(self):
        """(arcs, counts): the de-duplicated arc list as an int32 array (n, 7) of GRAPH_ARC_FIELDS and a dict of GRAPH_COUNTS."""
        self.unitigs_table = None
        self.cleaned_table = None
        counts = self._finish()
        self.arcs = np.zeros((counts["arcs"], 7), np.int32)
        self._ms._chk(self._lib.mhap_graph_copy_arcs(self._s, _opt(self.arcs)))
        self.counts = counts
        return self.arcs, self.counts

    def info(self):
        """(reads, records added so far, arcs of the last finish or -1)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ms._chk(self._lib.mhap_graph_info(self._s, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def classes(self):
        """The class code of every record added so far, in arrival order (uint8; GRAPH_CLASSES names them)."""
        out = np.zeros(self.info()[1], np.uint8)
        self._ms._chk(self._lib.mhap_graph_copy_classes(self._s, _opt(out)))
        return out

    def contained(self):
        """One byte per read: 1 when some record classes it contained."""
        out = np.zeros(len(self.ids), np.uint8)
        self._ms._chk(self._lib.mhap_graph_copy_read_flags(self._s, _opt(out)))
        return out

    def gfa(self, cleaned=False):
        """The GFA 1 text of the last finish; cleaned=True: without the reads and arcs the last clean() removed."""
        if cleaned:
            return format_gfa(self.ids, self.lengths, self.contained(), self.arcs, self.dropped(), self.removed())
        return format_gfa(self.ids, self.lengths, self.contained(), self.arcs)

    def _copy_unitigs(self):
        """The tables of the unitigs the session serves now, without their counts."""
        n, members, links, _ = self.unitigs_info()
        u = dict(unitig_start=np.zeros(n + 1, np.int64), unitig_len=np.zeros(n, np.int64), circular=np.zeros(n, np.uint8),
                 vertex=np.zeros(members, np.int32), offset=np.zeros(members, np.int64), span=np.zeros(members, np.int32),
                 links=np.zeros((links, 6), np.int32))
        self._ms._chk(self._lib.mhap_graph_copy_unitigs(self._s, _ptr(u["unitig_start"]), _opt(u["unitig_len"]), _opt(u["circular"])))
        self._ms._chk(self._lib.mhap_graph_copy_layout(self._s, _opt(u["vertex"]), _opt(u["offset"]), _opt(u["span"])))
        self._ms._chk(self._lib.mhap_graph_copy_links(self._s, _opt(u["links"])))
        return u

    def unitigs(self):
        """The unitigs of the last finish (mhap_graph_unitigs / _copy_*): a dict of unitig_start (n + 1), unitig_len (n), circular (n),
        the members' vertex, offset, span, the link rows (links, 6) of UNITIG_LINK_FIELDS, and counts, a dict of UNITIG_COUNTS.
        Always the uncleaned ones, after a clean() too."""
        counts = np.zeros(len(UNITIG_COUNTS), np.int64)
        self._ms._chk(self._lib.mhap_graph_unitigs(self._s, _ptr(counts)))
        u = self._copy_unitigs()
        u["counts"] = dict(zip(UNITIG_COUNTS, counts.tolist()))
        self.unitigs_table = u
        return u

    def clean(self, tip_reads=4, bubble_bases=50000, max_rounds=16):
        """Clip tips and pop simple bubbles in rounds (mhap_graph_clean; "graph cleaning" in include/mhap_hip.h): a dict of
        CLEAN_COUNTS.  Afterwards the session serves the cleaned unitigs: cleaned_unitigs() has their tables, unitig_sequences and
        unitig_gfa follow them, gfa(cleaned=True) is the cleaned read graph.  Each call starts again from the uncleaned graph."""
        counts = np.zeros(len(CLEAN_COUNTS), np.int64)
        self.cleaned_table = None
        self.unitigs_table = None
        p = _CleanParams(tip_reads, bubble_bases, max_rounds)
        self._ms._chk(self._lib.mhap_graph_clean(self._s, C.byref(p), _ptr(counts)))
        u = self._copy_unitigs()
        ucounts = np.zeros(len(UNITIG_COUNTS), np.int64)
        self._ms._chk(self._lib.mhap_graph_unitigs_counts(self._s, _ptr(ucounts)))
        u["counts"] = dict(zip(UNITIG_COUNTS, ucounts.tolist()))
        self.cleaned_table = self.unitigs_table = u
        self.clean_counts = dict(zip(CLEAN_COUNTS, counts.tolist()))
        return self.clean_counts

    def cleaned_unitigs(self):
        """The unitigs of the last clean(), in the shape of unitigs(), as they were read then: nothing is built again."""
        if self.cleaned_table is None:
            raise MhapError("GraphSession.cleaned_unitigs: no clean() since the last finish()")
        return self.cleaned_table

    def dropped(self):
        """One byte per read after a clean(): 0 in play, 1 dropped as a tip, 2 as a bubble."""
        out = np.zeros(len(self.ids), np.uint8)
        self._ms._chk(self._lib.mhap_graph_copy_dropped(self._s, _opt(out)))
        return out

    def removed(self):
        """One byte per arc of the list after a clean(): 1 when the arc is final and one of its reads is dropped."""
        out = np.zeros(len(self.arcs), np.uint8)
        self._ms._chk(self._lib.mhap_graph_copy_removed(self._s, _opt(out)))
        return out

    def spell_into(self, bases, offsets, out):
        """mhap_graph_spell: the sequences of all unitigs back to back into the uint8 array `out` (total_bases of the counts long);
        read r's bytes are bases[offsets[r]:offsets[r] + lengths[r]]."""
        bases = np.ascontiguousarray(bases, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.int64)
        if len(offsets) != len(self.ids):
            raise MhapError(f"GraphSession: {len(offsets)} offsets for {len(self.ids)} reads")
        if out.dtype != np.uint8 or not out.flags.c_contiguous or (self.unitigs_table is not None and len(out) != self.unitigs_table["counts"]["total_bases"]):
            raise MhapError("GraphSession.spell_into: out must be a contiguous uint8 array of total_bases bytes")
        self._ms._chk(self._lib.mhap_graph_spell(self._s, _opt(bases), C.c_int64(len(bases)), _opt(offsets), _opt(out)))
        return out

    def unitig_sequences(self, fasta, query_fasta=None):
        """The sequence of every unitig, a list of bytes (mhap_graph_spell): `fasta` (and `query_fasta`) hold the session's reads in
        read_ids order.  Runs unitigs() first when it has not run since the last finish."""
        u = self.unitigs_table or self.unitigs()
        bases, _, offsets, _ = _all_reads(fasta, query_fasta)
        raw = self.spell_into(bases, offsets, np.zeros(int(u["counts"]["total_bases"]), np.uint8)).tobytes()
        ends = np.cumsum(u["unitig_len"]).tolist()
        return [raw[e - n:e] for e, n in zip(ends, u["unitig_len"].tolist())]

    def unitig_gfa(self, fasta, query_fasta=None):
        """The GFA 1 text of the unitig graph of the last finish, with sequences."""
        seqs = self.unitig_sequences(fasta, query_fasta)
        return format_unitig_gfa(self.ids, self.unitigs_table, seqs)

    def unitigs_info(self):
        """(unitigs or -1 while there are none for the last finish, members, links, bases)."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ms._chk(self._lib.mhap_graph_unitigs_info(self._s, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value


HPC_TILE = 4096         # MHAP_HPC_TILE: the positions a workgroup of the two compression passes takes
HPC_SCAN_BLOCK = 4096   # MHAP_HPC_SCAN_BLOCK: the tile counts the scan takes at once
HPC_COUNTS = ("reads", "raw_bases", "compressed_bases", "long_runs", "longest_run", "empty_reads")   # mhap_hpc_info's counts, in order


def hpc_counts_line(counts):
    """The one stderr line of a homopolymer compression (the drivers print the same); counts: the MHAP_HPC_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Homopolymer compression: {c[0]} reads ({c[5]} empty), {c[1]} bases compressed to {c[2]}; {c[3]} runs longer than 1, "
            f"the longest of {c[4]}")


def hpc_expand_record(record, start_from, start_to=None):
    """One record in compressed coordinates carried to raw ones through explicit maps (mhap_hpc_expand_record, no GPU; "homopolymer
    compression" in include/mhap_hip.h).  start_from, start_to: the clen + 1 entries of the two reads' maps (None: the same read's)."""
    lib = load_library()
    rec = np.ascontiguousarray(record, dtype=RECORD_DTYPE).reshape(1)
    out = np.zeros(1, RECORD_DTYPE)
    sf = np.ascontiguousarray(start_from, np.int32)
    st = sf if start_to is None else np.ascontiguousarray(start_to, np.int32)
    if len(sf) < 1 or len(st) < 1 or lib.mhap_hpc_expand_record(_ptr(rec), _ptr(sf), C.c_int32(len(sf) - 1), _ptr(st), C.c_int32(len(st) - 1), _ptr(out)) != 0:
        raise MhapError("mhap_hpc_expand_record: a map has at least one entry")
    return out[0]


TRIM_COUNTS = ("reads", "deleted", "cut5", "cut3", "gapped", "bases_in", "bases_kept", "eligible_records")   # mhap_trim_finish's counts
TRIM_ROW_FIELDS = ("begin", "end", "runs", "covered")
TRIM_DELETED, TRIM_CUT5, TRIM_CUT3, TRIM_GAPPED = 1, 2, 4, 8   # the bits of a read's flag byte
TRIM_TILE = 4096   # MHAP_TRIM_TILE: the positions the run kernel takes at a time


class _TrimParams(C.Structure):
    _fields_ = [("min_cov", C.c_int32), ("end_clip", C.c_int32), ("min_span", C.c_int32), ("min_identity", C.c_double)]


def trim_counts_line(counts):
    """The one stderr line of a trimming (the driver prints the same); counts: the MHAP_TRIM_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Trim: {c[0]} reads, {c[1]} deleted, {c[2]} cut at 5', {c[3]} cut at 3', {c[4]} gapped; {c[6]} of {c[5]} bases kept, "
            f"{c[7]} eligible overlaps")


def trim_clip_record(record, clear_a, clear_b, min_cov=3, end_clip=500, min_span=2000, min_identity=0.0):
    """One record rewritten onto explicit clear ranges (mhap_trim_clip_record, no GPU): (kept, record)."""
    lib = load_library()
    rec = np.ascontiguousarray(record, dtype=RECORD_DTYPE).reshape(1)
    out = np.zeros(1, RECORD_DTYPE)
    ca, cb = np.ascontiguousarray(clear_a, np.int32).reshape(2), np.ascontiguousarray(clear_b, np.int32).reshape(2)
    p = _TrimParams(min_cov, end_clip, min_span, min_identity)
    rc = lib.mhap_trim_clip_record(_ptr(rec), _ptr(ca), _ptr(cb), C.byref(p), _ptr(out))
    if rc < 0:
        raise MhapError("mhap_trim_clip_record: bad parameters")
    return bool(rc), out[0]


TRIM_PENALTY = 2   # the refinement's cost of an error column next to +1 for a match: break-even at an identity of 2 / 3


def trim_refine_record(record, ops, penalty=TRIM_PENALTY):
    """One record cut to the best stretch of its path (mhap_trim_refine_record, no GPU): (refined, record)."""
    lib = load_library()
    rec = np.ascontiguousarray(record, dtype=RECORD_DTYPE).reshape(1)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    out = np.zeros(1, RECORD_DTYPE)
    rc = lib.mhap_trim_refine_record(_ptr(rec), _opt(ops), C.c_int64(len(ops)), C.c_int32(penalty), _ptr(out))
    if rc < 0:
        raise MhapError("mhap_trim_refine_record: bad argument")
    return bool(rc), out[0]


def trim_refine(records, op_offsets, ops, penalty=TRIM_PENALTY, handle=None, device=0):
    """Realigned records cut to the best stretch of their paths on the GPU (mhap_trim_refine; "read trimming" in include/mhap_hip.h):
    records, op_offsets and ops as realign_records_paths returns them.  The refined records."""
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    op_offsets = np.ascontiguousarray(op_offsets, dtype=np.int64)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    if len(op_offsets) != len(records) + 1:
        raise MhapError(f"trim_refine: {len(records)} records need {len(records) + 1} run offsets, not {len(op_offsets)}")
    ms = handle or MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device))
    try:
        obj = C.c_void_p()
        if ms._lib.mhap_align_paths_from_runs(_ptr(op_offsets), C.c_int64(len(records)), _opt(ops), C.byref(obj)) != 0:
            raise MhapError("trim_refine: op_offsets is not a list of run offsets over ops")
        out = np.zeros(len(records), RECORD_DTYPE)
        try:
            ms._chk(ms._lib.mhap_trim_refine(ms._h, _opt(records), C.c_int64(len(records)), obj, C.c_int32(penalty), _opt(out)))
        finally:
            ms._lib.mhap_align_paths_free(obj)
        return out
    finally:
        if handle is None:
            ms.close()


class TrimSession(_ReadsSession):
    """Reads cut to the stretch that other reads support (mhap_trim_begin / _add / _finish / _copy / _apply; the contract is the
    "read trimming" section of include/mhap_hip.h).

        with TrimSession(fasta.ids, fasta.lengths) as ts:
            ts.add(records)                       # what realign_records returned; any number of times
            counts = ts.finish()                  # a dict of TRIM_COUNTS
            rows, flags = ts.table()              # int32 (n, 4) of TRIM_ROW_FIELDS, uint8 (n) of the TRIM_* bits
            out, keep = ts.apply(records)         # the records on the trimmed reads; out[keep != 0] are the ones that stay
            cut = ts.trimmed(fasta)               # the surviving reads as a FastaData over the same bases

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix, _counts = "mhap_trim", TRIM_COUNTS
    rows = flags = None

    def __init__(self, read_ids, lengths, min_cov=3, end_clip=500, min_span=2000, min_identity=0.0, handle=None, device=0):
        super().__init__(read_ids, lengths, _TrimParams(min_cov, end_clip, min_span, min_identity), handle, device)

    def finish(self):
        """Make every read's row and flags; returns a dict of TRIM_COUNTS."""
        self.rows = self.flags = None
        self.counts = self._finish()
        return self.counts

    def table(self):
        """(rows, flags) of the last finish: int32 (n, 4) of TRIM_ROW_FIELDS and one byte of TRIM_* bits per read."""
        if self.rows is None:
            rows, flags = np.zeros((len(self.ids), 4), np.int32), np.zeros(len(self.ids), np.uint8)
            self._ms._chk(self._lib.mhap_trim_copy(self._s, _opt(rows), _opt(flags)))
            self.rows, self.flags = rows, flags
        return self.rows, self.flags

    def coverage(self, read_index):
        """cov of every position of one read as the adds so far have left it (int32)."""
        if not 0 <= read_index < len(self.ids):
            raise MhapError("TrimSession.coverage: no such read")
        out = np.zeros(int(self.lengths[read_index]), np.int32)
        self._ms._chk(self._lib.mhap_trim_coverage(self._s, C.c_int64(read_index), _opt(out)))
        return out

    def apply(self, records):
        """(out, keep): the records rewritten onto the trimmed reads of the last finish and one byte per record, 0 for a void one
        (which comes back as it went in); out[keep != 0] is the compacted list."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        out, keep = np.zeros(len(records), RECORD_DTYPE), np.zeros(len(records), np.uint8)
        self._ms._chk(self._lib.mhap_trim_apply(self._s, _opt(records), C.c_int64(len(records)), _opt(out), _opt(keep)))
        return out, keep

    def trimmed(self, fasta):
        """The surviving reads of the last finish as a FastaData: ids, trimmed lengths, and offsets shifted by `begin` into the same
        `bases` (nothing is copied).  `fasta` holds the session's reads in read_ids order."""
        if len(fasta) != len(self.ids):
            raise MhapError(f"TrimSession.trimmed: {len(fasta)} reads for a session of {len(self.ids)}")
        rows, flags = self.table()
        live = np.flatnonzero((flags & TRIM_DELETED) == 0)
        return FastaData(fasta.bases, fasta.offsets[live] + rows[live, 0], rows[live, 1] - rows[live, 0], self.ids[live],
                         getattr(fasta, "qualities", None))   # (parallel to the same bases: a trimmed read's qualities are the matching slice)


REPEAT_COUNTS = ("reads", "reads_with_interval", "whole_reads", "intervals", "repeat_bases", "bases", "eligible_records", "depth",
                 "threshold")   # mhap_repeat_finish's counts
REPEAT_ROW_FIELDS = ("intervals", "repeat_bases", "max_cov", "first_begin")
REPEAT_SOME, REPEAT_WHOLE = 1, 2   # the bits of a read's flag byte
REPEAT_BINS = 4096   # MHAP_REPEAT_BINS: the bins of the depth histogram, the last one holding every greater depth
REPEAT_DEFAULTS = dict(factor_pct=200, max_cov=0, min_run=500, min_unique=500, min_identity=0.0)   # choices, not measurements


class _RepeatParams(C.Structure):
    _fields_ = [("factor_pct", C.c_int32), ("max_cov", C.c_int32), ("min_run", C.c_int32), ("min_unique", C.c_int32),
                ("min_identity", C.c_double)]


def repeat_counts_line(counts):
    """The one stderr line of a repeat marking (the driver prints the same); counts: the MHAP_REPEAT_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Repeats: {c[0]} reads, {c[1]} with a repeat, {c[2]} repeat throughout; {c[3]} intervals, {c[4]} of {c[5]} bases; "
            f"{c[6]} eligible overlaps, depth {c[7]}, threshold {c[8]}")


def repeat_judge_record(record, intervals_a, intervals_b, factor_pct=200, max_cov=0, min_run=500, min_unique=500, min_identity=0.0):
    """One record against explicit interval lists [(begin, end), ...] of its two reads (mhap_repeat_judge_record, no GPU):
    (keep, uA, uB)."""
    lib = load_library()
    rec = np.ascontiguousarray(record, dtype=RECORD_DTYPE).reshape(1)
    ia, ib = (np.ascontiguousarray(x, np.int32).reshape(-1, 2) for x in (intervals_a, intervals_b))
    u = np.zeros(2, np.int32)
    p = _RepeatParams(factor_pct, max_cov, min_run, min_unique, min_identity)
    rc = lib.mhap_repeat_judge_record(_ptr(rec), _opt(ia), C.c_int64(len(ia)), _opt(ib),
                                      C.c_int64(len(ib)), C.byref(p), _ptr(u))
    if rc < 0:
        raise MhapError("mhap_repeat_judge_record: bad parameters, interval list or record")
    return bool(rc), int(u[0]), int(u[1])


class RepeatSession(_ReadsSession):
    """Repeats marked from the overlap pile-up (mhap_repeat_begin / _add / _finish / _copy / _histogram / _apply; the contract is the
    "repeat marking" section of include/mhap_hip.h).

        with RepeatSession(fasta.ids, fasta.lengths) as rs:
            rs.add(records)                       # realigned (and refined) records; any number of times
            counts = rs.finish()                  # a dict of REPEAT_COUNTS
            rows, flags, offsets, intervals = rs.table()   # read r's intervals: intervals[offsets[r]:offsets[r + 1]], (begin, end)
            bins = rs.histogram()                 # int64 (REPEAT_BINS)
            keep, unique = rs.apply(records)      # records[keep != 0] are the ones that stay; unique: int32 (n, 2) of uA, uB

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix, _counts = "mhap_repeat", REPEAT_COUNTS
    _table = counts = None

    def __init__(self, read_ids, lengths, factor_pct=200, max_cov=0, min_run=500, min_unique=500, min_identity=0.0, handle=None, device=0):
        super().__init__(read_ids, lengths, _RepeatParams(factor_pct, max_cov, min_run, min_unique, min_identity), handle, device)

    def finish(self):
        """Make the histogram, the depth and threshold and every read's intervals; returns a dict of REPEAT_COUNTS."""
        self._table = self.counts = None
        self.counts = self._finish()
        return self.counts

    def table(self):
        """(rows, flags, offsets, intervals) of the last finish: int32 (n, 4) of REPEAT_ROW_FIELDS, one byte of REPEAT_* bits per read,
        int64 (n + 1) and int32 (intervals, 2)."""
        if self._table is None:
            n = len(self.ids)
            rows, flags, offsets = np.zeros((n, 4), np.int32), np.zeros(n, np.uint8), np.zeros(n + 1, np.int64)
            iv = np.zeros((self.counts["intervals"] if self.counts else 0, 2), np.int32)   # (without a finish the copy refuses)
            self._ms._chk(self._lib.mhap_repeat_copy(self._s, _opt(rows), _opt(flags), _ptr(offsets), _opt(iv)))
            self._table = (rows, flags, offsets, iv)
        return self._table

    def histogram(self):
        """The REPEAT_BINS bins of the last finish (int64): positions by depth, the last bin holding every greater depth."""
        bins = np.zeros(REPEAT_BINS, np.int64)
        self._ms._chk(self._lib.mhap_repeat_histogram(self._s, _ptr(bins)))
        return bins

    def apply(self, records):
        """(keep, unique): one byte per record, 0 for a void one, and int32 (n, 2) of uA, uB (-1, -1 for an ineligible record)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        keep, unique = np.zeros(len(records), np.uint8), np.zeros((len(records), 2), np.int32)
        self._ms._chk(self._lib.mhap_repeat_apply(self._s, _opt(records), C.c_int64(len(records)), _opt(keep), _opt(unique)))
        return keep, unique


VARIANT_COUNTS = ("reads", "reads_with_site", "sites", "deep_positions", "bases", "accepted_views", "skipped_views")   # mhap_variant_finish's counts
VARIANT_SITE_FIELDS = ("pos", "major", "minor", "n_major", "n_minor", "depth")
VARIANT_TALLIES = ("informative", "agree", "disagree", "other")
VARIANT_COUNTERS = 6   # per position: base A C G T, del, span
VARIANT_TILE = 1024    # MHAP_VARIANT_TILE: the positions the site kernel takes at a time
VARIANT_DEFAULTS = dict(min_depth=8, min_minor=3, min_pct=25, max_del_pct=25, min_diff=2, diff_pct=50)   # provisional (EXPERIMENTS.md, "Variant filter")


class _VariantParams(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("min_depth", "min_minor", "min_pct", "max_del_pct", "min_diff", "diff_pct")]


def variant_counts_line(counts, set_aside, judged):
    """The one stderr line of a variant filter (the driver prints the same); counts: the MHAP_VARIANT_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Variant sites: {c[0]} reads, {c[1]} with a site; {c[2]} sites, {c[3]} of {c[4]} positions deep; {c[5]} views, "
            f"skipped_views = {c[6]}; {int(set_aside)} of {int(judged)} overlaps set aside")


class VariantSession(_Session):
    """Variant sites from the pile-up votes and the overlaps judged across them (mhap_variant_begin / _add / _votes / _finish / _copy /
    _apply; the contract is the "variant sites" section of include/mhap_hip.h).  The vote table (12 bytes per base) and the site
    bytes stay on the device from begin to close.

        with VariantSession(fasta, min_depth=8, ...) as vs:
            vs.add(records, op_offsets, ops)              # what realign_records_paths returned; any number of times
            counts = vs.finish()                          # a dict of VARIANT_COUNTS
            rows, offsets, sites = vs.table()             # read r's sites: sites[offsets[r]:offsets[r + 1]], VARIANT_SITE_FIELDS
            keep, tallies = vs.apply(records, op_offsets, ops)   # records[keep != 0] stay; tallies: int32 (n, 4) of VARIANT_TALLIES

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix = "mhap_variant"
    _table = counts = None

    def __init__(self, fasta, query_fasta=None, handle=None, device=0, **params):
        unknown = set(params) - set(VARIANT_DEFAULTS)
        if unknown:
            raise MhapError(f"VariantSession: no parameter {sorted(unknown)[0]}")
        bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
        self._bases = np.ascontiguousarray(bases, np.uint8)
        self.ids, self._offsets = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(offsets, np.int64)
        self.lengths = np.ascontiguousarray(lengths, np.int32)
        self.params = dict(VARIANT_DEFAULTS, **params)
        p = _VariantParams(**{k: int(x) for k, x in self.params.items()})
        begin = lambda: self._lib.mhap_variant_begin(   # noqa: E731
            self._ms._h, _ptr(self._bases), len(self._bases), _ptr(self.ids), _ptr(self._offsets), _ptr(self.lengths), len(self.ids),
            C.byref(p), C.byref(self._s))
        super().__init__(handle, device, lambda: self._ms._chk(begin()))

    def _with_paths(self, who, records, op_offsets, ops, call):
        """call(records, n, paths object) with the runs as a paths object, freed afterwards."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        op_offsets = np.ascontiguousarray(op_offsets, dtype=np.int64)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        if len(op_offsets) != len(records) + 1:
            raise MhapError(f"VariantSession.{who}: {len(records)} records need {len(records) + 1} run offsets, not {len(op_offsets)}")
        obj = C.c_void_p()
        if self._lib.mhap_align_paths_from_runs(_ptr(op_offsets), C.c_int64(len(records)), _opt(ops), C.byref(obj)) != 0:
            raise MhapError(f"VariantSession.{who}: op_offsets is not a list of run offsets over ops")
        try:
            return call(records, obj)
        finally:
            self._lib.mhap_align_paths_free(obj)

    def add(self, records, op_offsets, ops):
        """The votes of realigned records and their runs (pair q's are ops[op_offsets[q]:op_offsets[q + 1]])."""
        self._with_paths("add", records, op_offsets, ops,
                         lambda recs, obj: self._ms._chk(self._lib.mhap_variant_add(self._s, _opt(recs), C.c_int64(len(recs)), obj)))

    def finish(self):
        """Make the site bytes, the rows and the site list; returns a dict of VARIANT_COUNTS."""
        self._table = self.counts = None
        counts = np.zeros(len(VARIANT_COUNTS), np.int64)
        self._ms._chk(self._lib.mhap_variant_finish(self._s, _ptr(counts)))
        self.counts = dict(zip(VARIANT_COUNTS, counts.tolist()))
        return self.counts

    def table(self):
        """(rows, offsets, sites) of the last finish: int32 (n, 2) of n_sites and n_deep, int64 (n + 1) and int32 (sites, 6) of
        VARIANT_SITE_FIELDS."""
        if self._table is None:
            n = len(self.ids)
            rows, offsets = np.zeros((n, 2), np.int32), np.zeros(n + 1, np.int64)
            sites = np.zeros((self.counts["sites"] if self.counts else 0, 6), np.int32)   # (without a finish the copy refuses)
            self._ms._chk(self._lib.mhap_variant_copy(self._s, _opt(rows), _ptr(offsets), _opt(sites)))
            self._table = (rows, offsets, sites)
        return self._table

    def votes(self, read_index):
        """The raw counters of one read: a uint16 array (length, VARIANT_COUNTERS)."""
        if not 0 <= read_index < len(self.ids):
            raise MhapError(f"VariantSession.votes: read {read_index} is not among the {len(self.ids)} reads")
        out = np.zeros((int(self.lengths[read_index]), VARIANT_COUNTERS), np.uint16)
        self._ms._chk(self._lib.mhap_variant_votes(self._s, C.c_int64(read_index), _opt(out)))
        return out

    def apply(self, records, op_offsets, ops):
        """(keep, tallies): one byte per record, 0 for one that is set aside, and int32 (n, 4) of VARIANT_TALLIES."""
        def call(recs, obj):
            keep, tallies = np.zeros(len(recs), np.uint8), np.zeros((len(recs), 4), np.int32)
            self._ms._chk(self._lib.mhap_variant_apply(self._s, _opt(recs), C.c_int64(len(recs)), obj, _opt(keep), _opt(tallies)))
            return keep, tallies
        return self._with_paths("apply", records, op_offsets, ops, call)


SELECT_COUNTS = ("reads", "reads_with_entry", "reads_over", "entries", "kept", "eligible_records")   # mhap_select_finish's counts
SELECT_ROW_FIELDS = ("entries", "kept", "threshold", "max_key")
SELECT_A, SELECT_B = 1, 2   # the bits of a record's view byte
SELECT_LDS_KEYS = 8192   # MHAP_SELECT_LDS_KEYS: the longest segment of keys that stays in LDS across the passes of the select
SELECT_DEFAULTS = dict(best_n=40, min_span=500, min_identity=0.0)   # choices, not measurements


class _SelectParams(C.Structure):
    _fields_ = [("best_n", C.c_int32), ("min_span", C.c_int32), ("min_identity", C.c_double)]


def select_counts_line(counts):
    """The one stderr line of an overlap selection (the driver prints the same); counts: the MHAP_SELECT_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Best overlaps: {c[0]} reads, {c[1]} with a view, {c[2]} cut; {c[4]} of {c[3]} views kept; {c[5]} eligible overlaps")


def select_table_text(read_ids, rows):
    """The table file of a selection: one line per read, `read_id entries kept threshold`."""
    return "".join(f"{i} {r[0]} {r[1]} {r[2]}\n" for i, r in zip(np.asarray(read_ids).tolist(), np.asarray(rows).tolist()))


def select_judge_record(record, best_n=40, min_span=500, min_identity=0.0):
    """The keys of one record's two views (mhap_select_judge_record, no GPU): (eligible, kA, kB), a key of 0 for no such view."""
    lib = load_library()
    rec = np.ascontiguousarray(record, dtype=RECORD_DTYPE).reshape(1)
    keys = np.zeros(2, np.uint32)
    p = _SelectParams(best_n, min_span, min_identity)
    rc = lib.mhap_select_judge_record(_ptr(rec), C.byref(p), _ptr(keys))
    if rc < 0:
        raise MhapError("mhap_select_judge_record: bad parameters or an eligible record outside its reads")
    return bool(rc), int(keys[0]), int(keys[1])


class SelectSession(_ReadsSession):
    """Each read's best overlaps (mhap_select_begin / _add / _finish / _copy / _apply; the contract is the "overlap selection" section
    of include/mhap_hip.h).

        with SelectSession(fasta.ids, fasta.lengths, best_n=40) as ss:
            ss.add(records)                       # realigned records; any number of times
            rows, counts = ss.finish()            # int32 (n, 4) of SELECT_ROW_FIELDS and a dict of SELECT_COUNTS
            views = ss.apply(records)             # one byte per record: SELECT_A | SELECT_B

    handle: a MinHashSearch whose device and stream to use (else one is made and closed with the session)."""

    _prefix, _counts = "mhap_select", SELECT_COUNTS
    rows = counts = None

    def __init__(self, read_ids, lengths, best_n=40, min_span=500, min_identity=0.0, handle=None, device=0):
        super().__init__(read_ids, lengths, _SelectParams(best_n, min_span, min_identity), handle, device)

    def finish(self):
        """Make every read's threshold: (rows, counts), int32 (n, 4) of SELECT_ROW_FIELDS and a dict of SELECT_COUNTS."""
        self.rows = self.counts = None
        counts = self._finish()
        rows = np.zeros((len(self.ids), 4), np.int32)
        self._ms._chk(self._lib.mhap_select_copy(self._s, _opt(rows)))
        self.rows, self.counts = rows, counts
        return self.rows, self.counts

    def apply(self, records):
        """One byte per record against the thresholds of the last finish: bit 0 SELECT_A (view A kept), bit 1 SELECT_B."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        views = np.zeros(len(records), np.uint8)
        self._ms._chk(self._lib.mhap_select_apply(self._s, _opt(records), C.c_int64(len(records)), _opt(views)))
        return views


def select_overlaps(records, fasta, best_n=40, min_span=500, min_identity=0.0, query_fasta=None, handle=None, device=0):
    """Select over the realigned `records` of the reads of `fasta` (and `query_fasta`): (views, rows, counts, ids) — one byte per
    record, SelectSession.finish's rows and counts, and the ids the rows belong to."""
    _, ids, _, lengths = _all_reads(fasta, query_fasta)
    with SelectSession(ids, lengths, best_n=best_n, min_span=min_span, min_identity=min_identity, handle=handle, device=device) as ss:
        ss.add(records)
        rows, counts = ss.finish()
        return ss.apply(records), rows, counts, np.asarray(ids, np.int64)


CONSENSUS_COUNTS = ("members", "placed_by_record", "unplaced", "aligned", "no_alignment", "bases_in", "bases_out", "substitutions",
                    "deletions", "insertions", "low")   # mhap_consensus_run's counts, in order
CONSENSUS_STATS = ("len_in", "len_out", "n_sub", "n_del", "n_ins", "n_low")
CONSENSUS_PLACEMENT_FIELDS = ("unitig", "strand", "p", "how", "aligned")   # how: 0 member, 1 record, 2 unplaced
CONSENSUS_TILE = 4096


class _ConsensusParams(C.Structure):
    _fields_ = [("band", C.c_int32), ("min_cov", C.c_int32)]


def consensus_counts_line(counts):
    """The one stderr line of a unitig consensus (the driver prints the same); counts: the MHAP_CONSENSUS_COUNTS values in order."""
    c = [int(x) for x in counts]
    return (f"Consensus: {c[0]} members, {c[1]} reads placed by an overlap, {c[2]} unplaced; {c[3]} aligned, {c[4]} without alignment; "
            f"{c[5]} bases in, {c[6]} out: {c[7]} substitutions, {c[8]} deletions, {c[9]} insertions, {c[10]} low positions")


def format_consensus_gfa(read_ids, unitigs, sequences, position_maps):
    """The GFA 1 text of the unitig graph with consensus: format_unitig_gfa's, except that the S lines carry the consensus sequence
    and LN:i: its length, and the offset of every `a` line goes through the unitig's position map (position_maps[k][offset]).
    sequences: the consensus bytes per unitig; position_maps: one int64 array per unitig, ulen[k] long."""
    ids = np.asarray(read_ids).tolist()
    start, circ = unitigs["unitig_start"].tolist(), unitigs["circular"].tolist()
    vertex, offset, span = unitigs["vertex"].tolist(), unitigs["offset"].tolist(), unitigs["span"].tolist()
    out = ["H\tVN:Z:1.0\n"]
    for k, seq in enumerate(sequences):
        name = f"utg{k + 1:06d}{'c' if circ[k] else 'l'}"
        out.append(f"S\t{name}\t{seq.decode('latin-1')}\tLN:i:{len(seq)}\tnr:i:{start[k + 1] - start[k]}\n")
        out += [f"a\t{name}\t{int(position_maps[k][offset[m]])}\t{ids[vertex[m] >> 1]}:1-{span[m]}\t{'-' if vertex[m] & 1 else '+'}\t{span[m]}\n"
                for m in range(start[k], start[k + 1])]
    out += [format_gfa_unitig_link(r) + "\n" for r in np.ascontiguousarray(unitigs["links"], dtype=np.int32).reshape(-1, 6)]
    return "".join(out)


class ConsensusSession(_Session):
    """The consensus of the unitigs a GraphSession serves (mhap_consensus_begin / _add / _run / _copy*; the contract is the "unitig
    consensus" section of include/mhap_hip.h): every read is placed on a unitig — members exactly, the others through their best
    overlap with a member — aligned to the draft, and every draft position takes the majority of the pile.

        gs.unitigs()                                  # or gs.clean()
        with ConsensusSession(gs, fasta) as cs:
            cs.add(records)                           # the records the graph was given; any number of times
            counts = cs.run()                         # a dict of CONSENSUS_COUNTS
            seqs = cs.sequences()                     # the consensus bytes per unitig; cs.stats is int64 (n, 6) of CONSENSUS_STATS
            text = cs.gfa()                           # the unitig GFA with consensus

    A later finish(), unitigs() or clean() of the graph session invalidates this one."""

    _prefix = "mhap_consensus"

    def __init__(self, graph_session, fasta, band=0, min_cov=4, query_fasta=None, qualities=None, weights=None):
        """qualities, weights: as CorrectSession's (mhap_consensus_begin_weighted)."""
        self._gs = graph_session
        bases, ids, offsets, lengths = _all_reads(fasta, query_fasta)
        if len(ids) != len(graph_session.ids):
            raise MhapError(f"ConsensusSession: {len(ids)} reads for a graph of {len(graph_session.ids)}")
        self._bases = np.ascontiguousarray(bases, np.uint8)
        self._offsets = np.ascontiguousarray(offsets, np.int64)
        self._quals, self.weights = _weighted_args(self._bases, qualities, weights)
        p = _ConsensusParams(band, min_cov)
        if self._quals is None:
            begin = lambda: self._lib.mhap_consensus_begin(   # noqa: E731
                graph_session._s, _opt(self._bases), len(self._bases), _opt(self._offsets), C.byref(p), C.byref(self._s))
        else:
            begin = lambda: self._lib.mhap_consensus_begin_weighted(   # noqa: E731
                graph_session._s, _opt(self._bases), _ptr(self._quals if len(self._quals) else np.zeros(1, np.uint8)), len(self._bases),
                _opt(self._offsets), C.byref(p), C.byref(self.weights), C.byref(self._s))
        super().__init__(graph_session._ms, None, lambda: self._ms._chk(begin()))   # (the graph session's handle)

    def add(self, records):
        """The realigned records the graph was given (they stay on the device, 32 bytes each)."""
        records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        self._ms._chk(self._lib.mhap_consensus_add(self._s, _opt(records), C.c_int64(len(records))))

    def run(self):
        """Place, align, vote and call: a dict of CONSENSUS_COUNTS.  Afterwards `bytes`, `out_offsets` (n + 1), `stats` (n, 6)."""
        counts = np.zeros(len(CONSENSUS_COUNTS), np.int64)
        self._ms._chk(self._lib.mhap_consensus_run(self._s, _ptr(counts)))
        n, _, _, nout = self.info()
        self.out_offsets, self.stats, self.bytes = np.zeros(n + 1, np.int64), np.zeros((n, 6), np.int64), np.zeros(nout, np.uint8)
        self._ms._chk(self._lib.mhap_consensus_copy(self._s, _ptr(self.bytes) if nout else None, _ptr(self.out_offsets), _ptr(self.stats) if n else None))
        self.counts = dict(zip(CONSENSUS_COUNTS, counts.tolist()))
        return self.counts

    def info(self):
        """(unitigs of the last run or -1, reads, draft bases, consensus bytes)."""
        v = [C.c_int64(0) for _ in range(4)]
        self._ms._chk(self._lib.mhap_consensus_info(self._s, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def sequences(self):
        """The consensus of every unitig of the last run, a list of bytes."""
        n, _, _, nout = self.info()
        off, raw = np.zeros(n + 1, np.int64), np.zeros(nout, np.uint8)
        stats = np.zeros((max(n, 0), 6), np.int64)
        self._ms._chk(self._lib.mhap_consensus_copy(self._s, _ptr(raw) if nout else None, _ptr(off), _ptr(stats) if n > 0 else None))
        raw = raw.tobytes()
        return [raw[int(off[k]):int(off[k + 1])] for k in range(n)]

    def placements(self):
        """The placement table: int64 (reads, 5) of CONSENSUS_PLACEMENT_FIELDS."""
        out = np.zeros((self.info()[1], 5), np.int64)
        self._ms._chk(self._lib.mhap_consensus_copy_placements(self._s, _opt(out)))
        return out

    def position_maps(self):
        """Per unitig an int64 array over its draft positions: the consensus bytes before what the position emits."""
        n, _, nd, _ = self.info()
        out = np.zeros(nd, np.int64)
        self._ms._chk(self._lib.mhap_consensus_copy_map(self._s, _ptr(out) if nd else None))
        ends = np.cumsum(self.stats[:, 0]).tolist() if n > 0 else []
        return [out[e - int(ln):e] for e, ln in zip(ends, self.stats[:, 0].tolist())]

    def votes(self, k):
        """The raw counters of unitig k: a uint16 array (draft length, CORRECT_COUNTERS).  Tests only."""
        n = self.info()[0]
        if not 0 <= k < n:
            raise MhapError(f"ConsensusSession.votes: unitig {k} is not among the {n} unitigs")
        out = np.zeros((int(self.stats[k, 0]), CORRECT_COUNTERS), np.uint16)
        self._ms._chk(self._lib.mhap_consensus_votes(self._s, C.c_int64(k), _opt(out)))
        return out

    def quality(self, per_vote=15, cap=60):
        """(quals, hist) of the last run (mhap_consensus_quality; "base qualities" in include/mhap_hip.h): a uint8 array per unitig,
        as long as its consensus, and the int64 histogram of QUALITY_BINS bins over all of them."""
        n = self.info()[0]
        off = self.out_offsets if n >= 0 and hasattr(self, "out_offsets") else np.zeros(1, np.int64)   # (no run: the library refuses)
        return _qualities(self._ms, self._lib.mhap_consensus_quality, self._s, QualityParams(per_vote, cap), off)

    def times(self):
        """The host's wall time of the last run's stages in seconds: a dict of placement, alignment, vote, call."""
        out = np.zeros(4, np.float64)
        self._ms._chk(self._lib.mhap_consensus_times(self._s, _ptr(out)))
        return dict(zip(("placement", "alignment", "vote", "call"), out.tolist()))

    def gfa(self):
        """The GFA 1 text of the unitig graph with consensus, from the unitigs the graph session serves (format_consensus_gfa)."""
        u = self._gs.unitigs_table
        if u is None:
            raise MhapError("ConsensusSession.gfa: the graph session has no unitigs() or clean() since its last finish()")
        return format_consensus_gfa(self._gs.ids, u, self.sequences(), self.position_maps())

    def close(self):
        if not self._gs._s:   # (the graph session's handle may be gone with it: nothing is left to free through)
            self._s = C.c_void_p()
        super().close()


def string_graph(records, fasta, query_fasta=None, handle=None, device=0, **params):
    """The string graph of realigned records over the reads of `fasta` (and `query_fasta`): (arcs, counts, contained, gfa text) of a
    GraphSession; params: max_hang, int_frac_permille, min_ovlp, fuzz, min_identity."""
    _, ids, _, lengths = _all_reads(fasta, query_fasta)
    with GraphSession(ids, lengths, handle=handle, device=device, **params) as gs:
        gs.add(records)
        arcs, counts = gs.finish()
        return arcs, counts, gs.contained(), gs.gfa()


def unitigs(records, fasta, query_fasta=None, handle=None, device=0, **params):
    """The unitigs of the string graph of realigned records over the reads of `fasta` (and `query_fasta`): (the dict of
    GraphSession.unitigs(), the sequences as a list of bytes, the GFA text of the unitig graph); params as string_graph's."""
    _, ids, _, lengths = _all_reads(fasta, query_fasta)
    with GraphSession(ids, lengths, handle=handle, device=device, **params) as gs:
        gs.add(records)
        gs.finish()
        u = gs.unitigs()
        seqs = gs.unitig_sequences(fasta, query_fasta)
        return u, seqs, format_unitig_gfa(ids, u, seqs)


def _skip_bytes(skip, k):
    """skip k-mers (str or bytes) -> (uint8 array of the length-k ones back to back or None, their count)."""
    sk = [x.encode("latin-1") if isinstance(x, str) else bytes(x) for x in skip]
    sk = b"".join(x for x in sk if len(x) == k)
    return (np.frombuffer(sk, dtype=np.uint8) if sk else None), len(sk) // k


class KsimDevice:
    """A KmerStatSimulator session on one device (mhap_ksim_dev_*): device buffers kept across its calls."""

    def __init__(self, device=0, handle=None):
        self._own = handle is None
        self.ms = MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) if self._own else handle
        self._lib = self.ms._lib
        self.d = self._lib.mhap_ksim_dev_create(self.ms._h)
        if not self.d:
            err = self.ms._lib.mhap_last_error(self.ms._h)
            self.close()
            raise MhapError(err.decode() if err else "mhap_ksim_dev_create failed")

    def pair_stats(self, bases, pairs, k, bottom_k=1256, skip=(), paths=False):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 4))
        out = np.zeros((len(pairs), 3), dtype=np.int32)
        pth = np.zeros(len(pairs), dtype=np.int32)
        if len(pairs):
            skb, ns = _skip_bytes(skip, k)
            self.ms._chk(self._lib.mhap_ksim_dev_pair_stats(self.d, _ptr(bases), len(bases), _ptr(pairs), len(pairs), k, bottom_k, _ptr(skb),
                                                            ns, _ptr(out), _ptr(pth)))
        return (out, pth) if paths else out

    def trials(self, seed, trial0, n, L, offset, err, pi, pd, ps, flags, ref, k, bottom_k, skip, want_reads=False):
        """mhap_ksim_dev_trials: (stats (n, 2, 3) or None, reads (n, roles, L) or None, meta (n, 5), events (n, roles, 4))."""
        roles = 1 if flags & 2 else 3
        stats = None if flags & 2 else np.zeros((n, 2, 3), dtype=np.int32)
        reads = np.zeros((n, roles, L), dtype=np.uint8) if want_reads else None
        meta = np.zeros((n, 5), dtype=np.int32)
        events = np.zeros((n, roles, 4), dtype=np.int32)
        b, off, ln = ref
        skb, ns = _skip_bytes(skip, k) if k >= 1 else (None, 0)
        failed = C.c_int64(-1)
        rc = self._lib.mhap_ksim_dev_trials(self.d, seed, trial0, n, L, offset, err, pi, pd, ps, flags, _ptr(b), _ptr(off), _ptr(ln),
                                            0 if off is None else len(off), max(k, 1), bottom_k, _ptr(skb), ns, _ptr(stats), _ptr(reads),
                                            _ptr(meta), _ptr(events), C.byref(failed))
        if rc != 0:
            msg = self._lib.mhap_last_error(self.ms._h)
            raise MhapError((msg.decode() if msg else f"mhap_ksim_dev_trials failed ({rc})"), failed.value)
        return stats, reads, meta, events

    def close(self):
        if getattr(self, "d", None):
            self._lib.mhap_ksim_dev_destroy(self.d)
            self.d = None
        if self._own and self.ms is not None:
            self.ms.close()
            self.ms = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def pair_kmer_stats(bases, pairs, k, bottom_k=1256, skip=(), device=0, handle=None, paths=False):
    """KmerStatSimulator's compareKmers / compareMinHash counts of many segment pairs on the GPU (mhap_pair_kmer_stats; its header comment
    is the contract).  bases: uint8 array; pairs: int64 array (n, 4) of (a_off, a_len, b_off, b_len); skip: k-mers (str or bytes) left
    out of `shared` (entries whose length is not k never match).  Returns an int32 array (n, 3) of (shared, total, intersect), and with
    paths=True also the scratch each pair took on the device (1 = LDS, 2 = HBM).  handle: a MinHashSearch or a KsimDevice to use."""
    if isinstance(handle, KsimDevice):
        return handle.pair_stats(bases, pairs, k, bottom_k, skip, paths)
    with KsimDevice(device, handle) as d:
        return d.pair_stats(bases, pairs, k, bottom_k, skip, paths)


class FrequencyCounts:
    """Parsed `-f` filter file (J/sketch/FrequencyCounts.java:63-229): k-mer hash -> fraction (+ the --supress-noise whitelist)."""

    def __init__(self, hashes, fractions, filter_cutoff=1.0e-5, offset=0.0, repeat_idf_scale=3.0, no_tf=False, supress_noise=0,
                 whitelist=None, size_bloom=None):
        self.hashes = np.ascontiguousarray(hashes, dtype=np.int64)
        self.fractions = np.ascontiguousarray(fractions, dtype=np.float64)
        self.filter_cutoff = filter_cutoff
        self.offset = offset
        self.range = repeat_idf_scale
        self.no_tf = no_tf
        self.supress_noise = supress_noise            # removeUnique: 1 drop k-mers absent from the file, 2 give them idf 1
        self.whitelist = np.ascontiguousarray(whitelist if whitelist is not None else self.hashes, dtype=np.int64)
        # first number of the file's first line; only an object built WITHOUT a file falls back to the whitelist length
        self.size_bloom = max(1, len(self.whitelist)) if size_bloom is None else (1 if size_bloom == 0 else int(size_bloom))

    @classmethod
    def from_file(cls, path, filter_cutoff=1.0e-5, repeat_weight=0.9, repeat_idf_scale=3.0, no_tf=False, do_rc=True,
                  supress_noise=0):
        """The parser of mhap_set_filter_file (host_util.cpp), line for line: header "sizeBloom sizeRepeat" (both >= 0; a sizeBloom
        of 0 counts as 1, FrequencyCounts.java:102-121), then `kmer [fraction [ignored]]`; a malformed fraction drops the whole line."""
        lib = load_library()
        offset = repeat_weight if 0.0 <= repeat_weight < 1.0 else 0.0   # MhapMain.java:346-350
        hs, fr, allh = [], [], []
        out = C.c_int64()
        with open(path, "r") as fh:
            first = fh.readline().split()
            try:
                size_bloom, size_repeat = int(first[0]), int(first[1])
            except (IndexError, ValueError):
                raise MhapError("K-mer filter file first line must contain estimated number of k-mers in the file (long).")
            if size_bloom < 0 or size_repeat < 0:
                raise MhapError("K-mer filter file first line must contain estimated number of k-mers in the file (long).")
            for line in fh:
                parts = line.split(None, 2)
                if len(parts) < 1:
                    continue
                kmer = parts[0].encode("latin-1")
                if lib.mhap_hash_kmer(kmer, C.c_int32(len(kmer)), C.c_int32(1 if do_rc else 0), C.byref(out)) != 0:
                    continue
                frac = None
                if len(parts) >= 2:
                    try:
                        frac = float(parts[1])
                    except ValueError:
                        continue
                allh.append(out.value)
                if frac is not None:
                    hs.append(out.value)
                    fr.append(frac)
        return cls(np.array(hs, dtype=np.int64), np.array(fr, dtype=np.float64), filter_cutoff, offset,
                   repeat_idf_scale, no_tf, supress_noise, np.array(allh, dtype=np.int64), size_bloom)


    @classmethod
    def from_counts(cls, kc, filter_cutoff=1.0e-5, repeat_weight=0.9, repeat_idf_scale=3.0, no_tf=False, do_rc=True, supress_noise=0):
        """The filter that from_file gives on the file kc.write() writes, without the file: the same hashes, the fractions as the
        file's `%.10e` text parses back, the whitelist and size_bloom = kc.distinct (the header's first number)."""
        lib = load_library()
        offset = repeat_weight if 0.0 <= repeat_weight < 1.0 else 0.0   # MhapMain.java:346-350
        out = C.c_int64()
        hs = np.zeros(len(kc.kmers), dtype=np.int64)
        for i, s in enumerate(kc.kmer_strings()):
            b = s.encode("latin-1")
            if lib.mhap_hash_kmer(b, C.c_int32(len(b)), C.c_int32(1 if do_rc else 0), C.byref(out)) != 0:
                raise MhapError(f"mhap_hash_kmer failed on {s}")
            hs[i] = out.value
        fr = np.array([float(f"{x:.10e}") for x in kc.fractions.tolist()], dtype=np.float64)
        return cls(hs, fr, filter_cutoff, offset, repeat_idf_scale, no_tf, supress_noise, hs.copy(), kc.distinct)


class FastaScan:
    """A FASTA file mapped and scanned, not copied (mhap_fasta_scan_*): ids, lengths and names of its records; the index is fed from
    the mapped text in groups, host threads packing one group while the GPU sketches the previous one (MinHashSearch.add_scan)."""

    def __init__(self, path, id_offset=0):
        self._lib = load_library()
        self._s = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self._lib.mhap_fasta_scan_open(path.encode(), C.c_int64(id_offset), C.byref(self._s), err, C.c_size_t(512))
        if rc != 0:
            self._s = C.c_void_p()
            raise MhapError(err.value.decode() or f"mhap_fasta_scan_open failed ({rc})")
        self._lib.mhap_fasta_scan_reads.restype = C.c_int64
        self._lib.mhap_fasta_scan_bases.restype = C.c_int64
        self.n = self._lib.mhap_fasta_scan_reads(self._s)
        self.total_bases = self._lib.mhap_fasta_scan_bases(self._s)
        self.has_qualities = bool(self._lib.mhap_fasta_scan_has_qualities(self._s))   # the file is FASTQ

    def qualities(self):
        """One Phred byte per base, in the reads' order (a FASTQ file only)."""
        if not self.has_qualities:
            raise MhapError("FastaScan.qualities: the file is FASTA and brings no base qualities")
        out = np.zeros(max(self.total_bases, 1), np.uint8)
        if self._lib.mhap_fasta_scan_qualities(self._s, _ptr(out)) != 0:
            raise MhapError("mhap_fasta_scan_qualities failed")
        return out[:self.total_bases]

    def __len__(self):
        return int(self.n)

    def info(self):
        """(ids, lengths, names)"""
        ids = np.zeros(max(self.n, 1), np.int64)
        lens = np.zeros(max(self.n, 1), np.int32)
        hp, hb = C.c_char_p(), C.c_int64()
        rc = self._lib.mhap_fasta_scan_info(self._s, _ptr(ids), _ptr(lens), C.byref(hp), C.byref(hb))
        if rc != 0:
            raise MhapError(f"mhap_fasta_scan_info failed ({rc})")
        raw = C.string_at(hp, hb.value) if hb.value else b""
        names = [x.decode("latin-1") for x in raw.split(b"\0")[:self.n]]
        return ids[:self.n], lens[:self.n], names

    def close(self):
        if getattr(self, "_s", None) and self._s.value:
            self._lib.mhap_fasta_scan_free(self._s)
            self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerCounts:
    """Exact k-mer counts made on the GPU (mhap_kmer_count_*): the lines of the `-f` repeat filter file — k-mers (2 bits per base,
    A=0 C=1 G=2 T=3, first base most significant) whose share of all counted windows is at least the min_fraction they were made
    with, by descending count, then ascending value — and the totals of its header.  `histogram` (when asked for at finish, else
    None): (counts uint32, numbers uint64), for every count that occurs, in ascending order, the number of distinct k-mers counted
    that many times."""

    def __init__(self, lib, ptr):
        self._lib, self._c = lib, ptr
        total, distinct, lines, k = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        lib.mhap_kmer_counts_info(ptr, C.byref(total), C.byref(distinct), C.byref(lines), C.byref(k))
        self.total, self.distinct, self.k = total.value, distinct.value, k.value
        self.kmers = np.zeros(lines.value, dtype=np.uint64)
        self.counts = np.zeros(lines.value, dtype=np.uint64)
        if lines.value:
            lib.mhap_kmer_counts_lines(ptr, _ptr(self.kmers), _ptr(self.counts))
        self.fractions = self.counts.astype(np.float64) / float(max(self.total, 1))
        self.histogram = None
        nh = C.c_int64()
        if lib.mhap_kmer_counts_histogram_size(ptr, C.byref(nh)) == 0:
            hc, hn = np.zeros(nh.value, dtype=np.uint32), np.zeros(nh.value, dtype=np.uint64)
            if nh.value:
                lib.mhap_kmer_counts_histogram(ptr, _ptr(hc), _ptr(hn))
            self.histogram = (hc, hn)

    def __len__(self):
        return int(self.kmers.shape[0])

    def kmer_strings(self):
        if len(self) == 0:
            return []
        shifts = np.uint64(2) * np.arange(self.k - 1, -1, -1, dtype=np.uint64)
        codes = ((self.kmers[:, None] >> shifts[None, :]) & np.uint64(3)).astype(np.uint8)
        chars = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
        return [r.tobytes().decode("latin-1") for r in chars]

    def write(self, path):
        """The `-f` file: "<distinct> <lines>", then "<kmer>\t<fraction %.10e>" per line (mhap_kmer_counts_write)."""
        if not self._c:
            raise MhapError("KmerCounts already freed")
        if self._lib.mhap_kmer_counts_write(self._c, os.fspath(path).encode()) != 0:
            raise MhapError(f"cannot write the k-mer filter file {path}")

    def write_histogram(self, path):
        """The k-mer count histogram: "<count>\t<number>" per line in ascending count (mhap_kmer_counts_write_histogram), the file
        `python -m mhap_amd.histogram_stats` reads."""
        if not self._c:
            raise MhapError("KmerCounts already freed")
        if self.histogram is None:
            raise MhapError("these counts were made without the histogram (kmer_count_finish(..., histogram=True))")
        if self._lib.mhap_kmer_counts_write_histogram(self._c, os.fspath(path).encode()) != 0:
            raise MhapError(f"cannot write the k-mer count histogram {path}")

    def close(self):
        if getattr(self, "_c", None):
            self._lib.mhap_kmer_counts_free(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerSet:
    """The k-mers of a count whose final count is at least `min_count`, as a bitmap of 4^k bits on the device (mhap_kmer_set_*): what
    sequences are assessed against.  total: windows counted; distinct: values seen; members: values in the set; min_count: the
    threshold used (the valley of the count histogram when it was made with min_count=0)."""

    def __init__(self, lib, ptr):
        self._lib, self._s = lib, ptr
        total, distinct, members, k, canonical, mc = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32(), C.c_uint64()
        lib.mhap_kmer_set_info(ptr, C.byref(total), C.byref(distinct), C.byref(members), C.byref(k), C.byref(canonical), C.byref(mc))
        self.total, self.distinct, self.members = total.value, distinct.value, members.value
        self.k, self.canonical, self.min_count = k.value, bool(canonical.value), mc.value

    def close(self):
        if getattr(self, "_s", None):
            self._lib.mhap_kmer_set_free(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerEval:
    """Sequences walked against a KmerSet (mhap_kmer_eval_*).  rows: int64 (sequences, 5) = bases, windows, missing, runs, unsupported;
    intervals: int64 (intervals, 3) = sequence index, begin, end of every maximal stretch of unsupported positions; totals: the
    column sums of the rows; error, qv: mhap_kmer_qv of the totals.  `names` (when the sequences had names) go into the files."""
    COLUMNS = ("bases", "windows", "missing", "runs", "unsupported")

    def __init__(self, lib, ptr, names=None):
        self._lib, self._e, self.names = lib, ptr, names
        n, ni, k = C.c_int64(), C.c_int64(), C.c_int32()
        self.totals = np.zeros(5, dtype=np.int64)
        lib.mhap_kmer_eval_info(ptr, C.byref(n), C.byref(ni), C.byref(k), _ptr(self.totals))
        self.k = k.value
        self.rows = np.zeros((n.value, 5), dtype=np.int64)
        self.intervals = np.zeros((ni.value, 3), dtype=np.int64)
        if n.value:
            lib.mhap_kmer_eval_rows(ptr, _ptr(self.rows))
        if ni.value:
            lib.mhap_kmer_eval_intervals(ptr, _ptr(self.intervals))
        self.error, self.qv = kmer_qv(int(self.totals[1]), int(self.totals[2]), self.k)

    def __len__(self):
        return int(self.rows.shape[0])

    def _names(self):
        if self.names is None:
            return None
        if len(self.names) != len(self):
            raise MhapError(f"{len(self.names)} names for {len(self)} sequences")
        return b"".join(n.encode("latin-1") + b"\0" for n in self.names)

    def write_table(self, path):
        """"name\tbases\twindows\tmissing\truns\tunsupported\terror\tqv" per sequence, then a `total` line (mhap_kmer_eval_write_table)."""
        if not self._e:
            raise MhapError("KmerEval already freed")
        if self._lib.mhap_kmer_eval_write_table(self._e, self._names(), os.fspath(path).encode()) != 0:
            raise MhapError(f"cannot write the assessment table {path}")

    def write_bed(self, path):
        """"name\tbegin\tend" per interval of unsupported positions (mhap_kmer_eval_write_bed)."""
        if not self._e:
            raise MhapError("KmerEval already freed")
        if self._lib.mhap_kmer_eval_write_bed(self._e, self._names(), os.fspath(path).encode()) != 0:
            raise MhapError(f"cannot write the interval file {path}")

    def summary(self, reads_set, own_set=None, both=0):
        """The line both tools print (mhap_kmer_eval_summary)."""
        buf = C.create_string_buffer(1024)
        if self._lib.mhap_kmer_eval_summary(self._e, reads_set._s, own_set._s if own_set is not None else None, C.c_int64(both), buf, C.c_size_t(1024)) != 0:
            raise MhapError("mhap_kmer_eval_summary failed")
        return buf.value.decode()

    def close(self):
        if getattr(self, "_e", None):
            self._lib.mhap_kmer_eval_free(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kmer_histogram_valley(counts, numbers):
    """The smallest c >= 1 with n[c + 1] >= n[c] of a count histogram given as KmerCounts.histogram gives it (mhap_kmer_histogram_valley)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    numbers = np.ascontiguousarray(numbers, dtype=np.uint64)
    if counts.shape != numbers.shape or counts.ndim != 1:
        raise MhapError("counts and numbers must be one-dimensional and of one length")
    out = C.c_uint64()
    if load_library().mhap_kmer_histogram_valley(_opt(counts), _opt(numbers), C.c_int64(len(counts)), C.byref(out)) != 0:
        raise MhapError("the histogram's counts must be ascending and at least 1")
    return out.value


def kmer_qv(windows, missing, k):
    """(error per base, QV) from the missing windows of `windows` valid ones (mhap_kmer_qv): NaN without windows, (0, inf) without missing ones."""
    err, qv = C.c_double(), C.c_double()
    if load_library().mhap_kmer_qv(C.c_int64(windows), C.c_int64(missing), C.c_int32(k), C.byref(err), C.byref(qv)) != 0:
        raise MhapError(f"mhap_kmer_qv: bad arguments (windows {windows}, missing {missing}, k {k})")
    return err.value, qv.value


def count_kmers(source, k=16, canonical=True, min_fraction=2.5e-6, device=0, histogram=False):
    """Count the k-mers (k = 1..16) of a FastaData or a FASTA file (plain, gz or bz2; a path goes through the streamed ingest) on the GPU
    and return the KmerCounts of the `-f` repeat filter file.  Windows with a byte other than A/C/G/T are skipped; only the forward
    strand is read; canonical counts a k-mer together with its reverse complement under the smaller value.  histogram=True also
    keeps the k-mer count histogram (KmerCounts.histogram), made on the GPU in the same pass."""
    with MinHashSearch(MhapParams(num_hashes=1, ordered_sketch_size=1, device=device)) as ms:
        ms.kmer_count_begin(k, canonical)
        if isinstance(source, FastaData):
            ms.kmer_count_add(source)
        else:
            with FastaScan(os.fspath(source)) as scan:
                ms.kmer_count_add_scan(scan)
        return ms.kmer_count_finish(min_fraction, histogram=histogram)


class MatchResult:
    """One overlap record (J/impl/MatchResult.java)."""
    __slots__ = ("from_id", "to_id", "score", "raw", "a1", "a2", "alen", "b1", "b2", "blen", "to_rc")

    def __init__(self, rec):
        for k in self.__slots__:
            setattr(self, k, rec[k].item() if hasattr(rec[k], "item") else rec[k])

    def __str__(self):
        return format_record(self)


def format_record(rec):
    """MatchResult.toString (J/impl/MatchResult.java:98-113) through the library's Java-compatible formatter."""
    lib = load_library()
    arr = np.zeros(1, dtype=RECORD_DTYPE)
    for k in RECORD_DTYPE.names:
        if k != "pad":
            arr[0][k] = rec[k] if not isinstance(rec, MatchResult) else getattr(rec, k)
    buf = C.create_string_buffer(256)
    n = lib.mhap_format_record(_ptr(arr), buf, C.c_size_t(256))
    if n < 0:
        raise MhapError("mhap_format_record failed")
    return buf.value.decode()


def records_to_lines(records):
    lib = load_library()
    records = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
    buf = C.create_string_buffer(256)
    out = []
    base = records.ctypes.data
    for i in range(records.shape[0]):
        lib.mhap_format_record(C.c_void_p(base + i * RECORD_DTYPE.itemsize), buf, C.c_size_t(256))
        out.append(buf.value.decode())
    return out


def _collect_records(call, chk):
    """Run a search entry point with a sink that appends every batch of records to ONE growing array (each record is copied once out
    of the library's buffer; the array doubles when it fills up — a list of per-batch copies concatenated at the end moved every
    record twice, 2 x 1.8 GB a step on one rank's share of BASELINE configs[4]).  The sink is called from a library thread, one batch
    at a time."""
    # (untouched pages of np.empty cost nothing: room for 2^17 records up front saves the first doublings of an ordinary search)
    state = {"buf": np.empty(1 << 17, dtype=RECORD_DTYPE), "n": 0}
    isz = RECORD_DTYPE.itemsize

    def sink(recs, cnt, user):
        n, buf = state["n"], state["buf"]
        need = n + cnt
        if need > buf.shape[0]:
            # grow in place: realloc of a large block is a remap of its pages, not a copy (a fresh array + copy moved gigabytes
            # per doubling on one rank's share of BASELINE configs[4] and made the library's sink thread wait)
            buf.resize(max(need, 2 * buf.shape[0]), refcheck=False)
        # one memmove out of the library's buffer (wrapping the pointer in a NumPy array first cost 1.4 ms per call: C2's 41 915 records)
        C.memmove(buf.ctypes.data + n * isz, recs, cnt * isz)
        state["n"] = need
        return 0

    cb = _SINK(sink)
    chk(call(cb))
    return state["buf"][:state["n"]]


class MinHashSearch:
    """GPU counterpart of J/impl/MinHashSearch.java (+ the drivers of AbstractMatchSearch.java).

    add_data(fasta)            ~ new MinHashSearch(streamer, ...) / addData   (sketch fwd+rc, index)
    find_matches()             ~ AbstractMatchSearch.findMatches()            (self, toSelf=true)
    find_matches_stream(fasta) ~ AbstractMatchSearch.findMatches(streamer)    (-q, toSelf=false)
    """

    def __init__(self, params=None, kmer_filter=None):
        self._lib = load_library()
        self.params = params or MhapParams()
        self._h = C.c_void_p()
        err = C.create_string_buffer(512)
        p = self.params._c()
        rc = self._lib.mhap_create(C.byref(p), C.byref(self._h), err, C.c_size_t(512))
        if rc != 0:
            self._h = C.c_void_p()
            raise MhapError(err.value.decode() or f"mhap_create failed ({rc})")
        if kmer_filter is not None:
            self.set_filter(kmer_filter)

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mhap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise MhapError(f"{self._lib.mhap_last_error(self._h).decode()} (code {rc})")

    # -- configuration --------------------------------------------------------------------------
    def set_filter(self, fc):
        hashes, fractions = fc.hashes, fc.fractions
        if len(hashes) == 0:      # a filter whose table is empty is still a filter (every k-mer gets idf = range): non-NULL pointers say so
            hashes, fractions = np.zeros(1, np.int64), np.zeros(1, np.float64)
        self._chk(self._lib.mhap_set_filter(self._h, _ptr(hashes), _ptr(fractions), C.c_int64(len(fc.hashes)),
                                            C.c_double(fc.filter_cutoff), C.c_double(fc.offset), C.c_double(fc.range),
                                            C.c_int(1 if fc.no_tf else 0)))
        if getattr(fc, "supress_noise", 0):
            self._chk(self._lib.mhap_set_filter_whitelist(self._h, _ptr(fc.whitelist), C.c_int64(len(fc.whitelist)),
                                                          C.c_int64(fc.size_bloom), C.c_int32(fc.supress_noise)))

    def set_stream(self, hip_stream_ptr):
        self._chk(self._lib.mhap_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    # -- k-mer counting (the -f filter file) -----------------------------------------------------
    def kmer_count_begin(self, k=16, canonical=True):
        self._chk(self._lib.mhap_kmer_count_begin(self._h, C.c_int32(k), C.c_int32(1 if canonical else 0)))

    def kmer_count_add(self, fasta):
        self._chk(self._lib.mhap_kmer_count_add_reads(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                                      C.c_int64(len(fasta))))

    def kmer_count_add_scan(self, scan):
        self._chk(self._lib.mhap_kmer_count_add_scan(self._h, scan._s))

    def kmer_count_finish(self, min_fraction=2.5e-6, histogram=False, keep_open=False):
        out = C.c_void_p()
        if histogram or keep_open:
            flags = (MHAP_KMER_HISTOGRAM if histogram else 0) | (MHAP_KMER_KEEP_OPEN if keep_open else 0)
            self._chk(self._lib.mhap_kmer_count_finish_flags(self._h, C.c_double(min_fraction), C.c_uint32(flags), C.byref(out)))
        else:
            self._chk(self._lib.mhap_kmer_count_finish(self._h, C.c_double(min_fraction), C.byref(out)))
        return KmerCounts(self._lib, out)

    # -- sequence assessment (mhap_amd.kmer_qv) ------------------------------------------------
    def kmer_count_finish_set(self, min_count=0):
        """End the open count as a KmerSet of the k-mers counted at least min_count times (0: the valley of the count histogram)."""
        out = C.c_void_p()
        self._chk(self._lib.mhap_kmer_count_finish_set(self._h, C.c_uint64(min_count), C.byref(out)))
        return KmerSet(self._lib, out)

    def kmer_set_contains(self, kset, values):
        values = np.ascontiguousarray(values, dtype=np.uint64)
        out = np.zeros(len(values), dtype=np.uint8)
        self._chk(self._lib.mhap_kmer_set_contains(self._h, kset._s, _opt(values), C.c_int64(len(values)), _opt(out)))
        return out

    def kmer_set_eval(self, kset, source):
        """The sequences of a FastaData (bytes as they are) or of a FastaScan (through the streamed ingest) against the set: a KmerEval."""
        out = C.c_void_p()
        if isinstance(source, FastaScan):
            self._chk(self._lib.mhap_kmer_eval_scan(self._h, kset._s, source._s, C.byref(out)))
            return KmerEval(self._lib, out, source.info()[2])
        self._chk(self._lib.mhap_kmer_eval_reads(self._h, kset._s, _ptr(source.bases), _ptr(source.offsets), _ptr(source.lengths),
                                                 C.c_int64(len(source)), C.byref(out)))
        return KmerEval(self._lib, out, getattr(source, "names", None))

    def kmer_set_compare(self, a, b):
        """(members of a, members of b, members of both); sets that differ in k or canonical are refused."""
        na, nb, both = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._lib.mhap_kmer_set_compare(self._h, a._s, b._s, C.byref(na), C.byref(nb), C.byref(both)))
        return na.value, nb.value, both.value

    # -- index ----------------------------------------------------------------------------------
    def add_data(self, fasta):
        self._chk(self._lib.mhap_index_add_reads(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                                 _ptr(fasta.ids), C.c_int64(len(fasta))))

    def add_scan(self, scan):
        """Streamed ingest of a scanned FASTA file (mhap_index_add_scan): parse, pack, upload and sketch overlap."""
        self._chk(self._lib.mhap_index_add_scan(self._h, scan._s))

    def reserve(self, total_reads):
        """The reads an empty index is about to receive over several add_data calls (mhap_index_reserve)."""
        self._chk(self._lib.mhap_index_reserve(self._h, C.c_int64(total_reads)))

    def find_matches_scan(self, scan):
        """-q mode with the query reads of a scanned file."""
        return self._collect(lambda cb: self._lib.mhap_find_matches_scan(self._h, scan._s, cb, None))

    def stage(self, fasta):
        """Pack + upload reads so that they are resident in HBM (bench: outside the timed region)."""
        self._chk(self._lib.mhap_stage_reads(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                             _ptr(fasta.ids), C.c_int64(len(fasta))))

    def add_staged(self):
        self._chk(self._lib.mhap_index_add_staged(self._h))

    def sketch_staged_device(self, d_minhash_ptr, d_ordered_ptr, d_meta_ptr):
        self._chk(self._lib.mhap_sketch_staged_device(self._h, C.c_void_p(d_minhash_ptr), C.c_void_p(d_ordered_ptr),
                                                      C.c_void_p(d_meta_ptr)))

    def size(self):
        n = C.c_int64()
        self._chk(self._lib.mhap_index_size(self._h, C.byref(n)))
        return n.value

    def clear(self):
        self._chk(self._lib.mhap_index_clear(self._h))

    def sketch(self, fasta):
        """SequenceSketchStreamer.getSketch for a batch: returns dict of host arrays (both strands)."""
        n = len(fasta)
        H, S = max(1, self.params.num_hashes), self.params.ordered_sketch_size
        mh = np.zeros((2 * n, H), dtype=np.int32)
        od = np.zeros((2 * n, S, 2), dtype=np.int32)
        osz = np.zeros(2 * n, dtype=np.int32)
        st = np.zeros(2 * n, dtype=np.uint8)
        self._chk(self._lib.mhap_sketch_batch(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                              C.c_int64(n), _ptr(mh), _ptr(od), _ptr(osz), _ptr(st)))
        return {"minhash": mh, "ordered": od, "ordered_size": osz, "status": st}

    def export(self, first=0, count=None):
        total = self.size()
        count = total - first if count is None else count
        H, S = max(1, self.params.num_hashes), self.params.ordered_sketch_size
        out = {"ids": np.zeros(count, np.int64), "is_fwd": np.zeros(count, np.uint8), "seq_length": np.zeros(count, np.int32),
               "minhash": np.zeros((count, H), np.int32), "ordered": np.zeros((count, S, 2), np.int32),
               "ordered_size": np.zeros(count, np.int32), "ordered_seqlen": np.zeros(count, np.int32),
               "status": np.zeros(count, np.uint8)}
        self._chk(self._lib.mhap_index_export(self._h, C.c_int64(first), C.c_int64(count), _ptr(out["ids"]), _ptr(out["is_fwd"]),
                                              _ptr(out["seq_length"]), _ptr(out["minhash"]), _ptr(out["ordered"]),
                                              _ptr(out["ordered_size"]), _ptr(out["ordered_seqlen"]), _ptr(out["status"])))
        return out

    def add_sketches(self, sk):
        m = len(sk["ids"])
        a = {k: np.ascontiguousarray(v) for k, v in sk.items()}
        self._chk(self._lib.mhap_index_add_sketches(self._h, _ptr(a["ids"].astype(np.int64)), _ptr(a["is_fwd"].astype(np.uint8)),
                                                    _ptr(a["seq_length"].astype(np.int32)), _ptr(a["minhash"].astype(np.int32)),
                                                    _ptr(a["ordered"].astype(np.int32)), _ptr(a["ordered_size"].astype(np.int32)),
                                                    _ptr(a["ordered_seqlen"].astype(np.int32)), C.c_int64(m)))

    # -- multi-GPU plumbing (device pointers owned by the caller, e.g. torch tensors) -----------
    def sketch_reads_device(self, fasta, d_minhash_ptr, d_ordered_ptr, d_meta_ptr):
        self._chk(self._lib.mhap_sketch_reads_device(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                                     C.c_int64(len(fasta)), C.c_void_p(d_minhash_ptr), C.c_void_p(d_ordered_ptr),
                                                     C.c_void_p(d_meta_ptr)))

    def set_device_index(self, ids, is_fwd, d_minhash_ptr, d_ordered_ptr, d_meta_ptr):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        is_fwd = np.ascontiguousarray(is_fwd, dtype=np.uint8)
        self._chk(self._lib.mhap_index_set_device(self._h, _ptr(ids), _ptr(is_fwd), C.c_void_p(d_minhash_ptr),
                                                  C.c_void_p(d_ordered_ptr), C.c_void_p(d_meta_ptr), C.c_int64(len(ids))))

    # -- search ---------------------------------------------------------------------------------
    def _collect(self, call):
        return _collect_records(call, self._chk)

    def prepare_index(self):
        """Build the inverted index now (reads the MinHash/meta tables only; see mhap_index_prepare)."""
        self._chk(self._lib.mhap_index_prepare(self._h))

    def find_matches(self, q_first=0, q_count=-1):
        """Self overlap of forward entries [q_first, q_first+q_count) against the whole index."""
        return self._collect(lambda cb: self._lib.mhap_find_matches_self(self._h, C.c_int64(q_first), C.c_int64(q_count), cb, None))

    def find_matches_shard(self, shard, nshards):
        """This rank's share of the self overlap (reads with ordinal % nshards == shard are the queries)."""
        return self._collect(lambda cb: self._lib.mhap_find_matches_self_shard(self._h, C.c_int64(shard), C.c_int64(nshards), cb, None))

    def find_matches_stream(self, fasta):
        return self._collect(lambda cb: self._lib.mhap_find_matches_reads(self._h, _ptr(fasta.bases), _ptr(fasta.offsets),
                                                                          _ptr(fasta.lengths), _ptr(fasta.ids),
                                                                          C.c_int64(len(fasta)), cb, None))

    def find_matches_sketches(self, sk):
        """-q x.dat: precomputed (forward) query sketches against the index, toSelf=false."""
        a = {k: np.ascontiguousarray(v) for k, v in sk.items()}
        ids = a["ids"].astype(np.int64); sl = a["seq_length"].astype(np.int32); mh = a["minhash"].astype(np.int32)
        od = a["ordered"].astype(np.int32); osz = a["ordered_size"].astype(np.int32); osl = a["ordered_seqlen"].astype(np.int32)
        return self._collect(lambda cb: self._lib.mhap_find_matches_sketches(self._h, _ptr(ids), _ptr(sl), _ptr(mh), _ptr(od), _ptr(osz),
                                                                            _ptr(osl), C.c_int64(len(ids)), cb, None))

    def find_matches_device(self, d_q_minhash_ptr, d_q_ordered_ptr, d_q_meta_ptr, ids, to_self=True, before_second_stage=None, count_only=False):
        """Device-resident query sketches (forward rows of the ranks' tables) against this handle's index.
        before_second_stage: callable run once the candidates are known and before the ordered rows are read (e.g. the wait
        for their asynchronous all-gather).  count_only: no sink — the library reads the records back and converts them as always,
        nobody keeps them; returns their number (10^8 records and more per search: what a driver would stream to a file)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        gate = None
        if before_second_stage is not None:
            done = [False]

            def _gate(user):
                if not done[0]:
                    before_second_stage()
                    done[0] = True
                return 0
            gate = _GATE(_gate)
            self._chk(self._lib.mhap_set_second_stage_gate(self._h, gate, None))
        try:
            def call(cb):
                return self._lib.mhap_find_matches_device(self._h, C.c_void_p(d_q_minhash_ptr), C.c_void_p(d_q_ordered_ptr), C.c_void_p(d_q_meta_ptr),
                                                          _ptr(ids), C.c_int64(len(ids)), C.c_int(1 if to_self else 0), cb, None)
            if count_only:
                before = self.stats()["matches_found"]
                self._chk(call(_SINK(0)))
                return self.stats()["matches_found"] - before
            return self._collect(call)
        finally:
            if gate is not None:
                self._chk(self._lib.mhap_set_second_stage_gate(self._h, _GATE(0), None))
                if not done[0]:
                    before_second_stage()       # no candidates at all: the caller still expects the wait to have happened

    # -- one process per GPU: this handle as rank `rank` of `nranks` (the exchange runs inside the library, RCCL over xGMI) ----
    @staticmethod
    def dist_unique_id():
        """ncclGetUniqueId: 128 bytes that rank 0 hands to the other ranks (any channel) before dist_init."""
        buf = C.create_string_buffer(128)
        rc = load_library().mhap_dist_unique_id(buf, C.c_size_t(128))
        if rc != 0:
            raise MhapError(f"mhap_dist_unique_id failed ({rc}): RCCL is not loadable")
        return buf.raw

    def dist_init(self, rank, nranks, unique_id):
        self._chk(self._lib.mhap_dist_init(self._h, C.c_int32(rank), C.c_int32(nranks), C.c_char_p(bytes(unique_id))))

    def dist_set_eager(self, on=True):
        """Eager exchange (mhap_dist_set_eager): the add that fills this rank's empty index becomes collective and gathers the rank's
        forward rows while it computes; the sharded search then starts with all rows in place."""
        self._chk(self._lib.mhap_dist_set_eager(self._h, C.c_int32(1 if on else 0)))

    def dist_eager_searches(self):
        self._lib.mhap_dist_eager_searches.restype = C.c_int64
        return int(self._lib.mhap_dist_eager_searches(self._h))

    def dist_finalize(self):
        self._chk(self._lib.mhap_dist_finalize(self._h))

    def dist_find_matches(self):
        """Collective: self overlap of the union of the ranks' indexes; returns this rank's records."""
        return self._collect(lambda cb: self._lib.mhap_dist_find_matches_self(self._h, cb, None))

    def dist_find_matches_stream(self, fasta):
        """Collective, -q mode: `fasta` = the query reads dealt to this rank."""
        return self._collect(lambda cb: self._lib.mhap_dist_find_matches_reads(self._h, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                                                              _ptr(fasta.ids), C.c_int64(len(fasta)), cb, None))

    def dist_last_timing(self):
        t = (C.c_double * 3)()
        self._chk(self._lib.mhap_dist_last_timing(self._h, t))
        return {"gather_small_ms": t[0], "wait_ordered_ms": t[1], "total_ms": t[2]}

    def dist_info(self):
        """The transport's own view of this rank (mhap_dist_info): what a launcher checks to see that N ranks on N devices formed one communicator."""
        out = (C.c_int32 * 5)()
        pci = C.create_string_buffer(64)
        self._chk(self._lib.mhap_dist_info(self._h, out, pci, C.c_size_t(64)))
        ver = int(out[4])
        return {"comm_count": int(out[0]), "comm_user_rank": int(out[1]), "comm_device": int(out[2]), "handle_device": int(out[3]),
                "rccl_version": (f"{ver // 10000}.{ver // 100 % 100}.{ver % 100}" if ver else None), "pci_bus_id": pci.value.decode() or None}

    def dist_exchange_timing(self):
        """The eager exchange of the last add as the exchange stream saw it: mhap_dist_exchange_timing."""
        out = (C.c_double * 4)()
        self._chk(self._lib.mhap_dist_exchange_timing(self._h, out))
        return {"ordered_gather_ms": out[0], "ordered_bytes_received": out[1], "small_gather_ms": out[2], "small_bytes_received": out[3]}

    def dist_selftest(self, nbytes=1 << 20):
        """Collective: all-gather `nbytes` of a known pattern per rank through the handle's transport and check every block; returns the gather's ms."""
        ms = C.c_double(0.0)
        self._chk(self._lib.mhap_dist_selftest(self._h, C.c_size_t(nbytes), C.byref(ms)))
        return float(ms.value)

    # -- counters -------------------------------------------------------------------------------
    def stats(self):
        s = _Stats()
        self._chk(self._lib.mhap_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _Stats._fields_}

    def kernel_times(self):
        t = _KTimes()
        self._chk(self._lib.mhap_get_kernel_times(self._h, C.byref(t)))
        return {KERNEL_NAMES[i]: {"ms": t.ms[i], "launches": t.launches[i]} for i in range(len(KERNEL_NAMES))}

    def reset_kernel_times(self):
        self._chk(self._lib.mhap_reset_kernel_times(self._h))

    def synchronize(self):
        self._chk(self._lib.mhap_synchronize(self._h))


class MinHashSearchGroup:
    """One process, N GPUs: N ranks of one sharded index (mhap_group_*: AbstractMatchSearch's drivers over several devices).
    Reads are dealt round-robin; every rank sketches and indexes its share; a search gathers the forward query rows of all
    ranks (peer-to-peer copies over xGMI, or RCCL with MHAP_GROUP_TRANSPORT=rccl) and each rank searches them against its shard."""

    def __init__(self, params=None, n=1, devices=None, kmer_filter=None):
        self._lib = load_library()
        self.params = params or MhapParams()
        self._g = C.c_void_p()
        err = C.create_string_buffer(512)
        p = self.params._c()
        dev = (C.c_int32 * n)(*devices) if devices is not None else None
        rc = self._lib.mhap_group_create(C.byref(p), dev, C.c_int32(n), C.byref(self._g), err, C.c_size_t(512))
        if rc != 0:
            self._g = C.c_void_p()
            raise MhapError(err.value.decode() or f"mhap_group_create failed ({rc})")
        self.n = n
        if kmer_filter is not None:
            for r in range(n):
                self.rank(r).set_filter(kmer_filter)

    def rank(self, r):
        """A non-owning MinHashSearch view of rank r's handle (filters, counters)."""
        v = MinHashSearch.__new__(MinHashSearch)
        v._lib, v.params = self._lib, self.params
        h = self._lib.mhap_group_rank(self._g, C.c_int32(r))
        if not h:
            raise MhapError("rank out of range")
        v._h = C.c_void_p(h)
        v.close = lambda: None
        return v

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._lib.mhap_group_destroy(self._g)
            self._g = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MhapError(f"{self._lib.mhap_group_last_error(self._g).decode()} (code {rc})")

    def add_data(self, fasta):
        self._chk(self._lib.mhap_group_add_reads(self._g, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths), _ptr(fasta.ids),
                                                 C.c_int64(len(fasta))))

    def add_scan(self, scan):
        self._chk(self._lib.mhap_group_add_scan(self._g, scan._s))

    def clear(self):
        self._chk(self._lib.mhap_group_clear(self._g))

    def _collect(self, call):
        return _collect_records(call, self._chk)

    def find_matches(self):
        return self._collect(lambda cb: self._lib.mhap_group_find_matches_self(self._g, cb, None))

    def find_matches_stream(self, fasta):
        return self._collect(lambda cb: self._lib.mhap_group_find_matches_reads(self._g, _ptr(fasta.bases), _ptr(fasta.offsets), _ptr(fasta.lengths),
                                                                               _ptr(fasta.ids), C.c_int64(len(fasta)), cb, None))

    def stats(self):
        s = _Stats()
        self._chk(self._lib.mhap_group_get_stats(self._g, C.byref(s)))
        return {k: getattr(s, k) for k, _ in _Stats._fields_}
