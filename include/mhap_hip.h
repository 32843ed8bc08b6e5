/*
 * mhap_hip.h — C ABI of libmhaphip.so, the MI355X (gfx950) MinHash overlap engine.
 *
 * This is the drop-in boundary for MHAP's hot path.  The reference (marbl/MHAP, Java)
 * has no FFI; its only operator seam is the abstract class
 *   J/impl/AbstractMatchSearch.java:47   (J/ = src/main/java/edu/umd/marbl/mhap/)
 * with MinHashSearch as the sole implementation.  Per-read JNI calls would serialise
 * the GPU, so every entry point below is batch-granular.  Each entry point cites the
 * reference interface it replaces.  INTEGRATION.md shows the JNI stub + the Java
 * subclass (HipMinHashSearch extends AbstractMatchSearch) a maintainer would add.
 *
 * Conventions: C linkage, plain pointers and sizes, no exceptions cross the boundary.
 * Every call returns 0 on success or a negative MHAP_E_* code; the message is
 * available from mhap_last_error().  A handle is NOT re-entrant: the caller
 * serialises calls on one handle (the library overlaps work on its own HIP stream).
 * There is no CPU fallback: without a usable HIP device mhap_create() fails.
 */
#ifndef MHAP_HIP_H
#define MHAP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHAP_OK 0
#define MHAP_E_INVALID (-1)     /* bad argument / unsupported option (MhapRuntimeException analogue) */
#define MHAP_E_HIP (-2)         /* HIP runtime error, no device, kernel failure */
#define MHAP_E_NOMEM (-3)
#define MHAP_E_STATE (-4)       /* call sequence error (e.g. search before index) */
#define MHAP_E_IO (-5)          /* a file could not be opened / read */

/* Per-strand sketch status (mirrors the streamer's skip rules). */
#define MHAP_STRAND_OK 0
#define MHAP_STRAND_ZERO_NGRAMS 1 /* ZeroNGramsFoundException, J/impl/SequenceSketchStreamer.java:235-238 */
#define MHAP_STRAND_TOO_SHORT 2   /* L < --min-olap-length,    J/impl/SequenceSketchStreamer.java:129-133 */

/* Flag table of J/main/MhapMain.java:67-125 that reaches the hot path. */
typedef struct mhap_params {
  int32_t kmer_size;           /* -k                      (16)   MhapMain.java:75,107  */
  int32_t num_hashes;          /* --num-hashes            (512)  :87,108               */
  int32_t ordered_kmer_size;   /* --ordered-kmer-size     (12)   :89,116               */
  int32_t ordered_sketch_size; /* --ordered-sketch-size   (1536) :91,117               */
  int32_t num_min_matches;     /* --num-min-matches       (3)    :83,112               */
  int32_t min_store_length;    /* --min-store-length      (0)    :79,118               */
  int32_t min_olap_length;     /* --min-olap-length       (116)  :81,119               */
  int32_t device;              /* HIP device ordinal; -1 = current device              */
  double threshold;            /* --threshold             (0.78) :67,109               */
  double max_shift;            /* --max-shift             (0.2)  :77,111               */
  double repeat_weight;        /* --repeat-weight         (0.9)  :69,114               */
} mhap_params;

/* One overlap = the fields of J/impl/MatchResult.java:46-65 (before text formatting). */
typedef struct mhap_record {
  int64_t from_id, to_id;  /* SequenceId.getHeaderId()  */
  double score;            /* OverlapInfo.score (identity); the text column is 1-min(score,1) */
  double raw;              /* OverlapInfo.rawScore = number of valid shared k-mers */
  int32_t a1, a2, alen;    /* query interval + full length (fromLength)       */
  int32_t b1, b2, blen;    /* match interval (already flipped if to_rc) + toLength */
  int32_t to_rc;           /* 0 fwd / 1 reverse-complement entry              */
  int32_t pad;
} mhap_record;

/* Counters behind MhapMain.outputFinalStat (J/main/MhapMain.java:572-590). */
typedef struct mhap_stats {
  int64_t strands_indexed;        /* MinHashSearch.size()                        */
  int64_t queries_searched;       /* getNumberSequencesSearched()                */
  int64_t candidates_compared;    /* getNumberSequencesFullyCompared()           */
  int64_t matches_found;          /* getMatchesProcessed()                       */
  int64_t slot_compares;          /* slot comparisons done by the brute-force candidate kernel (MHAP_CANDIDATES=bruteforce) */
  int64_t table_elements;         /* getNumberElementsProcessed(): inverted-index hits walked             */
  int64_t slow_pairs;             /* candidates the wave-per-pair second stage handed to the per-lane merge */
  int64_t index_splits;           /* query hit sets too large for the LDS count table that were split into hash-partition passes */
} mhap_stats;

/* Per-kernel HIP-event timings accumulated on the handle's stream (for bench/roofline). */
#define MHAP_K_HASH 0      /* hash_kmers_kernel: murmur3 of every k-mer / k2-mer into HBM — only for reads the kernels cannot hash from
                              their 2-bit codes (raw bytes, k != 16 or k2 != 12, reads beyond 24 591 bases); 0 on the default path */
#define MHAP_K_WEIGHT 1    /* kmer_weight_kernel: per-strand k-mer multiplicity / tf-idf weight, weight classes, MinHash work lists */
#define MHAP_K_DEDUP MHAP_K_WEIGHT   /* (name of rounds 1-2) */
#define MHAP_K_MINHASH 2   /* minhash_kernel: weighted xorshift MinHash (hashes its k-mers from the 2-bit codes)            */
#define MHAP_K_ORDERED 3   /* ordered_kernel: 12-mer hashes + bottom-S select + sort                                     */
#define MHAP_K_CANDIDATE 4 /* candidate_kernel: brute-force all-pairs slot-equality count (MHAP_CANDIDATES=bruteforce only) */
#define MHAP_K_OVERLAP 5   /* overlap_join_kernel (+ overlap_kernel for the pairs it hands over): second-stage getOverlapInfo */
#define MHAP_K_INDEX_BUILD 6 /* index_build + index_finalize: inverted index (MinHashSearch.addSequence) */
#define MHAP_K_INDEX_QUERY 7 /* index_query_kernel: inverted index lookups + per-query hit counting  */
#define MHAP_K_COUNT 8
typedef struct mhap_kernel_times {
  double ms[MHAP_K_COUNT];      /* summed kernel time, milliseconds */
  int64_t launches[MHAP_K_COUNT];
} mhap_kernel_times;

/* Interface version of this header (bumped whenever a struct layout or a signature changes) and the sizes of its structs as the
 * library was compiled: a binding built against another header — a stale libmhaphip.so shipped next to newer host code — finds
 * out at load time instead of overrunning a buffer. */
#define MHAP_ABI_VERSION 4
int mhap_abi_version(void);
int mhap_abi_sizes(int32_t* out4);   /* {sizeof mhap_params, mhap_record, mhap_stats, mhap_kernel_times} */

typedef struct mhap_handle mhap_handle;

/* Record sink: called from the calling thread, one batch at a time; `recs` is owned by
 * the library and valid only during the call.  Replaces AbstractMatchSearch.outputResults
 * (J/impl/AbstractMatchSearch.java:316-338).  Return non-zero to abort the search. */
typedef int (*mhap_record_sink)(const mhap_record* recs, int64_t n, void* user);
/* Optional gate between the two stages of a search: called (from the calling thread) after the candidates of a batch of queries
 * are known and before their ordered sketches are read.  A multi-GPU host uses it to wait for the asynchronous exchange of the
 * ordered-sketch rows, which then overlaps the candidate stage.  Non-zero aborts the search.  NULL removes the gate. */
typedef int (*mhap_stage_gate)(void* user);
int mhap_set_second_stage_gate(mhap_handle* h, mhap_stage_gate gate, void* user);

/* Replaces `new MinHashSearch(...)` argument plumbing (J/impl/MinHashSearch.java:63-98). */
int mhap_create(const mhap_params* params, mhap_handle** out, char* err, size_t errcap);
void mhap_destroy(mhap_handle* h);
const char* mhap_last_error(const mhap_handle* h);
void mhap_default_params(mhap_params* p);

/* Host-built repeat filter = J/sketch/FrequencyCounts.java:63-229 after parsing.
 * hashes[i] = murmur3_x64_128 h1 of the (canonicalised per --no-rc) k-mer, fractions[i] its
 * column-2 value; entries with fraction < filter_cutoff are dropped here (:176-184).
 * offset = repeat_weight if 0<=rw<1 else 0 (MhapMain.java:346-350); range = --repeat-idf-scale.
 * Only --supress-noise 0 is supported.  n == 0 clears the filter. */
int mhap_set_filter(mhap_handle* h, const int64_t* hashes, const double* fractions, int64_t n,
                    double filter_cutoff, double offset, double range, int no_tf);
/* --supress-noise 1|2 (FrequencyCounts removeUnique, J/sketch/FrequencyCounts.java:66-68,137,192,272-278,297): the Bloom filter
 * over EVERY k-mer of the filter file (hashes: all n lines, not only the ones above the cutoff), built exactly like Guava 19.0's
 * BloomFilter.create(funnel(putLong), size_bloom, 1e-5) (strategy MURMUR128_MITZ_64).  mode 1: k-mers that are not in the
 * file are dropped from the MinHash sketch; mode 2: they get idf 1; mode 0 removes the whitelist.  Call after mhap_set_filter. */
int mhap_set_filter_whitelist(mhap_handle* h, const int64_t* hashes, int64_t n, int64_t size_bloom, int32_t mode);
/* new FrequencyCounts(reader, filterCutoff, offset, removeUnique, noTf, numThreads, range, doReverseCompliment)
 * (J/sketch/FrequencyCounts.java:63-229, called from J/main/MhapMain.java:337-361): reads the -f file (first line
 * "sizeBloom sizeRepeat", then `kmer fraction ...` lines), hashes the k-mers (canonical when do_rc) and installs the table
 * (+ the whitelist when remove_unique > 0).  kmer_sizes (may be NULL) receives the distinct k-mer lengths, e.g. "16". */
int mhap_set_filter_file(mhap_handle* h, const char* path, double filter_cutoff, double offset, int32_t remove_unique, int32_t no_tf,
                         double range, int32_t do_rc, char* kmer_sizes, size_t kmer_sizes_cap);

/* Sketch `n` reads (both strands) and append them to the index.  Replaces
 * SequenceSketchStreamer.enqueue/getSketch (J/impl/SequenceSketchStreamer.java:123-177,262-266)
 * + MinHashSearch.addSequence (J/impl/MinHashSearch.java:100-147).
 * bases: concatenated upper-cased sequence bytes (one byte per Java char);
 * offsets[i]/lengths[i] locate read i; ids[i] = SequenceId.getHeaderId (1-based FASTA order).
 * Every read takes two entries (fwd = 2*j, rc = 2*j+1, j = running read count); entries that
 * the reference would skip are kept as non-matchable placeholders (see mhap_index_status). */
int mhap_index_add_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths,
                         const int64_t* ids, int64_t n);

/* Two-step form of mhap_index_add_reads for callers that want the reads resident in HBM before the compute
 * starts (the benchmark's timed region): mhap_stage_reads packs the reads to 2 bits/base (raw bytes for reads
 * with non-ACGT chars) and uploads them once; mhap_index_add_staged then only launches kernels.  Staged reads
 * stay staged until the next mhap_stage_reads / mhap_index_add_reads / mhap_sketch_* call. */
int mhap_stage_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths,
                     const int64_t* ids, int64_t n);
int mhap_index_add_staged(mhap_handle* h);

/* The reads an EMPTY index is about to receive over the coming mhap_index_add_* calls (a file added in batches, as
 * AbstractMatchSearch.addData does, J/impl/AbstractMatchSearch.java:67-117): the sketch tables are sized once for all of
 * them, so that no batch makes them grow (a reallocation + copy of every row sketched so far).  The inverted index is built
 * from all rows by the first search after the last add (a counting sort of the postings: 3 ms per 10^8). */
int mhap_index_reserve(mhap_handle* h, int64_t total_reads);

/* Streamed FASTA ingest (FastaData + SequenceSketchStreamer.enqueueFullFile, J/impl/FastaData.java:101-204,
 * J/impl/SequenceSketchStreamer.java:179-222: the reference reads and sketches through a queue with T threads).
 * mhap_fasta_scan_open maps the file (plain text; gz / bz2 are inflated into memory first) and finds its records on all host
 * threads: ids (1-based count of non-empty records + id_offset), lengths, whether a read is pure ACGT — no copy of the bases.
 * mhap_index_add_scan then feeds the index in groups of <= 256 Mbase: host threads pack group g+1 from the text straight into
 * pinned 2-bit staging while the GPU sketches and indexes group g (two staging buffers), so parsing, packing, the upload and the
 * kernels overlap and the 1-byte-per-base copy of the reads never exists. */
typedef struct mhap_fasta_scan mhap_fasta_scan;
int mhap_fasta_scan_open(const char* path, int64_t id_offset, mhap_fasta_scan** out, char* err, size_t errcap);
void mhap_fasta_scan_free(mhap_fasta_scan* s);
int64_t mhap_fasta_scan_reads(const mhap_fasta_scan* s);          /* non-empty records */
int64_t mhap_fasta_scan_bases(const mhap_fasta_scan* s);
/* ids[n], lengths[n] (either may be NULL); headers: the n NUL-terminated names back to back (mhap_fasta.headers), valid until the scan is freed */
int mhap_fasta_scan_info(mhap_fasta_scan* s, int64_t* ids, int32_t* lengths, const char** headers, int64_t* headers_bytes);
/* 1 when the scanned file is FASTQ ("FASTQ input" below); then mhap_fasta_scan_qualities copies one Phred byte per base, in the
 * reads' order (mhap_fasta_scan_bases bytes).  MHAP_E_INVALID on a FASTA scan. */
int mhap_fasta_scan_has_qualities(const mhap_fasta_scan* s);
int mhap_fasta_scan_qualities(const mhap_fasta_scan* s, uint8_t* qualities);
int mhap_index_add_scan(mhap_handle* h, const mhap_fasta_scan* s);
/* the reads of the scan as query reads against the index (-q mode, mhap_find_matches_reads), in groups */
int mhap_find_matches_scan(mhap_handle* h, const mhap_fasta_scan* s, mhap_record_sink sink, void* user);

/* Exact k-mer counting (k = 1..16) on the GPU and the `-f` repeat filter file made from it (the file FrequencyCounts reads,
 * J/sketch/FrequencyCounts.java:63-200; MHAP itself never writes it).  A window [i, i+k) of a read counts when its k bytes are all
 * A, C, G or T (a scanned FASTA file is upper-cased by the ingest; mhap_kmer_count_add_reads takes its bytes as they are); its value
 * has 2 bits per base (A=0 C=1 G=2 T=3, first base most significant); canonical: min(value, value of its reverse complement).  Only
 * the forward strand is read, and reads shorter than --min-olap-length count too.  One count per handle at a time, between _begin and
 * _finish; index calls in between close it (MHAP_E_STATE), as does any failed add.  A k-mer seen more than 2^32 - 1 times is an error. */
typedef struct mhap_kmer_counts mhap_kmer_counts;
int mhap_kmer_count_begin(mhap_handle* h, int32_t k, int32_t canonical);
int mhap_kmer_count_add_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n);
/* the reads of a scanned file through the ingest's pipeline (host threads pack group g + 1 while the GPU counts group g) */
int mhap_kmer_count_add_scan(mhap_handle* h, const mhap_fasta_scan* s);
/* ends the count: the lines are the k-mers with (double)count / total >= min_fraction, by descending count, then ascending value */
int mhap_kmer_count_finish(mhap_handle* h, double min_fraction, mhap_kmer_counts** out);
/* the same with flags (0: exactly mhap_kmer_count_finish; unknown bits: MHAP_E_INVALID, the count stays open).  MHAP_KMER_HISTOGRAM
 * also keeps the histogram of the final counts, made on the device in the same pass: for every count c >= 1, the number of distinct
 * values counted c times (the lines and the `-f` file are the same with it as without it). */
#define MHAP_KMER_HISTOGRAM 1
int mhap_kmer_count_finish_flags(mhap_handle* h, double min_fraction, uint32_t flags, mhap_kmer_counts** out);
/* windows counted, distinct values, lines, k */
int mhap_kmer_counts_info(const mhap_kmer_counts* c, int64_t* total, int64_t* distinct, int64_t* lines, int32_t* k);
int mhap_kmer_counts_lines(const mhap_kmer_counts* c, uint64_t* kmers, uint64_t* counts);   /* `lines` entries each, in file order */
/* the `-f` file: "<distinct> <lines>", then "<kmer>\t<count / total as %.10e>" per line; MHAP_E_IO when it cannot be written */
int mhap_kmer_counts_write(const mhap_kmer_counts* c, const char* path);
/* The histogram (counts made with MHAP_KMER_HISTOGRAM; else MHAP_E_STATE and *n = 0): n entries in ascending count, nonzero ones only;
 * the numbers sum to `distinct` and count x number sums to `total`.  _write_histogram writes "<count>\t<number>\n" per entry, the
 * k-mer count histogram GetHistogramStats reads (J/main/GetHistogramStats.java:50-55: Integer.parseInt of column 0, Long.parseLong of
 * column 1; a count above 2^31 - 1 ends its reading there); MHAP_E_IO when the file cannot be written. */
int mhap_kmer_counts_histogram_size(const mhap_kmer_counts* c, int64_t* n);
int mhap_kmer_counts_histogram(const mhap_kmer_counts* c, uint32_t* counts, uint64_t* numbers);
int mhap_kmer_counts_write_histogram(const mhap_kmer_counts* c, const char* path);
void mhap_kmer_counts_free(mhap_kmer_counts* c);
/* MHAP_KMER_KEEP_OPEN in the flags of mhap_kmer_count_finish_flags: the counts are made as usual and the count stays open on the
 * handle (the finish reads the open state and leaves it as it is), so that one count of the reads gives the `-f` file and, from
 * mhap_kmer_count_finish_set after it, the set below.  A failed finish closes the count with or without it. */
#define MHAP_KMER_KEEP_OPEN 2

/* Sequence assessment without a reference: sequences (corrected reads, unitigs, a consensus) against the k-mers of the reads they
 * came from.  A k-mer of a sequence that the reads do not support is an error (from these a consensus QV); a solid k-mer of the
 * reads that the sequences lack is lost sequence (from these completeness).  Windows, values and canonical are the counter's.
 *
 * The set.  mhap_kmer_count_finish_set ends an open count as mhap_kmer_count_finish does and leaves on the device a bitmap of 4^k
 * bits (512 MiB at k = 16, sized by k alone): bit v is set iff the final count of value v is >= min_count.  min_count 0: the
 * valley of the count histogram, the smallest c >= 1 with n[c + 1] >= n[c], where n[c] is the number of distinct values counted c
 * times (0 where absent) - below it lie the k-mers that the reads' errors made.  mhap_kmer_histogram_valley is that rule on the
 * arrays mhap_kmer_counts_histogram returns (host only; counts ascending and >= 1, else MHAP_E_INVALID).  The set owns its memory,
 * outlives the count and is used with handles on the device it was made on.  _info: windows counted, distinct values, members (set
 * bits), k, canonical, the min_count used.  _contains: out[i] = 1 when the set holds values[i].
 *
 * Sequences against a set.  For a sequence of n bases and window starts i in [0, n - k]: valid_i as the counter defines it (a
 * scanned file is upper-cased by the ingest, mhap_kmer_eval_reads takes its bytes as they are), present_i = valid_i and the set holds
 * the window's value, missing_i = valid_i and it does not.  Every sequence gets a row of five int64: bases = n; windows = the valid
 * ones; missing = the missing ones; runs = the i with missing_i and (i = 0 or not missing_{i-1}), so an invalid or a present window
 * ends a run; unsupported = the positions p that some valid window contains and no present window contains.  The intervals are the
 * maximal stretches [begin, end) of consecutive unsupported positions, as (sequence index, begin, end), ordered by sequence, then
 * begin.  A sequence shorter than k, or without a valid window, has zeros after `bases`.  Integers only: the results are a function
 * of the input.  mhap_kmer_eval_scan takes the groups of a scanned file through the streamed ingest and accumulates over them.
 * _info: sequences, intervals, k and totals[5], the column sums of the rows.  _rows: sequences x 5, _intervals: intervals x 3.
 *
 * mhap_kmer_qv: error = 1 - (1 - missing / windows)^(1 / k) per base, qv = -10 log10 of it; windows = 0: NaN for both; missing = 0:
 * error 0, qv +inf.  mhap_kmer_eval_write_table writes "name\tbases\twindows\tmissing\truns\tunsupported\terror\tqv" per sequence
 * (error as %.6e, qv as %.2f) and a last line named total; names are NUL-terminated and back to back, as mhap_fasta_scan_info hands
 * them (NULL: seq1, seq2, ...).  mhap_kmer_eval_write_bed writes "name\tbegin\tend" per interval.  MHAP_E_IO when a file cannot be
 * written.  mhap_kmer_eval_summary writes the one line both tools print: the totals, the QV and, with the set of the sequences' own
 * k-mers (own, may be NULL) and `both` from mhap_kmer_set_compare, completeness = both / members of the reads' set.
 *
 * Set against set.  mhap_kmer_set_compare counts the members of a, of b and of both; sets that differ in k or canonical are refused
 * (MHAP_E_INVALID).  Completeness of an assembly: a = the reads' solid set, b = the set of the assembly's own k-mers (count the
 * assembly, min_count 1).
 *
 * Limits: k <= 16 is the counter's; at k = 16 a genome of some hundred megabases fills much of the 4^16 values with its own k-mers, an
 * erroneous k-mer is then present by chance and the QV saturates - bacterial genomes are the intended use.  Sequences are below 2^31
 * bases.  With reads at 10 % error a min_count of 1 is nearly useless (the reads' error k-mers excuse the sequences' errors): hence
 * the valley. */
typedef struct mhap_kmer_set mhap_kmer_set;
typedef struct mhap_kmer_eval mhap_kmer_eval;
int mhap_kmer_histogram_valley(const uint32_t* counts, const uint64_t* numbers, int64_t n, uint64_t* valley);
int mhap_kmer_qv(int64_t windows, int64_t missing, int32_t k, double* error, double* qv);
int mhap_kmer_count_finish_set(mhap_handle* h, uint64_t min_count, mhap_kmer_set** out);
void mhap_kmer_set_free(mhap_kmer_set* s);
int mhap_kmer_set_info(const mhap_kmer_set* s, int64_t* total, int64_t* distinct, int64_t* members, int32_t* k, int32_t* canonical, uint64_t* min_count);
int mhap_kmer_set_contains(mhap_handle* h, const mhap_kmer_set* s, const uint64_t* values, int64_t n, uint8_t* out);
int mhap_kmer_set_compare(mhap_handle* h, const mhap_kmer_set* a, const mhap_kmer_set* b, int64_t* a_members, int64_t* b_members, int64_t* both);
int mhap_kmer_eval_reads(mhap_handle* h, const mhap_kmer_set* s, const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n,
                         mhap_kmer_eval** out);
int mhap_kmer_eval_scan(mhap_handle* h, const mhap_kmer_set* s, const mhap_fasta_scan* scan, mhap_kmer_eval** out);
void mhap_kmer_eval_free(mhap_kmer_eval* e);
int mhap_kmer_eval_info(const mhap_kmer_eval* e, int64_t* sequences, int64_t* intervals, int32_t* k, int64_t* totals);
int mhap_kmer_eval_rows(const mhap_kmer_eval* e, int64_t* rows);
int mhap_kmer_eval_intervals(const mhap_kmer_eval* e, int64_t* intervals);
int mhap_kmer_eval_write_table(const mhap_kmer_eval* e, const char* names, const char* path);
int mhap_kmer_eval_write_bed(const mhap_kmer_eval* e, const char* names, const char* path);
int mhap_kmer_eval_summary(const mhap_kmer_eval* e, const mhap_kmer_set* reads, const mhap_kmer_set* own, int64_t both, char* line, size_t cap);

/* Sketch only (no index change); outputs to caller-allocated HOST arrays, any may be NULL:
 * minhash[2n][max(1,H)], ordered[2n][S][2] (hash,pos), ordered_size[2n], status[2n].
 * Strand order: 2*i = forward, 2*i+1 = reverse complement.  Used by parity tests and the
 * `.dat` writer (J/impl/SequenceSketch.java:123-148). */
int mhap_sketch_batch(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n,
                      int32_t* minhash, int32_t* ordered, int32_t* ordered_size, uint8_t* status);

/* Ingest precomputed sketches (from `.dat`, J/impl/SequenceSketch.java:61-96): `m` entries, host arrays.
 * is_fwd[e], seq_length[e] = full base length, ordered_seqlen[e] = L-k2+1 as stored in the file. */
int mhap_index_add_sketches(mhap_handle* h, const int64_t* ids, const uint8_t* is_fwd, const int32_t* seq_length,
                            const int32_t* minhash, const int32_t* ordered, const int32_t* ordered_size,
                            const int32_t* ordered_seqlen, int64_t m);

/* Index introspection: number of entries (incl. placeholders); copy-out of the tables (any NULL). */
int mhap_index_size(mhap_handle* h, int64_t* entries);
int mhap_index_export(mhap_handle* h, int64_t first, int64_t count, int64_t* ids, uint8_t* is_fwd, int32_t* seq_length,
                      int32_t* minhash, int32_t* ordered, int32_t* ordered_size, int32_t* ordered_seqlen,
                      uint8_t* status);
int mhap_index_clear(mhap_handle* h);
/* Build the inverted index (MinHashSearch.addSequence's per-slot maps, J/impl/MinHashSearch.java:123-141) for the current
   entries now instead of at the first search; only the MinHash and meta tables are read, so a caller that adopted device
   tables with mhap_index_set_device may still be filling the ordered-sketch table (e.g. an all-gather in flight). */
int mhap_index_prepare(mhap_handle* h);

/* Multi-GPU plumbing (one process per GPU): the per-rank shard tables live in device memory
 * owned by the CALLER (e.g. torch tensors that RCCL all-gathers over xGMI).
 *  - mhap_sketch_reads_device: sketch n reads into caller device buffers
 *      d_minhash int32[2n][Hrow], d_ordered int32[2n][S][2], d_meta int32[2n][4] =
 *      {ordered_size, ordered_seqlen, seq_length, status}; Hrow = max(1,H).
 *  - mhap_index_set_device: adopt (no copy) gathered tables of `m` entries as the index;
 *      ids/is_fwd are host arrays.  The buffers must outlive the handle's use of them. */
int mhap_sketch_reads_device(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths,
                             int64_t n, void* d_minhash, void* d_ordered, void* d_meta);
int mhap_index_set_device(mhap_handle* h, const int64_t* ids, const uint8_t* is_fwd, void* d_minhash,
                          void* d_ordered, void* d_meta, int64_t m);
/* Same as mhap_sketch_reads_device for reads previously staged with mhap_stage_reads (kernels only). */
int mhap_sketch_staged_device(mhap_handle* h, void* d_minhash, void* d_ordered, void* d_meta);

/* Self-overlap: every forward entry in [q_first, q_first+q_count) is searched against the whole
 * index with toSelf=true.  Replaces AbstractMatchSearch.findMatches()
 * (J/impl/AbstractMatchSearch.java:121-199) + MinHashSearch.findMatches(sketch,true)
 * (J/impl/MinHashSearch.java:150-251).  q_count < 0 means "to the end".  Entry indices, not ids. */
int mhap_find_matches_self(mhap_handle* h, int64_t q_first, int64_t q_count, mhap_record_sink sink, void* user);

/* Sharded self-overlap for one-process-per-GPU runs: this call searches the forward entries whose read
 * ordinal (position among the index's reads) is congruent to `shard` modulo `nshards`; the union over all
 * shards equals mhap_find_matches_self(h, 0, -1).  Round-robin balances the triangular id rule.  The ordinal counts the forward
 * entries in entry order, placeholders included: entry / 2 for sketched reads, the entry itself in an index of forward rows only. */
int mhap_find_matches_self_shard(mhap_handle* h, int64_t shard, int64_t nshards, mhap_record_sink sink, void* user);

/* Index-vs-stream (-q mode, toSelf=false): sketch the `n` query reads (forward only,
 * J/impl/AbstractMatchSearch.java:203-285) and search them against the index. */
int mhap_find_matches_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths,
                            const int64_t* ids, int64_t n, mhap_record_sink sink, void* user);

/* Index-vs-stream with PRECOMPUTED query sketches (a `.dat` file given to -q: only its forward entries are
 * queries, J/impl/SequenceSketchStreamer.java:291-303 with fwdOnly=true): `m` query entries as host arrays laid out
 * like mhap_index_add_sketches; toSelf=false. */
int mhap_find_matches_sketches(mhap_handle* h, const int64_t* ids, const int32_t* seq_length, const int32_t* minhash,
                               const int32_t* ordered, const int32_t* ordered_size, const int32_t* ordered_seqlen, int64_t m,
                               mhap_record_sink sink, void* user);
/* Query sketches that already sit in device memory (the layout mhap_sketch_staged_device / mhap_sketch_reads_device write:
 * minhash int32[m][--num-hashes], ordered int32[m][--ordered-sketch-size][2], meta int32[m][4]) against the index — the
 * multi-GPU exchange step: every rank keeps the index of its OWN reads and the forward query sketches of the other ranks
 * visit it one after the other.  ids: host array, one id per query row; rows whose meta status is not 0 are
 * skipped.  to_self != 0 applies findMatches(hashes, toSelf = true)'s id rules (J/impl/MinHashSearch.java:200-225), so every
 * unordered pair of one data set is reported once however its two reads are spread over ranks. */
int mhap_find_matches_device(mhap_handle* h, const void* d_q_minhash, const void* d_q_ordered, const void* d_q_meta, const int64_t* ids,
                             int64_t m, int to_self, mhap_record_sink sink, void* user);

/* ---- several GPUs: one sharded index, the exchange inside the library -------------------------------------
 * The reference has one JVM, one index and a thread pool (AbstractMatchSearch.addData :67-117, findMatches() :121-199,
 * J/impl/AbstractMatchSearch.java).  Over N GPUs the reads are dealt round-robin (read i of the data set -> rank i % N, which
 * balances the id < id rule of J/impl/MinHashSearch.java:215-219), every rank sketches and indexes ITS reads only, and a search
 * all-gathers the forward-strand query rows of all ranks (MinHash rows, meta and ids first; the 6x larger ordered rows behind
 * the candidate stage) and runs every query against the rank's own index shard with the toSelf id rules — each unordered pair is
 * reported exactly once, by the rank that stores its lower-id read.  No collective after the gather; records go to the sink.
 *
 * Two ways to form the ranks, same code underneath:
 *  (a) one process per GPU (bench.py under torchrun, an MPI-style host): every process creates its handle; rank 0 calls
 *      mhap_dist_unique_id and the host hands the 128 bytes to the other ranks (any channel); all call mhap_dist_init, which
 *      creates an RCCL communicator over the handles' devices (ncclCommInitRank; collectives run over xGMI).
 *  (b) one process, N devices (mhap-hip --gpus N, the JNI host of INTEGRATION.md): mhap_group_* below owns N handles and one
 *      host thread per rank; the gather is direct peer-to-peer copies over xGMI (hipMemcpyPeerAsync: each rank pulls the other
 *      ranks' rows), or RCCL (ncclCommInitAll) with MHAP_GROUP_TRANSPORT=rccl. */
#define MHAP_DIST_ID_BYTES 128
int mhap_dist_unique_id(void* id, size_t cap);                       /* ncclGetUniqueId; cap >= MHAP_DIST_ID_BYTES */
int mhap_dist_init(mhap_handle* h, int32_t rank, int32_t nranks, const void* id);   /* collective over the nranks handles */
int mhap_dist_finalize(mhap_handle* h);
/* Collective: self-overlap of the union of the ranks' indexes (every rank calls it; each gets the records of the pairs whose
 * lower-id read it stores).  The index must consist of sketched reads (mhap_index_add_reads / _staged): forward and reverse
 * entries in pairs.  Replaces AbstractMatchSearch.findMatches() for the sharded index. */
int mhap_dist_find_matches_self(mhap_handle* h, mhap_record_sink sink, void* user);
/* Collective, -q mode (AbstractMatchSearch.findMatches(streamer), toSelf = false): this rank sketches the n query reads it was
 * dealt (forward strands only), the query rows of all ranks are gathered, and every rank searches them against its shard. */
int mhap_dist_find_matches_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths,
                                 const int64_t* ids, int64_t n, mhap_record_sink sink, void* user);
/* wall-clock split of the last collective search on this rank, milliseconds: {pack + small gathers, index + candidate stage wait
 * on the ordered rows, whole call} */
/* Eager exchange: with on != 0, the add that fills an EMPTY index of this rank (mhap_index_add_reads / _staged / _scan) becomes a collective
 * call — every rank must make it, in the same order as its searches — and gathers the rank's forward rows while it is still computing:
 * the ordered rows under the MinHash kernel, the MinHash rows under the index build.  mhap_dist_find_matches_self then starts with every
 * rank's rows in place.  An add that cannot take part (not the first one, more than one launch group, any rank saying so) falls back
 * to the exchange at search time on all ranks together.  Replaces nothing in the reference (it has one index in one JVM,
 * J/impl/AbstractMatchSearch.java:67-117); it is the overlap of SURVEY.md §8(e)'s all-gather with the sketch phase. */
int mhap_dist_set_eager(mhap_handle* h, int32_t on);
int64_t mhap_dist_eager_searches(mhap_handle* h);   /* searches of this rank that found every rank's rows already gathered by the add */
int mhap_dist_last_timing(mhap_handle* h, double* out3);
/* The eager exchange of the last add as the exchange stream saw it (the gathers run UNDER the add's kernels): out4 = {ms of the ordered
 * rows' all-gather, bytes this rank received in it, ms of the MinHash + meta + id rows' all-gathers, bytes received}; -1 ms = not run
 * since the last call.  Waits for the gathers.  With mhap_dist_selftest (the same volume with no kernel beside it) this separates fabric
 * time from the interaction with a power-bound compute kernel (bench.py --exchange-only).  No reference counterpart (§8e tooling). */
int mhap_dist_exchange_timing(mhap_handle* h, double* out4);
/* The transport's own view of this rank (RCCL: ncclCommCount / ncclCommUserRank / ncclCommCuDevice / ncclGetVersion), for a launcher that
 * wants to confirm that its N processes formed ONE communicator over N devices — the reference has nothing to compare: one JVM, one index
 * (AbstractMatchSearch.java:67-117).  out5 = {ranks, this rank, communicator's device, handle's device, RCCL version code};
 * pci = PCI bus id of the device ("0000:05:00.0"). */
int mhap_dist_info(mhap_handle* h, int32_t* out5, char* pci, size_t pci_cap);
/* The exchange by itself: all-gathers `bytes` (<= 1 GiB) of a known pattern per rank through the handle's transport, under the same
 * watchdog as a search, and checks every rank's block.  Collective over the ranks.  ms_out: wall time of the gather (may be NULL). */
int mhap_dist_selftest(mhap_handle* h, size_t bytes, double* ms_out);

typedef struct mhap_group mhap_group;
/* N handles on the given devices (NULL: devices 0..n-1; repeats allowed — several ranks may share a device, which is how a
 * one-GPU box tests the N > 1 path). */
int mhap_group_create(const mhap_params* params, const int32_t* devices, int32_t n, mhap_group** out, char* err, size_t errcap);
void mhap_group_destroy(mhap_group* g);
int32_t mhap_group_size(const mhap_group* g);
mhap_handle* mhap_group_rank(mhap_group* g, int32_t rank);         /* for per-rank set-up (filters) and counters */
const char* mhap_group_last_error(const mhap_group* g);
/* AbstractMatchSearch.addData over N GPUs: read i of this call goes to rank (reads added so far + i) % N; the ranks sketch and
 * index their shares concurrently.  May be called repeatedly (batches of one file, several files). */
int mhap_group_add_reads(mhap_group* g, const char* bases, const int64_t* offsets, const int32_t* lengths, const int64_t* ids, int64_t n);
int mhap_group_clear(mhap_group* g);
/* mhap_index_add_scan over the ranks: record i of the scan goes to rank (reads added so far + i) % N; every rank runs its own
 * pack / upload / sketch pipeline over its share of the mapped text */
int mhap_group_add_scan(mhap_group* g, const mhap_fasta_scan* s);
/* findMatches() / findMatches(streamer) over the sharded index; the sink is called from the ranks' threads, one call at a time. */
int mhap_group_find_matches_self(mhap_group* g, mhap_record_sink sink, void* user);
int mhap_group_find_matches_reads(mhap_group* g, const char* bases, const int64_t* offsets, const int32_t* lengths, const int64_t* ids,
                                  int64_t n, mhap_record_sink sink, void* user);
/* counters summed over the ranks, except queries_searched: that sum divided by N.  The division is exact: every rank probes every
 * gathered row that carries a sketch, and no rank counts a padding row or an unsketched read.  candidates_compared and table_elements
 * add up to what one index of all the reads counts (a stored strand and its postings are on exactly one rank). */
int mhap_group_get_stats(mhap_group* g, mhap_stats* sum);

int mhap_get_stats(mhap_handle* h, mhap_stats* out);
int mhap_get_kernel_times(mhap_handle* h, mhap_kernel_times* out);
int mhap_reset_kernel_times(mhap_handle* h);
/* Use an externally created hipStream_t (e.g. torch's current stream); NULL = library stream.  The call first waits for the work
 * the handle queued on the stream it leaves.  Ordering a caller may rely on: the library's kernels are queued on the given stream, so
 * they run behind whatever the caller queued there before the call, and every entry point returns only once its own work on the
 * stream is complete.  Nothing else is ordered: the meta words of caller-owned tables (mhap_index_set_device,
 * mhap_find_matches_device) and the copies of mhap_index_export are read outside that stream, and work on the caller's OTHER
 * streams is never waited for — such buffers must be complete before the call (the ordered rows excepted, see mhap_index_prepare and
 * mhap_set_second_stage_gate). */
int mhap_set_stream(mhap_handle* h, void* hip_stream);
int mhap_synchronize(mhap_handle* h);

/* ---- host-side helpers (no GPU): the reference's IO conventions --------------------------- */

/* Java String.format("%s %s %.6f %.6f %d %d %d %d %d %d %d %d") of MatchResult.toString
 * (J/impl/MatchResult.java:98-113) with numeric headers; returns bytes written (no NUL counted). */
int mhap_format_record(const mhap_record* r, char* out, size_t cap);

/* FASTA ingest with FastaData semantics (J/impl/FastaData.java:125-204): lines concatenated,
 * upper-cased, ids = 1-based running count of non-empty records (+id_offset).  The returned
 * object owns the arrays; free with mhap_fasta_free. */
typedef struct mhap_fasta {
  char* bases; int64_t* offsets; int32_t* lengths; int64_t* ids; int64_t n; int64_t total_bases;
  char* headers;            /* n NUL-terminated names back to back: the header line after '>' up to the first white space or comma
                               (what --store-full-id prints, FastaData.java:155-156) */
  int64_t headers_bytes;
} mhap_fasta;
int mhap_fasta_read(const char* path, int64_t id_offset, mhap_fasta* out, char* err, size_t errcap);
void mhap_fasta_free(mhap_fasta* f);

/* FASTQ input.  Both readers above (mhap_fasta_read, mhap_fasta_scan_open) take a file whose first byte, after gz / bz2 inflation, is
 * '@' for FASTQ; the plain-text suffixes "fastq" and "fq" join FastaData's.  A file that begins with '>' is read as before.
 *   Record grammar.  A header line that opens with '@'; sequence lines up to a line that begins with '+', whose rest is ignored;
 *   quality lines until as many quality bytes are read as the record has sequence bytes — so a record may span several lines, and a
 *   quality line may begin with '@' or '+'.  Line ends are the FASTA reader's: \n, \r, \r\n.
 *   What a record gives is what its FASTA twin (">name" and the sequence) gives: upper-cased bases, ids as the 1-based count of non-empty
 *   records + id_offset, the name after '@' up to the first white space or comma, lengths, offsets and the pure-ACGT flag.
 *   Qualities.  Phred = byte - 33, 0 .. 93, one per base in the reads' order; they come through the entry points below and
 *   mhap_fasta_scan_has_qualities / mhap_fasta_scan_qualities, never through mhap_fasta.  The streamed ingest packs bases as before
 *   and uploads no qualities: the search does not use them.
 *   Refused with MHAP_E_INVALID and one line that names the record, counted from 1 with empty records: a record that does not start
 *   with '@', one without a '+' line, a file that ends before a record's qualities are complete, a quality line that runs past the
 *   sequence length, a quality byte outside 33 .. 126.
 * mhap_fasta_read_qualities is mhap_fasta_read that also returns the quality array (total_bases bytes, free with
 * mhap_qualities_free); *qualities is NULL for a FASTA file. */
int mhap_fasta_read_qualities(const char* path, int64_t id_offset, mhap_fasta* out, uint8_t** qualities, char* err, size_t errcap);
void mhap_qualities_free(uint8_t* qualities);

/* Batched local alignment on the GPU: the Smith-Waterman check of EstimateROC's computeDP (J/main/EstimateROC.java:746-800), SSW's
 * scoring as EstimateROC calls it (Aligner.align(s1, s2, MATCH_MATRIX, 2, 1, true), matrix :302-308).  bases: the reads' bytes as
 * mhap_fasta holds them (upper-cased); pairs: n rows of 5 int64 {a_off, a_len, b_off, b_len, b_rc}.  s1 = bases[a_off, a_off + a_len),
 * s2 = bases[b_off, b_off + b_len), reverse-complemented through Utils.rc's table (J/utils/Utils.java:496-507) when b_rc != 0.
 *   substitution +2 when the two bytes are equal (N against N too), -2 otherwise; a gap of length L costs 2 + (L - 1):
 *   E(i,j) = max(H(i,j-1) - 2, E(i,j-1) - 1)   deletion, consumes s2        H(i,j) = max(0, H(i-1,j-1) + sub, E(i,j), F(i,j))
 *   F(i,j) = max(H(i-1,j) - 2, F(i-1,j) - 1)   insertion, consumes s1
 * The path rules are this project's (SSW's cigar comes from a second banded pass; parity with it is not pinned):
 *   end cell: the maximum H; on ties the smallest j (position in s2), then the smallest i;
 *   predecessors: H prefers the diagonal, then E, then F; E and F prefer extension over opening on ties;
 *   a cell with H = 0 ends every path through it; an alignment begins at a diagonal step out of an H = 0 cell.
 * results: n rows of 7 int32 {score, read_begin, read_end, ref_begin, ref_end, columns, errors}; read_* are 0-based inclusive rows of s1,
 * ref_* columns of s2 (as SSW reports read_begin1 ... ref_end1); columns = M + I + D of the path, errors = mismatched M columns + I + D.
 * A pair without a positive cell (an empty segment included) gives {0, -1, -1, -1, -1, 0, 0}.  MHAP_E_INVALID for a segment outside
 * the n_bases bases. */
int mhap_align_pairs(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t* results);

/* ---- the realignment stage: aligned ends and a counted identity for reported overlaps -------- */

/* mhap_align_pairs inside a band.  pairs: n rows of 7 int64 {a_off, a_len, b_off, b_len, b_rc, diag, band}; the first five as above.
 * With i the 0-based position in s1 and j the 0-based position in s2 (after the reverse complement when b_rc), cell (i, j) is in the
 * band iff |j - i - diag| <= band.  The contract is mhap_align_pairs' with one sentence added:
 *   a cell outside the band has H = 0 and E = F = -infinity and carries nothing.
 * (A diagonal step never leaves the band, and an E or F that opens from an out-of-band H = 0 is negative, so the band's edge needs no
 * rule of its own.)  When every cell of the matrix is in the band the seven result fields equal mhap_align_pairs' on the same pair; a
 * band that misses the matrix, or an empty segment, gives {0, -1, -1, -1, -1, 0, 0}.  MHAP_E_INVALID, with the pair's index in the
 * message, for band < 0 or a segment outside the n_bases bases.  Work and memory follow the band clipped to the matrix, not the
 * matrix (realign_kernels.hip). */
int mhap_align_pairs_banded(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs /* n x 7 */, int64_t n,
                            int32_t* results /* n x 7 */);

/* Overlap records -> banded pairs (no GPU).  The reads are (read_ids[r], offsets[r], lengths[r]) into one array of bases; a record's
 * reads are found by id through a host map.  Per record: s1 = the whole `from` read, s2 = the whole `to` read, b_rc = to_rc.
 * MatchResult's flip (J/impl/MatchResult.java:56-57) is undone when to_rc: b1' = blen - b2 - 1, b2' = blen - b1 - 1, else b1' = b1,
 * b2' = b2.  diag = floor(((b1' + b2') - (a1 + a2)) / 2), floor toward -infinity.  band > 0: that value; band = 0 (automatic):
 * max(1, (int)(max(a2 - a1, b2' - b1') * max_shift)), the tolerance the second stage applies around its median shift
 * (J/sketch/BottomOverlapSketch.java:205).  MHAP_E_INVALID for a record whose id is not among read_ids or whose alen / blen disagree
 * with the read's length; the message, which names the record, is mhap_realign_plan_error() of the calling thread. */
int mhap_realign_plan(const mhap_record* recs, int64_t n, const int64_t* read_ids, const int64_t* offsets, const int32_t* lengths,
                      int64_t n_reads, double max_shift, int32_t band /* 0 = auto */, int64_t* pairs /* n x 7 */);
const char* mhap_realign_plan_error(void);

/* Plan, align in the band and convert back.  The automatic band (band = 0) uses the max_shift of the handle's parameters.  out[q]:
 * ids, alen, blen, to_rc and raw copied from recs[q]; a1 = read_begin, a2 = read_end; b1, b2 = ref_begin, ref_end, flipped back when
 * to_rc; score = 1.0 - (double)errors / columns.  detail (may be NULL): n rows of 3 int32 {score, columns, errors} of the alignment.
 * A record without an alignment comes back with score 0, the four positions 0 and a detail row of zeros: the caller decides what to do
 * with it.  The bases are uploaded once; records go through the kernel 65 536 at a time, so device memory besides the bases is 88
 * bytes per record of a batch plus at most 1 GiB of pass boundaries, whatever n is.  Errors as mhap_realign_plan (message:
 * mhap_last_error) and mhap_align_pairs_banded. */
int mhap_realign_records(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                         const int32_t* lengths, int64_t n_reads, const mhap_record* recs, int64_t n, int32_t band,
                         mhap_record* out, int32_t* detail /* n x 3: score, columns, errors; may be NULL */);

/* ---- the realignment stage's paths: each alignment column by column, and PAF ---------------- */

/* The path of a banded alignment is the one whose begin cell, columns and errors mhap_align_pairs_banded reports; no rule is added.  It
 * is read off the recurrences above, starting at the reported end cell in state H:
 *   in H at (i, j): H = 0 stops.  With D = H(i-1, j-1) + sub: the diagonal when D > 0, D >= E(i,j) and D >= F(i,j); otherwise state E
 *     when E(i,j) > 0 and E(i,j) >= F(i,j); otherwise state F;
 *   in E at (i, j): the column consumes s2 only; the predecessor is E at (i, j-1) when E(i,j-1) - 1 >= H(i,j-1) - 2, else H at (i, j-1);
 *   in F at (i, j): the column consumes s1 only; the predecessor is F at (i-1, j) when F(i-1,j) - 1 >= H(i-1,j) - 2, else H at (i-1, j);
 *   a cell outside the band has H = 0 and E = F = -infinity, so a path never enters it.
 * A path is a list of uint32 runs, len << 4 | code, in order from the begin cell to the end cell, with BAM's codes: 7 '=' a diagonal
 * column on equal bytes, 8 'X' a diagonal column on different bytes, 1 'I' an F column (consumes s1 only), 2 'D' an E column (consumes
 * s2 only).  len >= 1 and adjacent runs have different codes, except that a run longer than 2^28 - 1 is split into several runs of
 * its code.  s2 is the reverse complement of the stored segment when b_rc, and the path is in that orientation.  A pair without an
 * alignment has no runs.  It follows that the lengths of '=', 'X', 'I' sum to read_end - read_begin + 1, those of '=', 'X', 'D' to
 * ref_end - ref_begin + 1, all of them to `columns`, those of 'X', 'I', 'D' to `errors`, that the first and the last run are '=', and
 * that +2 per '=' column, -2 per 'X' column and -(2 + (L - 1)) per gap of L columns sum to `score`.
 *
 * mhap_align_pairs_banded_paths: mhap_align_pairs_banded (same arguments, same errors, byte-identical results) and the paths of all
 * pairs in a library-owned object: *out on success, NULL on any error.  The direction of every cell the path can have visited is kept
 * on the device, 4 bits per cell, for a group of pairs at a time: at most 2 GiB of them, or MHAP_REALIGN_TRACE_BYTES bytes (the
 * environment, read at each call); a pair that needs more goes alone, and when that cannot be allocated the call fails with
 * MHAP_E_HIP, the pair's index in the message, and returns nothing. */
typedef struct mhap_align_paths mhap_align_paths;
int mhap_align_pairs_banded_paths(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs /* n x 7 */, int64_t n,
                                  int32_t* results /* n x 7 */, mhap_align_paths** out);
/* mhap_realign_records (same arguments, same errors, byte-identical out and detail) and the path of every record's planned pair:
 * record q's runs are those of the pair mhap_realign_plan gives it, so on a to_rc record they run along the reverse complement of
 * the `to` read.  A record without an alignment has no runs. */
int mhap_realign_records_paths(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                               const int32_t* lengths, int64_t n_reads, const mhap_record* recs, int64_t n, int32_t band,
                               mhap_record* out, int32_t* detail /* may be NULL */, mhap_align_paths** paths);
/* n = the pairs (records) of the call, n_ops = all their runs; either pointer may be NULL */
int mhap_align_paths_info(const mhap_align_paths* p, int64_t* n, int64_t* n_ops);
/* pair q's runs are ops[op_offsets[q] .. op_offsets[q + 1]) */
int mhap_align_paths_copy(const mhap_align_paths* p, int64_t* op_offsets /* n + 1 */, uint32_t* ops /* n_ops */);
void mhap_align_paths_free(mhap_align_paths* p);

/* One PAF line of a realigned record (no GPU), tab-separated, no newline:
 *   qname qlen qstart qend strand tname tlen tstart tend nmatch alnlen 255 NM:i:<errors> AS:i:<score> cg:Z:<cigar>
 * qlen = alen, qstart = a1, qend = a2 + 1, tlen = blen, tstart = b1, tend = b2 + 1 (b1, b2 of the realigned record are on the `to`
 * read's own strand), strand '-' when to_rc, nmatch = columns - errors, alnlen = columns; detail3 = the record's {score, columns,
 * errors}.  cg:Z writes the runs with the letters = X I D: in path order on '+', in reverse order on '-' (PAF's CIGAR runs along the
 * target's forward strand with the query reverse-complemented, and no operation changes when both sequences are reverse-complemented).
 * snprintf semantics: returns the line's length; when cap is too small the line is truncated (NUL-terminated when cap > 0) and the
 * length needed is returned.  -1 for a null record, detail or name, or ops missing with n_ops > 0. */
int mhap_format_paf(const mhap_record* realigned, const int32_t* detail3, const uint32_t* ops, int64_t n_ops, const char* qname,
                    const char* tname, char* out, size_t cap);

/* A paths object from runs the caller holds (no GPU): pair q's runs are ops[op_offsets[q] .. op_offsets[q + 1]), op_offsets[0] = 0 and
 * non-decreasing.  What mhap_align_paths_copy wrote gives back an equal object; freed with mhap_align_paths_free.  MHAP_E_INVALID (and
 * *out = NULL) for a null pointer, n < 0 or offsets that are not such a list. */
int mhap_align_paths_from_runs(const int64_t* op_offsets /* n + 1 */, int64_t n, const uint32_t* ops, mhap_align_paths** out);

/* ---- read correction: a pile-up vote over every read from the realigned overlaps' paths, and a majority call ---------------------- */

/* The plain method: every realigned overlap votes column by column on both of its reads, and each read position takes the majority.
 * No partial-order graph and no cap on coverage; which views vote is the caller's choice (mhap_correct_add_views, with the bytes
 * that "overlap selection" below makes: each read's best views, one round, for this stage only).  A, C, G, T below are the upper-case bytes; bytes are the ones
 * the aligner compared (s2 is the reverse complement, through Utils.rc's table, of the stored `to` read when to_rc).
 *
 * Which records vote.  A realigned record is out[q] of mhap_realign_records_paths with its runs: s1 = read A (`from`), rows i from
 * a1; s2 = read B (`to`), reverse-complemented when to_rc, columns j from (to_rc ? blen - b2 - 1 : b1).  A record without runs (no
 * alignment) votes nothing, a record whose two ids are equal votes nothing, and nothing is de-duplicated: a record given twice votes
 * twice.  Every other record votes twice, once per view; a view is a list of columns in increasing target order:
 *   view A (target A, evidence B):   '=' / 'X' -> M(t = i, e = s2[j]);   'I' (consumes s1 only) -> Del(t = i);   'D' -> Ins(e = s2[j])
 *   view B (target B, evidence A), !to_rc:   '=' / 'X' -> M(t = j, e = s1[i]);   'D' -> Del(t = j);   'I' -> Ins(e = s1[i])
 *   view B, to_rc: the !to_rc list in reverse order, every t replaced by blen - 1 - t and every e by its complement through the same
 *     table (a byte the table does not change stays what it is).
 * Paths begin and end with '=', so every group of consecutive Ins columns lies between two target-consuming columns and belongs to the
 * target position t of the one before it (in the view's order).
 *
 * Votes.  22 counters per target position t: base[4] (A, C, G, T), del, span, ins[KI = 4][4].
 *   M(t, e) adds 1 to base[t][e] when e is A, C, G or T, else nothing;   Del(t) adds 1 to del[t];
 *   for every two consecutive target-consuming columns t, t' of a view, span[t] += 1 (the view continues past t);
 *   in the Ins group after t the k-th byte (k from 0) adds 1 to ins[t][k][e] when k < 4 and e is A, C, G or T; any other byte votes
 *   nothing but still takes its slot.
 * Counters are 16 bits wide, two to a 32-bit word, so that a vote is one integer atomic add of 1 or 1 << 16: with 2 spare counters
 * that is 24 counters, 48 bytes per base of the read set, resident on the device from begin to free.  The width is exact because the
 * host counts the views it accepts per target, in arrival order (record by record, view A before view B): a view adds at most 1 to
 * any counter, and a view whose target already has 65 535 accepted views is skipped whole and counted in skipped_views.  Integer sums
 * do not depend on arrival order, so the result is the same from run to run and however the records are split over calls.
 *
 * The call for a read of length L, with min_cov (4 unless the caller says otherwise) and own = the read's byte at t, for t = 0 .. L - 1:
 *   1. d = base[t][A] + base[t][C] + base[t][G] + base[t][T] + del[t].
 *   2. d < min_cov: emit own and count the position as low.
 *   3. Otherwise add 1 to base[t][own] when own is A, C, G or T, and total = d + 1.
 *   4. 2 del[t] > total: emit nothing and count a deletion.
 *   5. Otherwise emit the base with the most votes: own when it is among those tied for the maximum, else the first of A, C, G, T at
 *      the maximum, own itself when every base count is 0; count a substitution when the emitted byte differs from own.
 *   6. Whatever 2 - 5 did: when t < L - 1 and span[t] >= min_cov, for k = 0 .. 3 with m = max over b of ins[t][k][b]: 2 m > span[t] + 1
 *      emits that base (the first of A, C, G, T at the maximum) and counts an insertion; otherwise the junction is done.
 * Per read the result is the corrected bytes and six int32 {len_in, len_out, n_sub, n_del, n_ins, n_low}; a read nobody voted on
 * comes back unchanged with n_low = len_in.
 *
 * The session.  mhap_correct_begin uploads the bases of the reads (read_ids[r], offsets[r], lengths[r]) once and allocates and zeroes
 * the vote table; the handle must outlive the session, whose errors are the handle's (mhap_last_error).  mhap_correct_add takes the
 * realigned records and the paths object of one mhap_realign_records_paths call (or mhap_align_paths_from_runs), any number of times,
 * n = 0 included; the runs go up again, 4 bytes each, and one wave per accepted view adds its votes (correct_kernels.hip).  A record's
 * reads are found by id as mhap_realign_plan finds them; MHAP_E_INVALID, naming the record, for an id not among read_ids, an alen or
 * blen that disagrees with the read's length, a paths object of another n, runs that are not a path between (a1, the first column)
 * and (a2, the last) beginning and ending with '=', or two adjacent runs of one code unless the earlier one has the length 2^28 - 1
 * (a split run, the paths' own rule above: the vote takes the later run for the continuation of the earlier, so a hand-made path
 * that merely repeats a code would vote differently from the columns it spells); a refused call has cast no vote.
 * mhap_correct_finish makes the call for every read on the device (min_cov >= 1) and returns out_offsets (read r's corrected bytes
 * are [out_offsets[r], out_offsets[r + 1]) of the output), the six counts per read and the views skipped so far; it may be repeated,
 * and more records may be added after it.
 * mhap_correct_copy writes the out_offsets[n_reads] bytes of the last finish.  Votes cross to the host only through
 * mhap_correct_votes: the 24 counters of every position of read read_index (its position in read_ids), position-major, in the order
 * base A C G T, del, span, ins[0] A C G T, ins[1] .., ins[2] .., ins[3] .., and the two spare ones, which stay 0. */
typedef struct mhap_correct_session mhap_correct_session;
int mhap_correct_begin(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                       const int32_t* lengths, int64_t n_reads, mhap_correct_session** session);
int mhap_correct_add(mhap_correct_session* s, const mhap_record* realigned, int64_t n, const mhap_align_paths* paths);
/* mhap_correct_add with one byte per record that says which of its views vote ("overlap selection" below makes them): bit 0 view A,
 * bit 1 view B; views == NULL is mhap_correct_add.  A view whose bit is clear casts no vote, does not count towards its target's
 * 65 535 views and is not a skipped view; every check of the record runs all the same. */
int mhap_correct_add_views(mhap_correct_session* s, const mhap_record* realigned, int64_t n, const mhap_align_paths* paths,
                           const uint8_t* views /* n, or NULL */);
int mhap_correct_finish(mhap_correct_session* s, int32_t min_cov, int64_t* out_offsets /* n_reads + 1 */, int32_t* stats /* n_reads x 6 */,
                        int64_t* skipped_views);
int mhap_correct_copy(mhap_correct_session* s, uint8_t* bytes);
int mhap_correct_votes(mhap_correct_session* s, int64_t read_index, uint16_t* counters /* length x 24 */);
void mhap_correct_free(mhap_correct_session* s);

/* ---- string graph: dovetails, contained reads and transitive reduction over the realigned overlaps, and GFA ------------------------- */

/* The layout step that follows an overlapper (Myers 2005): every realigned overlap is classed, contained reads are set aside, the
 * dovetails become the arcs of a bidirected graph and the arcs that a two-arc path explains are removed.  Tips and simple bubbles are
 * removed on request ("graph cleaning" below).  Reads are trimmed and chimeras split in a stage of their own in front of this one ("read trimming" below), whose reads and records this one takes unchanged.  Everything is integer arithmetic (sums and products of lengths in
 * int64); the only floating comparison is score < min_identity on the record's double.
 *
 * Input.  A table of reads (read_ids[r], lengths[r]; no bases), realigned records (out[q] of mhap_realign_records) and the parameters
 * max_hang (1000), int_frac_permille (800), min_ovlp (2000), fuzz (1000), min_identity (0.0).
 *
 * Vertices.  Read r (its position in read_ids) has the vertices 2 r (forward) and 2 r + 1 (reverse complement); v ^ 1 is the other strand.
 *
 * The class of a record.  qs = a1, qe = a2 + 1, ql = alen, tl = blen; (ts, te) = (b1, b2 + 1) when !to_rc, else (tl - b2 - 1, tl - b1):
 * the `to` read as aligned; tl5 = ts, tl3 = tl - te; ext5 = min(qs, tl5), ext3 = min(ql - qe, tl3).  The first rule that holds:
 *   0 NONE         from_id == to_id, or score == 0 (no alignment), or score < min_identity;
 *   1 INTERNAL     ext5 > max_hang, or ext3 > max_hang, or (qe - qs) * 1000 < (qe - qs + ext5 + ext3) * int_frac_permille;
 *   2 A_CONTAINED  qs <= tl5 and ql - qe <= tl3: the `from` read is contained;
 *   3 B_CONTAINED  qs >= tl5 and ql - qe >= tl3: the `to` read is contained;
 *   4 SHORT        qe - qs + ext5 + ext3 < min_ovlp, or te - ts + ext5 + ext3 < min_ovlp;
 *   5 DOVETAIL     everything else (both inequalities are strict here).
 * A dovetail gives two arcs (u, v, len); with A, B the two reads' positions in read_ids and o = to_rc (0 or 1):
 *   qs > tl5:    (2 A, 2 B + o, qs - tl5)   and  (2 B + (1 - o), 2 A + 1, tl3 - (ql - qe));
 *   otherwise:   (2 B + o, 2 A, tl5 - qs)   and  (2 A + 1, 2 B + (1 - o), (ql - qe) - tl3).
 * len is how far v begins after u begins; ol = length(read(u)) - len is the overlap the arc stands for.
 *
 * Contained reads.  A read is contained when any record classes it so, and every arc with a contained read at either end is dropped.
 *
 * The arc list.  The surviving arcs sorted by (u, len, v); of the arcs with equal (u, v) only the first is kept.  An arc's q is the
 * arrival index (over all adds, from 0) of a record that produced a kept arc's (u, v, len): a label, on which nothing else depends.
 * The complement of u -> v is v ^ 1 -> u ^ 1; a record gives an arc and its complement, so the complement is always in the list.
 *
 * Reduction.  Every vertex is reduced on its own, on the de-duplicated list as it is before any reduction.  For vertex v with the
 * arcs v -> w_i in list order:
 *   1. every w_i is IN_PLAY;   2. longest = len(the last arc) + fuzz;
 *   3. pass 1, over i in order: skip w_i unless it is still IN_PLAY; the arcs w_i -> x in list order, stopping at the first with
 *      len(v -> w_i) + len(w_i -> x) > longest: an x that is IN_PLAY becomes ELIMINATED;
 *   4. pass 2, over every i whatever its mark: of the arcs w_i -> x in list order the first, then every arc with len < fuzz, stopping
 *      at the first later arc with len >= fuzz: an x that is IN_PLAY becomes ELIMINATED;
 *   5. the arcs v -> w with w ELIMINATED are `reduced`.
 * The final arcs are those that are not reduced and whose complement is not reduced.
 *
 * Results.  The class of every record (one byte, in arrival order), a contained flag per read, the arc list as rows of 7 int32
 * {u, v, len, ol, q, reduced, final}, and MHAP_GRAPH_COUNTS int64 counts: records, the six classes in the order above, contained
 * reads, arcs, reduced arcs, final arcs.  Everything except the q labels and the order of the per-record classes is invariant under
 * any permutation of the records and any split of them over calls.
 *
 * The session.  mhap_graph_begin takes the table of reads (params NULL: the defaults); the handle must outlive the session, whose
 * errors are the handle's (mhap_last_error).  mhap_graph_add classes the records on the device (graph_kernels.hip), any number of
 * times, n = 0 included, and does not wait for the device.  A record's reads are found by id as mhap_realign_plan finds them;
 * MHAP_E_INVALID, naming the record, for an id not among read_ids or an alen / blen that disagrees with the table; a refused call
 * adds nothing.  mhap_graph_finish builds the list, reduces it and returns the counts; it may be repeated, and more records may be
 * added after it.  mhap_graph_info: the reads, the records added so far and the arcs of the last finish (-1 before the first); any
 * pointer may be NULL.  mhap_graph_copy_arcs writes the rows of the last finish, mhap_graph_copy_classes one byte per record added
 * so far, mhap_graph_copy_read_flags one byte (0 / 1) per read.  Device memory: 33 bytes per record and 8 per read from begin to
 * free, and from the first finish on 48 more per read and 73 per surviving arc.
 *
 * GFA 1.  `H\tVN:Z:1.0`, then `S\t<id>\t*\tLN:i:<length>` for every read that is not contained, in read_ids order, then one L line per
 * final arc in list order; every line ends with '\n' and ids are numeric.  The text depends on the set of records only.
 * mhap_format_gfa_link (no GPU) writes the L line of one row, `L\t<id(u)>\t<+|->\t<id(v)>\t<+|->\t<ol>M` without the newline, '-' for
 * an odd vertex: snprintf semantics as mhap_format_paf; -1 for a null pointer.
 *
 * ---- unitigs: the final arcs compacted into chains, with their sequences -----------------------------------------------------------
 * Tips and simple bubbles go only when mhap_graph_clean is called ("graph cleaning" below); chimera detection is not part of this.  A
 * unitig is spelled from the reads as stored (the correction stage may be run before); the consensus over a unitig's reads is a
 * stage of its own behind this one ("unitig consensus" below).  Integer arithmetic; offsets and lengths in bases are int64.
 *
 * Input.  The state of a session after a mhap_graph_finish: the arc list with its `final` flags, the contained flags, the read
 * lengths.  Only final arcs count.  `final` is symmetric (u -> v is final exactly when v ^ 1 -> u ^ 1 is), so in-degree(v) =
 * out-degree(v ^ 1); no arc joins the two strands of one read (such a record classes as NONE).
 *
 * Joined arcs.  next(v) = w when v has exactly one final out-arc v -> w and w ^ 1 has exactly one final out-arc (w has in-degree 1);
 * otherwise v has no next.  prev is the inverse of next, and next(v) = w <=> next(w ^ 1) = v ^ 1.  A contained read has no vertices
 * here; every other read has both of its vertices in play, a read that no arc touches included.
 *
 * Unitigs.  The maximal chains of next, and the cycles of next.  Every chain has a twin, its reverse complement (the vertices ^ 1 in
 * reverse order), with which it shares no read.  A linear chain is kept in the orientation with head < tail ^ 1; a cycle in the
 * orientation that holds the smallest vertex number of the cycle and its twin, and it starts at that vertex.  Unitigs are numbered
 * from 0 in ascending order of their first vertex, linear and circular together.
 *
 * Layout.  Member i of a unitig is a vertex v_i with span_i: the len of the joined arc v_i -> v_i+1; for the last member of a circular
 * unitig the len of the closing arc back to member 0; for the last member of a linear unitig the whole read length.  offset_i is the
 * sum of the spans before it, the unitig's length the sum of all its spans.  (1 <= len < length(read(u)) for every arc, so a span
 * never exceeds its read.)
 *
 * Sequence.  For each member in order, the first span_i bytes of its read in the member's orientation, concatenated: an even vertex
 * uses the stored bytes, an odd vertex the reverse complement through the table of Utils.rc that the realignment and correction
 * kernels use for to_rc reads (upper-cased, complemented; a byte the table does not know stays as it is).
 *
 * Links.  Every final arc that is not a joined arc; it leaves the tail of a unitig or of a twin and enters the head of a unitig or
 * of a twin.  A row is 6 int32 {from_unitig, from_orient, to_unitig, to_orient, ol, arc}: orient 0 is the kept orientation, 1 the
 * twin, arc the index in the arc list.  Links are in arc-list order; circular unitigs have none.
 *
 * Counts.  MHAP_UNITIG_COUNTS int64: unitigs, circular unitigs, members, joined arcs, links, bases of the longest unitig, bases of
 * all unitigs.  Everything above depends on the set of records only, not on their order or their split over adds.
 *
 * The calls.  mhap_graph_unitigs needs a completed finish with no record added after it (MHAP_E_INVALID otherwise) and builds
 * everything anew on the device (graph_kernels.hip: one lane per vertex for next / prev / span; list ranking by pointer doubling,
 * ceil(log2(max(2, vertices in play))) rounds queued without a host wait, once for the chains, once to carry a cycle's smallest
 * vertex round it and once for the cycles cut there; numbering and placement by prefix sums, no ordering by atomics).  A later
 * mhap_graph_finish invalidates the unitigs: the copy and spell calls return MHAP_E_INVALID until mhap_graph_unitigs has run again.
 * mhap_graph_unitigs_info: the sizes the copy calls need (n_unitigs -1 while invalid); any pointer may be NULL.
 * mhap_graph_copy_unitigs: member k's of unitig i are unitig_start[i] .. unitig_start[i + 1].  mhap_graph_spell writes the sequences
 * of all unitigs back to back (unitig i at the sum of the lengths before it); read r's bytes are bases[offsets[r], offsets[r] +
 * lengths[r]), and a read outside the n_bases bases refuses the call with a message.  mhap_graph_spell_device is the same with
 * `bases` already on the handle's device (offsets and out on the host).  The spelling kernel runs over tiles of MHAP_SPELL_CHUNK
 * output bytes, which find their members by binary search, so neither a long read nor a run of short spans serialises; every
 * output byte has exactly one writer.  Device memory, from the first mhap_graph_unitigs to mhap_graph_free: 130 bytes per vertex
 * (two per read), 12 per arc, 24 per member, 17 per unitig, 24 per link; the spell calls add 8 per read, the output, and
 * mhap_graph_spell the bases.
 *
 * GFA 1 of the unitig graph (a second text: the one above is unchanged).  `H\tVN:Z:1.0`; per unitig k
 * `S\tutg%06d{l|c}\t<sequence>\tLN:i:<length>\tnr:i:<members>` with the number k + 1 and l for linear, c for circular, followed by
 * its members as `a\t<utg name>\t<offset>\t<read id>:1-<span>\t<+|->\t<span>`; last one `L\t<utg>\t<+|->\t<utg>\t<+|->\t<ol>M` per link in
 * link order ('-' for the twin).  Every line ends with '\n'.  mhap_format_gfa_unitig_link (no GPU) writes the L line of one link row
 * without the newline: snprintf semantics, -1 for a null pointer.
 *
 * ---- graph cleaning: tips clipped and simple bubbles popped, in rounds ---------------------------------------------------------------
 * An opt-in stage behind mhap_graph_finish: short dead-end branches (a missed overlap, a read with a bad end) and two-path bubbles (a
 * local disagreement) are removed, so that unitigs run through where they were.  Integer only; it depends on the set of records only.
 * It is defined on the unitig graph of a snapshot: every decision of a round is a function of that round's tables alone, never of
 * another decision of the same round.  Not done: read trimming, chimera detection, bubbles that are not simple.
 *
 * State.  A `dropped` byte per read (0 in play, 1 tip, 2 bubble) and a `removed` byte per arc of the list (1 when the arc is final
 * and either of its reads is dropped); all zero when a cleaning begins.
 *
 * A round.  The unitigs are built exactly as above with two changes: a dropped read has no vertices, as a contained read has none,
 * and only the final arcs that are not removed count.  An oriented unitig is (X, o): o = 0 the kept orientation, 1 the twin.  The
 * out-links of (X, o) are the link rows that leave it; its in-links from (W, w) are exactly the out-links (X, 1 - o) -> (W, 1 - w),
 * every link's complement being in the table.  rank(X) = (members, bases, -number), compared lexicographically: two different
 * unitigs never tie.
 *
 * Tips.  (T, o) is a tip candidate when T is linear, members(T) <= tip_reads, (T, o) has no in-link and at least one out-link; so in
 * at most one orientation, and an isolated chain, a lone read or a circular unitig never is one.  A candidate is removed when every
 * target (J, j) of its out-links has a holder: an in-link from some (W, w) with W != T where (W, w) is no tip candidate or
 * rank(W) > rank(T).  A junction thus keeps its best way in, and a terminal fork loses only its lesser arms.
 *
 * Bubbles.  (B, o) is a branch between (S, s) and (E, e) when B is linear, bases(B) <= bubble_bases, (B, o) has exactly one in-link,
 * from (S, s), and exactly one out-link, to (E, e), and B is neither S nor E.  A branch is removed when a branch (B', o') of another
 * unitig between the same (S, s) and (E, e) has rank(B') > rank(B).  S may have any number of out-links; only such simple bubbles
 * are popped.  The twin (B, 1 - o) is a branch between (E, 1 - e) and (S, 1 - s) with the same siblings: one verdict from either side.
 *
 * Applying a round.  Every member read of a removed unitig gets dropped = 1 (tip) or 2 (bubble) — no unitig is both, a tip having no
 * in-link — and `removed` is computed again.  Rounds repeat until one removes nothing or max_rounds have run; the count of rounds
 * includes the last, empty one.  Then the unitigs are built once more, from the cleaned graph: the build the copy and spell calls serve.
 *
 * Parameters: tip_reads (4), bubble_bases (50 000), max_rounds (16).  Counts: MHAP_CLEAN_COUNTS int64: rounds, tip unitigs, tip reads,
 * bubble unitigs, bubble reads, arcs removed.
 *
 * The calls.  mhap_graph_clean (params NULL: the defaults) needs a completed finish with no record added after it, as
 * mhap_graph_unitigs does; MHAP_E_INVALID for a negative parameter or max_rounds < 1.  It may be repeated: each call starts again
 * from the uncleaned graph.  After it mhap_graph_unitigs_info, _copy_unitigs, _copy_layout, _copy_links, _spell and _spell_device
 * serve the cleaned unitigs, and mhap_graph_unitigs_counts gives their MHAP_UNITIG_COUNTS (always those of the unitigs now served:
 * of the last mhap_graph_unitigs or mhap_graph_clean, MHAP_E_INVALID while there are none); a link row's `arc` is still the index in the arc list, which does not change (mhap_graph_copy_arcs
 * and its rows are what they were).  mhap_graph_unitigs keeps its meaning: it builds the uncleaned unitigs, which the copy calls then
 * serve again, and does not disturb the two bytes.  mhap_graph_copy_dropped writes one byte per read, mhap_graph_copy_removed one per
 * arc; both return MHAP_E_INVALID before the first clean and after a later mhap_graph_finish, which forgets the clean state and
 * invalidates the unitigs as before.  On the device (graph_kernels.hip) a round is the unitig build and six kernels, one lane per
 * oriented unitig, unitig, member or arc, placed by binary search in the link table, which is in arc-list order; the host waits
 * once per round, for the round's counts.  Device memory, from the first mhap_graph_clean to mhap_graph_free: 20 bytes per read and
 * 1 per arc, and the unitig tables at their largest: 41 bytes per read (a unitig and a member each) and 24 per arc (a link each).
 *
 * GFA.  The text of the cleaned read graph is the GFA 1 text of the string graph without the S lines of dropped reads and the L
 * lines of removed arcs; the text of the cleaned unitig graph is the unitig text of the cleaned unitigs. */
typedef struct mhap_graph_params {
  int32_t max_hang, int_frac_permille, min_ovlp, fuzz;
  double min_identity;
} mhap_graph_params;
#define MHAP_GRAPH_COUNTS 11
typedef struct mhap_graph_session mhap_graph_session;
void mhap_graph_default_params(mhap_graph_params* p);
int mhap_graph_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_graph_params* params,
                     mhap_graph_session** session);
int mhap_graph_add(mhap_graph_session* s, const mhap_record* realigned, int64_t n);
int mhap_graph_finish(mhap_graph_session* s, int64_t* counts /* MHAP_GRAPH_COUNTS */);
int mhap_graph_info(const mhap_graph_session* s, int64_t* n_reads, int64_t* n_records, int64_t* n_arcs);
int mhap_graph_copy_arcs(mhap_graph_session* s, int32_t* rows /* n_arcs x 7 */);
int mhap_graph_copy_classes(mhap_graph_session* s, uint8_t* classes /* n_records */);
int mhap_graph_copy_read_flags(mhap_graph_session* s, uint8_t* flags /* n_reads */);
void mhap_graph_free(mhap_graph_session* s);
int mhap_format_gfa_link(const int32_t* row7, const int64_t* read_ids, char* out, size_t cap);
#define MHAP_UNITIG_COUNTS 7
#define MHAP_SPELL_CHUNK 4096
int mhap_graph_unitigs(mhap_graph_session* s, int64_t* counts /* MHAP_UNITIG_COUNTS */);
int mhap_graph_unitigs_info(const mhap_graph_session* s, int64_t* n_unitigs, int64_t* n_members, int64_t* n_links, int64_t* n_bases);
int mhap_graph_copy_unitigs(mhap_graph_session* s, int64_t* unitig_start /* n + 1 */, int64_t* unitig_len /* n */, uint8_t* circular /* n */);
int mhap_graph_copy_layout(mhap_graph_session* s, int32_t* vertex /* members */, int64_t* offset /* members */, int32_t* span /* members */);
int mhap_graph_copy_links(mhap_graph_session* s, int32_t* rows /* links x 6 */);
int mhap_graph_spell(mhap_graph_session* s, const uint8_t* bases, int64_t n_bases, const int64_t* offsets /* n_reads */, uint8_t* out /* all bases */);
int mhap_graph_spell_device(mhap_graph_session* s, const uint8_t* device_bases, int64_t n_bases, const int64_t* offsets /* n_reads */,
                            uint8_t* out /* all bases */);
int mhap_format_gfa_unitig_link(const int32_t* row6, char* out, size_t cap);
typedef struct mhap_clean_params { int32_t tip_reads, bubble_bases, max_rounds; } mhap_clean_params;
#define MHAP_CLEAN_COUNTS 6
void mhap_graph_default_clean_params(mhap_clean_params* p);
int mhap_graph_clean(mhap_graph_session* s, const mhap_clean_params* params /* NULL: the defaults */, int64_t* counts /* MHAP_CLEAN_COUNTS */);
int mhap_graph_copy_dropped(mhap_graph_session* s, uint8_t* per_read /* n_reads */);
int mhap_graph_copy_removed(mhap_graph_session* s, uint8_t* per_arc /* n_arcs */);
int mhap_graph_unitigs_counts(mhap_graph_session* s, int64_t* counts /* MHAP_UNITIG_COUNTS */);

/* ---- unitig consensus: every read placed on a unitig, aligned to the draft, a pile-up vote and a majority call per draft position ---- */

/* A unitig as spelled carries the error rate of one read at every position, and the contained reads, which hold most of the coverage,
 * contribute nothing.  This stage places every read it can on a served unitig, aligns it to the draft in a band round its place with
 * the banded aligner above, lets every alignment vote as view A of the correction contract ("read correction"), and calls every draft
 * position as that contract calls a read position.  One round; no chimera detection, no read trimming.  Every consensus byte has a
 * quality from its counters ("base qualities" below); the reads' own qualities are not read, and a called deletion reports none.
 *
 * Draft.  The spelling of the unitigs the graph session serves (of the last mhap_graph_unitigs or mhap_graph_clean), exactly what
 * mhap_graph_spell writes; unitig k has the length ulen[k].  A unitig of 2^31 bases or more refuses the run and is named.
 *
 * Placement.  A placement of read X is (unitig, strand, p): X in orientation `strand` (0 as stored, 1 reverse-complemented) begins at
 * draft position p, which may be negative or lie beyond the end.
 *   Members.  Member i of a unitig, vertex v, is placed exactly: on its unitig, strand v & 1, p = offset_i.
 *   Records.  A record places the non-member read X when its class under the graph session's parameters (the rule of "string graph",
 *   the same code) is neither NONE nor INTERNAL, exactly one of its two reads is a member of a served unitig — call it M — and X is
 *   the other.  A member is never placed from a record; contained reads and reads dropped by a cleaning are the non-members that matter.
 *   Frame.  In the aligner's frame A is forward over [qs, qe) and B has strand to_rc over [ts, te) (qs, qe, ts, te as in "string
 *   graph").  When M's strand in that frame differs from M's strand in its unitig (v & 1) the frame is reversed: every interval [s, e)
 *   on a read of length L becomes [L - e, L - s) and both strands flip.  Then M lies over [ms, me) in unitig orientation and X has
 *   strand sX over [xs, xe).
 *   Candidate.  p = floor(((offset_M + ms) + (offset_M + me) - (xs + xe)) / 2) in int64, floor toward -infinity, on M's unitig with
 *   strand sX.
 *   Choice.  Of the qualifying candidates of X: the greatest xe - xs, then the smallest member vertex, then the smallest (p, sX).  The
 *   choice depends on the set of records only, not on their order, their split over adds or their repetition.
 *   A non-member without a qualifying record is unplaced.
 *   Circular unitigs.  p is reduced modulo ulen into [0, ulen), and the unitig is then the linear sequence it is spelled as: a read
 *   that runs over the cut votes only where its best local alignment lies.  No alignment wraps round.
 *
 * Guard.  The counters are 16 bits wide, as in correction, and exact because each placed read casts one view and a view adds at most
 * 1 to any counter: for every tile of MHAP_CONSENSUS_TILE draft positions of a unitig (tile j = positions [j T, (j + 1) T)) the
 * placed reads whose window (below) meets the tile are counted, and a tile above 65 535 refuses the run with MHAP_E_INVALID, the
 * unitig and the tile in the message, before any vote.  MHAP_CONSENSUS_TILE_CAP=c (1 .. 65 534, tests only, read at each run) lowers
 * the 65 535.
 *
 * Plan and align.  One pair per placed read, over one array holding the reads followed by the drafts: band = the given band when
 * > 0, else max(1, (int)(length(X) * max_shift)) with the handle's max_shift; w0 = max(0, p - band), w1 = min(ulen, p + length(X) +
 * band); s1 = draft[w0, w1), s2 = the stored read with b_rc = strand, diag = w0 - p.  The pairs go through
 * mhap_align_pairs_banded_paths' contract, unchanged.  An empty window (w1 <= w0) counts as no alignment; a pair without an
 * alignment votes nothing and is counted.
 *
 * Vote.  One view per aligned pair: view A of the correction contract with the target the unitig and t = w0 + i — M, Del, Ins columns,
 * span, ins[KI = 4][4], only A, C, G, T vote.  24 counters (22 and 2 spare) per draft position, 48 bytes, in the planes of the
 * correction table laid out per unitig; the column walk is the correction kernel's own code.
 *
 * Call.  The six steps of the correction call with own = the draft byte and L = ulen, min_cov from the parameters.  On the device the
 * call runs over tiles of MHAP_CONSENSUS_TILE positions, so a long unitig does not serialise: the junction after t belongs to t's
 * tile, t < L - 1 is the unitig's rule and not the tile's, and every output byte has one writer.
 *
 * Results.  The consensus bytes of all unitigs back to back with out_offsets (n + 1); per unitig six int64 {len_in, len_out, n_sub,
 * n_del, n_ins, n_low}; the placement table, per read five int64 {unitig or -1, strand, p, how (0 member, 1 record, 2 unplaced),
 * aligned 0 / 1}; the position map, one int64 per draft position (unitigs back to back): the bytes its unitig's consensus holds before
 * what this position emits, the exclusive prefix of the emitted lengths; and MHAP_CONSENSUS_COUNTS int64 counts: members, reads placed
 * by a record, unplaced reads, aligned, without alignment, bases in, bases out, substitutions, deletions, insertions, low positions.
 *
 * The session.  mhap_consensus_begin sits on a graph session, which must outlive it, and on that session's handle, whose errors are
 * the session's (mhap_last_error); it keeps the reads' bytes (read r of the graph's table is bases[offsets[r], offsets[r] +
 * lengths[r])) and the parameters (NULL: band 0 = automatic, min_cov 4).  mhap_consensus_add takes the records the graph was given,
 * any number of times, n = 0 included; a record's reads are found and its lengths checked as mhap_graph_add does, a refused call adds
 * nothing, and the records stay on the device, 32 bytes each.  mhap_consensus_run needs served unitigs (MHAP_E_INVALID otherwise), does
 * everything above and returns the counts; it may be repeated, and more records may be added after it.  A mhap_graph_finish,
 * mhap_graph_unitigs or mhap_graph_clean on the graph session after the begin invalidates the consensus session: every call but
 * mhap_consensus_free then returns MHAP_E_INVALID.  mhap_consensus_info: the sizes the copy calls need (n_unitigs -1 before the first
 * completed run).  mhap_consensus_copy, _copy_placements and _copy_map write the results of the last run; mhap_consensus_votes (tests)
 * the 24 counters of every position of one unitig in the order of mhap_correct_votes; mhap_consensus_times the host's wall time of
 * the last run's four stages in seconds: placement (the tables, the draft and the guard included), alignment, vote, call.  Device memory (consensus_kernels.hip has the
 * kernels): 8 bytes per read from begin and 32 per record from the first add on; during and after a run 1 byte per base of the reads, 132 per
 * read, 58 per draft base (the draft, the votes, the map, and one more in the graph session), 32 per tile, the output, 4 per run of
 * a path and 56 per aligned read, besides what the aligner takes for a call. */
typedef struct mhap_consensus_params { int32_t band, min_cov; } mhap_consensus_params;
#define MHAP_CONSENSUS_TILE 4096
#define MHAP_CONSENSUS_COUNTS 11
typedef struct mhap_consensus_session mhap_consensus_session;
void mhap_consensus_default_params(mhap_consensus_params* p);
int mhap_consensus_begin(mhap_graph_session* g, const uint8_t* bases, int64_t n_bases, const int64_t* offsets /* n_reads */,
                         const mhap_consensus_params* params /* NULL: the defaults */, mhap_consensus_session** session);
int mhap_consensus_add(mhap_consensus_session* s, const mhap_record* realigned, int64_t n);
int mhap_consensus_run(mhap_consensus_session* s, int64_t* counts /* MHAP_CONSENSUS_COUNTS */);
int mhap_consensus_info(mhap_consensus_session* s, int64_t* n_unitigs, int64_t* n_reads, int64_t* n_draft_bases, int64_t* n_out_bytes);
int mhap_consensus_copy(mhap_consensus_session* s, uint8_t* bytes /* n_out_bytes */, int64_t* out_offsets /* n_unitigs + 1 */,
                        int64_t* stats /* n_unitigs x 6 */);
int mhap_consensus_copy_placements(mhap_consensus_session* s, int64_t* rows /* n_reads x 5 */);
int mhap_consensus_copy_map(mhap_consensus_session* s, int64_t* map /* n_draft_bases */);
int mhap_consensus_votes(mhap_consensus_session* s, int64_t unitig, uint16_t* counters /* length x 24 */);
int mhap_consensus_times(mhap_consensus_session* s, double* seconds /* 4: placement, alignment, vote, call */);
void mhap_consensus_free(mhap_consensus_session* s);

/* ---- base qualities: how far each corrected or consensus byte can be trusted, from the counters that decided it --------------------- */

/* One quality byte, 0 .. 93, goes with every byte that the call of "read correction" or of "unitig consensus" emits, at the offset of
 * that byte.  It is a function of the position's 24 counters, own, min_cov and the two parameters below, in integer arithmetic only,
 * so it is the same from run to run; tests/quality_ref.py restates it.
 *
 * Parameters.  per_vote: tenths of a Phred unit per net vote, 1 .. 1000; cap: 1 .. 93.  The defaults are {15, 60}: the slope is the
 * one tools/quality_calibration.py measured against a truth genome (12.9, to the nearest 5; EXPERIMENTS.md, "Base qualities"), the cap
 * a convention.
 *
 * Rule.  Q(m) = min(cap, per_vote * max(m, 0) / 10), C integer division.  At position t with the raw counters base[4], del, span,
 * ins[k][4] as the call reads them, d = base[A] + base[C] + base[G] + base[T] + del and n = d + 1 (own counts once):
 *   The base byte, the first byte of a position that is not called deleted, e: not A, C, G or T: quality 0, fixed.  Otherwise
 *     s = base[e] + (own == e ? 1 : 0) and the margin is m = 2 s - n: the votes for e less everything else.  The same in the
 *     low-coverage branch (d < min_cov), where e = own and s = base[own] + 1.
 *   Inserted byte k, e: m = 2 ins[k][e] - (span + 1), positive because the call emitted it.
 *   The stop margin.  The last byte emitted at t also answers for the junction not going on: when t < L - 1 and the position emitted
 *     n_ins < 4 inserted bytes, m_stop = (span + 1) - 2 max over b of ins[n_ins][b], and the last byte's margin becomes min(m, m_stop)
 *     unless its quality is the fixed 0.  This holds whether or not span >= min_cov: a junction with an insertion majority that the
 *     call did not make for lack of span gives its base byte quality 0.
 *   No byte, no quality: a position called deleted without an insertion emits nothing and its evidence is not reported.
 * The same pass counts a histogram of 94 int64 bins over all quality bytes of the call.
 *
 * mhap_correct_quality needs a completed mhap_correct_finish with no record added since and uses that finish's min_cov, which the
 * session remembers; quals takes out_offsets[n_reads] bytes.  mhap_consensus_quality is the same against the last completed
 * mhap_consensus_run (n_out_bytes bytes); a run the guard refused, or a graph session that has moved on, leaves nothing to ask for.
 * MHAP_E_INVALID with a message otherwise, and for per_vote or cap out of range; params == NULL: the defaults; hist may be NULL.  They
 * may be repeated with other parameters.  The pass is a kernel of its own next to each call kernel (correct_kernels.hip,
 * consensus_kernels.hip) over one shared device function (vote_common.hpp); device memory: 1 byte per output byte from the first call.
 * The reads' own qualities weigh the votes on request ("quality-weighted votes" below).
 * Left out: qualities for called deletions; qualities in the GFA. */
typedef struct mhap_quality_params { int32_t per_vote, cap; } mhap_quality_params;
#define MHAP_QUALITY_BINS 94
void mhap_quality_default_params(mhap_quality_params* p);
int mhap_correct_quality(mhap_correct_session* s, const mhap_quality_params* params /* NULL: the defaults */,
                         uint8_t* quals /* out_offsets[n_reads] */, int64_t* hist /* MHAP_QUALITY_BINS, or NULL */);
int mhap_consensus_quality(mhap_consensus_session* s, const mhap_quality_params* params /* NULL: the defaults */,
                           uint8_t* quals /* n_out_bytes */, int64_t* hist /* MHAP_QUALITY_BINS, or NULL */);

/* ---- quality-weighted votes: the pile-up of "read correction" and "unitig consensus" with the reads' own base qualities -------------- */

/* Opt-in.  A session begun with qualities (one Phred byte per base, parallel to `bases`, as "FASTQ input" delivers them) follows the
 * contract of "read correction" with every "adds 1" replaced by a weight; tests/weighted_vote_ref.py restates it.
 *
 * The weight of a base of Phred q, with the parameters 0 <= q_lo <= q_hi <= 93:   q < q_lo: 1;   q_lo <= q < q_hi: 2;   q >= q_hi: 3.
 * The neutral weight is 2.
 *
 * Votes.  M(t, e) adds w(q_e) to base[t][e]; the k-th byte of an Ins group adds w(q_e) to ins[t][k][e]; q_e is the quality of the
 * evidence byte at its stored position, so a reverse-complemented byte has the quality of the byte it was complemented from.  A byte
 * that is not A, C, G or T votes nothing, as before.  Del(t) and span[t] add the neutral 2.  A vote stays one integer atomic add, of w
 * or w << 16; a view adds at most 3 to a counter, so a target accepts 21 845 views (65 535 / 3) before views are skipped and counted in
 * skipped_views, on the host in arrival order as before, and the unitig consensus refuses a tile that more than 21 845 reads meet.
 *
 * The call.  d is the same sum.  d < 2 min_cov: low.  Otherwise own adds w(q_own) in the correction and the neutral 2 in the unitig
 * consensus (a draft byte has no single quality), total = d + that weight, and 2 del > total calls a deletion; the maximum and its
 * tie rules are unchanged.  A junction is voted on when span >= 2 min_cov, and an inserted base is emitted when 2 m > span + 2.
 *
 * Base qualities, the margins of "base qualities" in weighted units: Q = min(cap, per_vote * max(m, 0) / 20), where the own term of
 * the base margin is the weight above, n = d + that weight, an inserted byte has m = 2 ins[k][e] - (span + 2), and the stop margin is
 * (span + 2) - 2 max over b of ins[n_ins][b].
 *
 * The oracle inside the rule: with every quality in [q_lo, q_hi) each counter is twice its unweighted value and each comparison the
 * unweighted one times 2, so the bytes, the six counts and the output qualities are those of the unweighted session.
 *
 * mhap_correct_begin_weighted / mhap_consensus_begin_weighted are their siblings with `qualities` (n_bases bytes; NULL: the call is its
 * sibling, the session unweighted) and the weight parameters (NULL: the defaults; MHAP_E_INVALID unless 0 <= q_lo <= q_hi <= 93).  The
 * qualities go up once, one byte per base.  Every other entry point keeps its signature and, on a weighted session, follows this rule
 * through the weighted instantiations of the same kernels (vote_common.hpp over weighted_vote.hpp's policies); mhap_correct_votes and
 * mhap_consensus_votes return the weighted counters.  The defaults are the pair that left the fewest wrong bytes on the restatement
 * (EXPERIMENTS.md, "Quality-weighted votes").
 * Left out: qualities in the search, trimming, repeat and graph stages; qualities for called deletions; quality-aware alignment;
 * writing the input's qualities back out. */
typedef struct mhap_weight_params { int32_t q_lo, q_hi; } mhap_weight_params;
#define MHAP_WEIGHTED_VIEW_CAP 21845
void mhap_weight_default_params(mhap_weight_params* p);
int mhap_correct_begin_weighted(mhap_handle* h, const uint8_t* bases, const uint8_t* qualities /* n_bases, or NULL */, int64_t n_bases,
                                const int64_t* read_ids, const int64_t* offsets, const int32_t* lengths, int64_t n_reads,
                                const mhap_weight_params* weights /* NULL: the defaults */, mhap_correct_session** session);
int mhap_consensus_begin_weighted(mhap_graph_session* g, const uint8_t* bases, const uint8_t* qualities /* n_bases, or NULL */,
                                  int64_t n_bases, const int64_t* offsets /* n_reads */, const mhap_consensus_params* params,
                                  const mhap_weight_params* weights /* NULL: the defaults */, mhap_consensus_session** session);

/* ---- read trimming: every read cut to the stretch that other reads support, chimeras split, records rewritten onto the cut reads ---- */

/* The step in front of the string graph (the coverage rule of miniasm's first pass): a chimeric read joins two loci and a read with
 * an unsupported end keeps hangs that cost it its dovetails; neither the class rule nor the cleaning removes what follows.  Here
 * every aligned interval is shrunk by end_clip at both ends and piled up per read, and a read keeps the longest stretch that
 * min_cov of them cover, widened again by end_clip.  At a chimeric junction the overlaps of both sides end, so after the shrink
 * nothing covers it and the read falls into two stretches, of which the longer survives.  One round; left out: a second round on
 * the trimmed records.  "Overlap selection" below picks each read's best views for the read correction only: nothing is selected in
 * front of this stage.  A repeat's false overlaps count as coverage here; "repeat marking" below sets
 * them aside in front of this stage when it is asked to, within its two-copy limit.
 * Everything is integer arithmetic in int64; the only floating comparison is score < min_identity on the record's double.  The
 * result is a function of the multiset of records: invariant under any permutation of the records and any split of them over
 * calls.  Nothing is de-duplicated: a record given twice counts twice, as in the correction stage.
 *
 * Input.  A table of reads (read_ids[r], lengths[r]; no bases), realigned records as for mhap_graph_add, and the parameters
 * min_cov (3), end_clip (500), min_span (2000), min_identity (0.0); the defaults are choices, not measurements.  min_cov >= 1,
 * end_clip >= 0 and min_span >= 0, else MHAP_E_INVALID.
 *
 * Eligible record.  from_id != to_id, score != 0 and not score < min_identity.
 *
 * Contributions.  An eligible record gives read A (`from`) the interval [a1 + end_clip, a2 + 1 - end_clip) when a2 + 1 - a1 >= min_span
 * and the interval is not empty, and read B (`to`) the interval [b1 + end_clip, b2 + 1 - end_clip) under the same two conditions on
 * b: b1, b2 are in B's own forward coordinates already (the class rule's ts / te show it), so to_rc plays no part.  The two sides
 * are judged independently.
 *
 * Coverage.  cov_r[p] = the number of contributed intervals of read r that contain p.   Runs.  A run is a maximal stretch of
 * positions with cov >= min_cov.
 *
 * Clear range.  Of the longest runs [s, e) the one that begins first; the clear range is [s - end_clip, e + end_clip), which lies in
 * [0, length] by construction.  A read without a run is deleted and has the clear range (0, 0).
 *
 * Per-read result.  Four int32 {begin, end, runs, covered} — covered: the positions with cov >= min_cov — and one flag byte: bit 0
 * MHAP_TRIM_DELETED, bit 1 MHAP_TRIM_CUT5 (begin > 0), bit 2 MHAP_TRIM_CUT3 (end < length), bit 3 MHAP_TRIM_GAPPED (runs > 1: a
 * chimera or a gap in coverage, which overlaps cannot tell apart; the read is unusable across either).  A deleted read has no
 * other bit.  MHAP_TRIM_COUNTS int64 counts: reads, deleted, cut5, cut3, gapped, bases in, bases kept, eligible records.
 *
 * A record rewritten onto the trimmed reads (trim_common.hpp: one function for host and device).  Frame as in the class rule: qs = a1,
 * qe = a2 + 1; (ts, te) = (b1, b2 + 1) when !to_rc, else (blen - b2 - 1, blen - b1).  A's clear range is (ca, ea); B's in the frame is
 * (cb, eb) = clear[B] when !to_rc, else (blen - end_B, blen - begin_B).  SQ = qe - qs, ST = te - ts; div is the floor:
 *   d5q = max(0, ca - qs)   d5t = max(0, cb - ts)   d3q = max(0, qe - ea)   d3t = max(0, te - eb)
 *   s5q = max(d5q, d5t * SQ div ST)    s5t = max(d5t, d5q * ST div SQ)
 *   s3q = max(d3q, d3t * SQ div ST)    s3t = max(d3t, d3q * ST div SQ)
 *   qs' = qs + s5q   qe' = qe - s3q   ts' = ts + s5t   te' = te - s3t
 * The record is kept iff it is eligible, neither read is deleted (an explicit clear range with end <= begin is a deleted read), SQ > 0,
 * ST > 0, qe' > qs' and te' > ts'; every other record is void.  A kept record comes out with a1 = qs' - ca, a2 = qe' - 1 - ca,
 * alen = ea - ca and, with u = ts' - cb, v = te' - cb, blen = eb - cb: (b1, b2) = (u, v - 1) when !to_rc, else (blen - v, blen - u - 1);
 * ids, score, raw and to_rc unchanged.  A record between two untouched reads therefore comes out byte for byte as it went in.
 *
 * The session.  mhap_trim_begin takes the table of reads (params NULL: the defaults); the handle must outlive the session, whose
 * errors are the handle's (mhap_last_error).  mhap_trim_add piles the records up on the device (trim_kernels.hip: one lane per
 * record, up to four atomic adds of +1 / -1 into a per-base difference array), any number of times, n = 0 included, and does not
 * wait for the device; ids and alen / blen are checked as mhap_graph_add checks them, and a record with score != 0 must have
 * 0 <= a1 <= a2 < alen and 0 <= b1 <= b2 < blen: MHAP_E_INVALID naming the record, and a refused call adds nothing.
 * mhap_trim_finish makes the rows and flags (one workgroup per read over tiles of MHAP_TRIM_TILE positions) and returns the counts;
 * it may be repeated, and more records may be added after it.  mhap_trim_copy writes the rows and flags of the last finish.
 * mhap_trim_coverage (tests): cov of every position of read read_index as the adds so far have left it.  mhap_trim_apply, after a
 * finish: out[q] = in[q] rewritten and keep[q] = 1 for a kept record, out[q] = in[q] and keep[q] = 0 for a void one; records are
 * checked as in the add; the caller compacts.  mhap_trim_clip_record uses no GPU and takes explicit clear ranges {begin, end} of the
 * two reads: 1 kept (out rewritten), 0 void (out = in), -1 for a null pointer or bad parameters.  Device memory from begin to free:
 * 4 bytes per base and 48 per read (each read's slots rounded up to four), 32 per record of the largest add, 64 of the largest apply.
 *
 * Refinement, in front of the add.  The realignment's local alignment (+2 / -2, gaps 2 + 1 per base) keeps gaining score between
 * unrelated sequences, so the overlap of a chimeric read comes back running through the junction and the coverage rule would see no
 * gap there.  Before a record is piled up, its path ("the realignment stage's paths") is therefore scored again, +1 per '=' column
 * and -penalty per X, I or D column, and the record is cut to the best stretch: the runs are walked in order with a running sum
 * that starts again from 0 at an '=' run when it is <= 0, and the best stretch is the one behind the first strictly greatest sum
 * seen at the end of an '=' run; it begins and ends with '=' columns.  penalty 2 (the tools' default) breaks even at an identity of
 * 2 / 3: two reads with up to 15 % error each agree in 0.85^2 = 0.72 of their columns or more and gain, an alignment through unrelated
 * sequence agrees in little over half and loses.  The refined record has the stretch's a1, a2, b1, b2 (b flipped back when to_rc) and
 * score = 1 - errors / columns of the stretch; everything else is unchanged, and a record whose path has no '=' column comes back as
 * it is.  mhap_trim_refine does it on the device, one lane per record (paths: those of the n records, as mhap_realign_records_paths
 * or mhap_align_paths_from_runs gives them; MHAP_E_INVALID for another number of records, for runs outside the object or penalty < 1);
 * mhap_trim_refine_record is the same rule on the host for one record and its runs: 1 refined, 0 unchanged, -1 for a bad argument. */
typedef struct mhap_trim_params {
  int32_t min_cov, end_clip, min_span;
  double min_identity;
} mhap_trim_params;
#define MHAP_TRIM_COUNTS 8
#define MHAP_TRIM_TILE 4096
#define MHAP_TRIM_DELETED 1
#define MHAP_TRIM_CUT5 2
#define MHAP_TRIM_CUT3 4
#define MHAP_TRIM_GAPPED 8
typedef struct mhap_trim_session mhap_trim_session;
void mhap_trim_default_params(mhap_trim_params* p);
int mhap_trim_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_trim_params* params,
                    mhap_trim_session** session);
int mhap_trim_add(mhap_trim_session* s, const mhap_record* realigned, int64_t n);
int mhap_trim_finish(mhap_trim_session* s, int64_t* counts /* MHAP_TRIM_COUNTS */);
int mhap_trim_copy(mhap_trim_session* s, int32_t* rows /* n_reads x 4 */, uint8_t* flags /* n_reads */);
int mhap_trim_coverage(mhap_trim_session* s, int64_t read_index, int32_t* cov /* length */);
int mhap_trim_apply(mhap_trim_session* s, const mhap_record* in, int64_t n, mhap_record* out, uint8_t* keep /* n */);
int mhap_trim_clip_record(const mhap_record* in, const int32_t* clearA /* 2 */, const int32_t* clearB /* 2 */, const mhap_trim_params* params,
                          mhap_record* out);
int mhap_trim_refine(mhap_handle* h, const mhap_record* realigned, int64_t n, const mhap_align_paths* paths, int32_t penalty, mhap_record* out);
int mhap_trim_refine_record(const mhap_record* in, const uint32_t* ops, int64_t n_ops, int32_t penalty, mhap_record* out);
void mhap_trim_free(mhap_trim_session* s);

/* ---- repeat marking: repeats found from the overlap pile-up, overlaps that lie in nothing but repeat set aside ---- */

/* An opt-in step in front of the trimming and the string graph (the overlap-based repeat rule of Canu and Falcon as integer
 * arithmetic).  Two reads from different copies of a repeat overlap inside the repeat; where the repeat sits at a read's end that
 * overlap looks like a dovetail, becomes an arc between two loci, counts as support in the trimming, is a fork and no tip to the
 * cleaning, and makes the consensus vote reads of one copy onto another.  Here the aligned intervals are piled up per read, the
 * stretches of a read that lie well above the typical depth are marked, and every overlap that has no anchor outside such stretches
 * on either of its reads is void.  The result is a function of the multiset of records: invariant under any permutation of the
 * records and any split of them over calls, and the same bytes from run to run.  Nothing is de-duplicated.
 *
 * Input.  A table of reads (read_ids[r], lengths[r]; no bases), realigned records as for mhap_trim_add, and the parameters
 * factor_pct (200), max_cov (0: derive it), min_run (500), min_unique (500), min_identity (0.0); the defaults are choices, not
 * measurements.  factor_pct >= 100, max_cov >= 0, min_run >= 1 and min_unique >= 0, else MHAP_E_INVALID.
 *
 * Eligible record.  The trimming's rule: from_id != to_id, score != 0 and not score < min_identity.
 *
 * Coverage.  An eligible record gives read A the interval [a1, a2 + 1) and read B the interval [b1, b2 + 1) (b is in B's forward
 * coordinates already, so to_rc plays no part): the trimming's contribution with end_clip = 0 and min_span = 0, no shrink and no
 * minimum span.  cov_r[p] = the number of contributed intervals of read r that contain p.
 *
 * Typical depth D.  hist[c] = the positions p in [0, length_r) over all reads with min(cov_r[p], MHAP_REPEAT_BINS - 1) == c; N1 = the
 * sum of hist[c] over c >= 1; D = the smallest c >= 1 with 2 * (hist[1] + ... + hist[c]) >= N1 (the lower median of the covered
 * positions), 0 when N1 == 0.  When max_cov == 0 and D == MHAP_REPEAT_BINS - 1 the last bin has swallowed the median: the finish fails
 * with MHAP_E_INVALID and a message that says to give max_cov.
 *
 * Threshold T.  max_cov when max_cov > 0, else D * factor_pct div 100.  Position p of read r is a repeat position iff cov_r[p] > T.
 *
 * Repeat intervals.  The maximal runs [s, e) of repeat positions of read r with e - s >= min_run, ascending.  CSR: int64
 * offsets[n_reads + 1] and int32 pairs {begin, end}.  Per read four int32 {intervals, repeat_bases (the sum of e - s), max_cov (the
 * greatest cov_r[p], 0 for an empty read), first_begin or -1} and one flag byte: bit 0 MHAP_REPEAT_SOME (an interval), bit 1
 * MHAP_REPEAT_WHOLE (one interval, and it is [0, length)).  MHAP_REPEAT_COUNTS int64 counts: reads, reads with an interval,
 * whole-repeat reads, intervals, repeat bases, bases, eligible records, D, T.
 *
 * Judging a record.  For an eligible record uA = (a2 + 1 - a1) - (the positions of [a1, a2 + 1) inside A's intervals) and uB likewise
 * on B; keep = 1 iff uA >= min_unique and uB >= min_unique, else 0.  An ineligible record has keep = 1 and uA = uB = -1: later stages
 * have their own rule for it.  Records are never rewritten.
 *
 * What it does not do.  A two-copy repeat at ordinary depth piles up to about twice D only where the reads of both copies happen to
 * lie, which is not reliably above any usable threshold: on exact records the default keeps all or nearly all of its false overlaps
 * at three of four seeds, factor_pct 150 still keeps 212 of 467 at one, and 140 and 125 void up to 36 and 419 of about 8 600 true
 * overlaps with a good anchor (EXPERIMENTS.md, "Repeat marking").  Intervals are neither padded nor merged, so a dip in the
 * pile-up inside a repeat splits its interval and a run shorter than min_run is no interval at all.  One round: the depth is not
 * measured again without the void records.
 *
 * The session mirrors mhap_trim_*.  mhap_repeat_begin takes the table of reads (params NULL: the defaults); the handle must outlive
 * the session, whose errors are the handle's.  mhap_repeat_add piles records up (the trimming's add kernel, shared, with the
 * parameters above), any number of times, n = 0 included, without waiting; the same checks and refusals as mhap_trim_add, and a
 * refused call adds nothing.  mhap_repeat_finish makes the bins, D and T, the rows, flags, offsets and intervals, waits once and
 * returns the counts; it may be repeated, and more records may be added after it.  mhap_repeat_copy writes the rows, flags, offsets
 * and intervals (counts[3] pairs) of the last finish; mhap_repeat_histogram its MHAP_REPEAT_BINS bins.  mhap_repeat_apply, after a
 * finish: keep[q] and unique[2 q], unique[2 q + 1] = uA, uB; records are checked as in the add; the caller compacts.
 * mhap_repeat_judge_record uses no GPU and takes explicit interval lists {begin, end} of the two reads (ascending, disjoint, inside
 * the read): 1 keep, 0 void, -1 for a null pointer, bad parameters, a bad list or an eligible record outside its reads; unique
 * (may be NULL) takes uA, uB.  Device memory from begin to free: 4 bytes per base (the difference array, each read's slots rounded
 * up to four), 45 per read, 12 per interval the reads could have (the sum of (length + 1) div (min_run + 1)), 32 per record of the
 * largest add and 48 of the largest apply, 32 KiB of bins. */
typedef struct mhap_repeat_params {
  int32_t factor_pct, max_cov, min_run, min_unique;
  double min_identity;
} mhap_repeat_params;
#define MHAP_REPEAT_COUNTS 9
#define MHAP_REPEAT_BINS 4096
#define MHAP_REPEAT_SOME 1
#define MHAP_REPEAT_WHOLE 2
typedef struct mhap_repeat_session mhap_repeat_session;
void mhap_repeat_default_params(mhap_repeat_params* p);
int mhap_repeat_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_repeat_params* params,
                      mhap_repeat_session** session);
int mhap_repeat_add(mhap_repeat_session* s, const mhap_record* realigned, int64_t n);
int mhap_repeat_finish(mhap_repeat_session* s, int64_t* counts /* MHAP_REPEAT_COUNTS */);
int mhap_repeat_copy(mhap_repeat_session* s, int32_t* rows /* n_reads x 4 */, uint8_t* flags /* n_reads */, int64_t* offsets /* n_reads + 1 */,
                     int32_t* intervals /* counts[3] x 2 */);
int mhap_repeat_histogram(mhap_repeat_session* s, int64_t* bins /* MHAP_REPEAT_BINS */);
int mhap_repeat_apply(mhap_repeat_session* s, const mhap_record* in, int64_t n, uint8_t* keep /* n */, int32_t* unique /* n x 2 */);
int mhap_repeat_judge_record(const mhap_record* in, const int32_t* intervalsA, int64_t nA, const int32_t* intervalsB, int64_t nB,
                             const mhap_repeat_params* params, int32_t* unique /* 2, or NULL */);
void mhap_repeat_free(mhap_repeat_session* s);

/* ---- variant sites: positions where the pile-up shows two well-supported alleles, overlaps that disagree across them set aside ---- */

/* An opt-in step in front of the repeat marking, the trimming and the string graph (what HiCanu and hifiasm do in front of their
 * graphs, as integer arithmetic).  Every other stage takes two reads that align well for two views of one sequence; this one asks
 * whether they agree where the pile-up says there are two alleles, which is what tells the two haplotypes of a diploid sample, or the
 * two copies of a diverged repeat, apart.  The result is a function of the multiset of accepted views: the same bytes from run to
 * run and however the records are split over calls or ordered, except for which views the cap below skips.  Nothing is
 * de-duplicated.  A, C, G, T are the upper-case bytes, with the codes 0, 1, 2, 3; the complement of code b is 3 - b.
 *
 * Input.  The reads (bases, read_ids[r], offsets[r], lengths[r], as for mhap_correct_begin), realigned records with their paths as for
 * mhap_correct_add, and the parameters min_depth (8), min_minor (3), min_pct (25), max_del_pct (25), min_diff (2), diff_pct (50).  The
 * defaults are provisional (EXPERIMENTS.md, "Variant filter").  min_depth, min_minor and min_diff >= 1 and the three percentages in
 * 0 .. 100, else MHAP_E_INVALID with a message that gives the six values.
 *
 * 1. Votes.  Which records vote, their two views and the columns of a view are those of "read correction" above, word for word.  Six
 * counters per target position t: base[4] (A, C, G, T), del and span, with the correction's meaning: M(t, e) adds 1 to base[t][e]
 * when e is A, C, G or T; Del(t) adds 1 to del[t]; two consecutive target-consuming columns t, t' of a view add 1 to span[t].  Ins
 * columns vote nothing: there are no insertion slots.  Every vote is 1; base qualities play no part.  The counters are 16 bits wide,
 * two to a word, 12 bytes per base; the cap is the correction's: views are accepted per target in arrival order (record by record,
 * view A before view B), and a view whose target already has 65 535 accepted views is skipped whole and counted in skipped_views.
 * The six counters equal the first six of mhap_correct_votes for the same records and paths.
 *
 * 2. Sites.  For position t of a read with own byte o: c[b] = base[t][b], plus 1 when o is b; depth = c[A] + c[C] + c[G] + c[T] +
 * del[t] (so a position nobody voted on has depth 1 when o is A, C, G or T, else 0).  major = the b with the greatest c[b], the
 * lowest code among those tied; minor = the same over the other three codes.  The position is deep iff depth >= min_depth, and a site
 * iff all of these hold, in integers:
 *   o is A, C, G or T;   depth >= min_depth;   c[minor] >= min_minor;   100 c[minor] >= min_pct depth;   100 del[t] <= max_del_pct depth.
 * Per base one site byte stays on the device: bit 0 site, and for a site bits 1 - 2 major and bits 3 - 4 minor (0 for no site).  Per
 * read two int32 {n_sites, n_deep}.  The site list has one row of six int32 {pos, major, minor, c[major], c[minor], depth} per site,
 * in the order of the reads and then of the positions; int64 offsets[n_reads + 1] are the prefix sums of n_sites, so read r's rows
 * are [offsets[r], offsets[r + 1]).  MHAP_VARIANT_COUNTS int64 counts: reads, reads with a site, sites, deep positions, bases,
 * accepted views, skipped views.
 *
 * 3. Judging a record.  A record that would not vote (no runs, or equal ids) has four zero tallies and keep = 1.  Of any other, every
 * '=' / 'X' column (i, j) of the path is classed from a = s1[i], b = s2[j] (read B's byte in the aligner's orientation, complemented
 * through the aligner's table when to_rc), the site byte of A at i, and the site byte of B at its own position (blen - 1 - j when
 * to_rc, else j) with major and minor replaced by their complements when to_rc.  The column is informative iff either byte is a
 * site.  Its allele pair is {major, minor} of the one that is; when both are, the two pairs must be equal as sets, else the column
 * counts as other.  With a and b both in the pair the column counts as agree when a == b and as disagree when not; with either
 * outside it (any byte that is not A, C, G or T is) as other.  tallies[q] = {informative, agree, disagree, other} as int32, and
 *   keep[q] = !(disagree >= min_diff && 100 disagree >= diff_pct (agree + disagree)).
 * The rule is symmetric in the two reads by construction: a column's class reads a and b, and the two site bytes, as unordered
 * pairs, so a record and the same alignment written from read B's side (rows and columns exchanged, and for to_rc everything
 * complemented and reversed) get the same four tallies and the same keep.  Records are never rewritten.
 *
 * What it does not do.  Votes are not weighed by quality; indels are no variants (a position the pile-up mostly deletes is no site,
 * that is all); sites are not phased into blocks; the read correction and the consensus stay haplotype-blind; one GPU.
 *
 * The session.  mhap_variant_begin uploads the bases once and allocates and zeroes the vote table (params NULL: the defaults); the
 * handle must outlive the session, whose errors are the handle's.  mhap_variant_add accepts, validates, caps and refuses exactly as
 * mhap_correct_add does — MHAP_E_INVALID, naming the record, for an id not among read_ids, an alen or blen that disagrees with the
 * read's length, a paths object of another n, or runs that do not spell the record's intervals (the same two rules) — and a refused
 * call has cast no vote; one wave per accepted view adds its votes (variant_kernels.hip).  After a completed mhap_variant_finish the
 * add is refused: the site bytes are those of the votes before it.  mhap_variant_votes: the six counters of every position of read
 * read_index, position-major, in the order A C G T del span; for tests.  mhap_variant_finish makes the site bytes, the rows, the
 * offsets and the list on the device (one workgroup per read over tiles of MHAP_VARIANT_TILE positions, longest reads first; a site's
 * row comes from a prefix sum, never from an atomic) and returns the counts; it may be repeated.  mhap_variant_copy writes the rows,
 * offsets and the counts[2] rows of the list.  mhap_variant_apply, after a finish (else MHAP_E_INVALID): one wave per record walks the
 * path again; the records and paths are checked as in the add and a refused call writes nothing; the caller compacts.  Device memory
 * from begin to free: 14 bytes per base (votes, site byte, the base), 44 per read, 24 per site, 4 per run and 64 per view of the
 * largest add, 97 per record of the largest apply. */
typedef struct mhap_variant_params {
  int32_t min_depth, min_minor, min_pct, max_del_pct, min_diff, diff_pct;
} mhap_variant_params;
#define MHAP_VARIANT_COUNTS 7
#define MHAP_VARIANT_TILE 1024
typedef struct mhap_variant_session mhap_variant_session;
void mhap_variant_default_params(mhap_variant_params* p);
int mhap_variant_begin(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                       const int32_t* lengths, int64_t n_reads, const mhap_variant_params* params, mhap_variant_session** session);
int mhap_variant_add(mhap_variant_session* s, const mhap_record* realigned, int64_t n, const mhap_align_paths* paths);
int mhap_variant_votes(mhap_variant_session* s, int64_t read_index, uint16_t* counters /* length x 6 */);
int mhap_variant_finish(mhap_variant_session* s, int64_t* counts /* MHAP_VARIANT_COUNTS */);
int mhap_variant_copy(mhap_variant_session* s, int32_t* rows /* n_reads x 2 */, int64_t* offsets /* n_reads + 1 */, int32_t* sites /* counts[2] x 6 */);
int mhap_variant_apply(mhap_variant_session* s, const mhap_record* realigned, int64_t n, const mhap_align_paths* paths, uint8_t* keep /* n */,
                       int32_t* tallies /* n x 4 */);
void mhap_variant_free(mhap_variant_session* s);

/* ---- overlap selection: every read keeps its best_n best views as evidence, the others are set aside view by view ---- */

/* An opt-in step in front of the read correction (the overlap selection of Canu's evidence-coverage cap and minimum evidence length
 * and of Falcon's max_n_read, as integer arithmetic).  A read inside a repeat family is seen by hundreds of overlaps, most of them
 * from other copies, and a read at a coverage of 300 pays for 300 views where 40 would do.  Here every view of a record gets a key,
 * the counted matches on the read it sits on, and a read keeps the best_n views with the greatest keys.  The choice is made per read
 * and per view: a record may be among the best of its `from` read and not of its `to` read, so the result is two bits per record,
 * not a shorter list of records.  Every output byte is a function of the multiset of records: invariant under any permutation of the
 * records and any split of them over calls, and the same from run to run.  Nothing is de-duplicated.
 *
 * Input.  A table of reads (read_ids[r], lengths[r]; no bases), realigned records as for mhap_repeat_add, and the parameters best_n
 * (40), min_span (500) and min_identity (0.0); the defaults are choices, not measurements.  best_n >= 1 and min_span >= 0, else
 * MHAP_E_INVALID.
 *
 * Eligible record.  The trimming's rule and one clause more: from_id != to_id, score != 0, not score < min_identity, and
 * score == score (a NaN is not eligible).
 *
 * Entries.  An eligible record gives up to two entries: view A on read `from` with the span sA = a2 + 1 - a1, view B on read `to`
 * with the span sB = b2 + 1 - b1 (b is in B's forward coordinates, so to_rc plays no part).  A view exists only when its span is
 * >= min_span.  Its key is 1 + (uint32) floor((double) span * min(score, 1.0)), a product below 0 (a negative score that a negative
 * min_identity let through) counting as 0: between 1 and 2^31 - 8, and 0 stands for "no such view".  select_common.hpp holds the
 * one function, compiled for host and device: one compare, one min, one multiply and one floor, nothing that can be contracted.
 *
 * Threshold.  E_r = the entries of read r.  thr_r = 1 when E_r <= best_n, else the best_n-th greatest key of r counted with
 * multiplicity.  An entry is kept iff key >= thr_r, that is, iff fewer than best_n entries of its read have a strictly greater key.
 * Ties at the last place are all kept, so a read may keep more than best_n; no tie-break field is needed, and none exists.
 *
 * Outputs.  Per read four int32 {entries, kept, thr, greatest key (0 when it has no entry)}.  MHAP_SELECT_COUNTS int64 counts: reads,
 * reads with an entry, reads with more than best_n entries, entries, kept entries, eligible records.  Per judged record one byte:
 * bit 0 MHAP_SELECT_A (view A kept), bit 1 MHAP_SELECT_B; an ineligible record, or a view below min_span, has the bit clear.
 *
 * What it does not do.  No best-n per read end for the string graph, no selection in front of the trimming or the unitig consensus,
 * and one round: the keys are not made again from the corrected reads.  The key does not know a repeat from a unique stretch: where
 * more than best_n copies of a repeat align better than the true neighbours, the copies win.
 *
 * The session mirrors mhap_repeat_*.  mhap_select_begin takes the table of reads (params NULL: the defaults); the handle must
 * outlive the session, whose errors are the handle's.  mhap_select_add (select_kernels.hip) uploads the records once and one lane per
 * record writes its two entries and counts them per read, any number of times, n = 0 included, without waiting (when the entries'
 * buffer is full it doubles, and that copy is waited for); the same checks and refusals as mhap_trim_add, a refused call adds
 * nothing, and a session takes 2^31 - 1 records and 2^30 - 1 reads.  mhap_select_finish makes the segments, thresholds, rows and
 * counts (a radix select over the key's four bytes, one workgroup per read with more than best_n entries at a time; a segment of
 * at most MHAP_SELECT_LDS_KEYS keys stays in LDS), waits once and returns the counts; it may be repeated, and more records may be
 * added after it.  mhap_select_copy writes the rows of the last finish (MHAP_E_STATE before one).  mhap_select_apply, after a finish
 * (MHAP_E_STATE before one), judges any records, added or not, against the thresholds of the last finish: views[q]; records are
 * checked as in the add.  mhap_select_judge_record uses no GPU: keys[0], keys[1] = the keys of view A and B, 0 for no such view;
 * 1 for an eligible record, 0 for an ineligible one, -1 for a null pointer, bad parameters or an eligible record outside its reads.
 * Device memory from begin to free: 16 bytes per record (the entries; up to twice that after a doubling), 8 per record for the keys
 * in their segments, 32 per record of the largest add or apply and 1 of the largest apply, and 40 per read. */
typedef struct mhap_select_params {
  int32_t best_n, min_span;
  double min_identity;
} mhap_select_params;
#define MHAP_SELECT_COUNTS 6
#define MHAP_SELECT_LDS_KEYS 8192
#define MHAP_SELECT_A 1
#define MHAP_SELECT_B 2
typedef struct mhap_select_session mhap_select_session;
void mhap_select_default_params(mhap_select_params* p);
int mhap_select_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_select_params* params,
                      mhap_select_session** session);
int mhap_select_add(mhap_select_session* s, const mhap_record* realigned, int64_t n);
int mhap_select_finish(mhap_select_session* s, int64_t* counts /* MHAP_SELECT_COUNTS */);
int mhap_select_copy(mhap_select_session* s, int32_t* rows /* n_reads x 4 */);
int mhap_select_apply(mhap_select_session* s, const mhap_record* in, int64_t n, uint8_t* views /* n */);
int mhap_select_judge_record(const mhap_record* in, const mhap_select_params* params, uint32_t* keys /* 2 */);
void mhap_select_free(mhap_select_session* s);

/* ---- homopolymer compression: every run of equal bytes collapsed to one, the map back kept, records carried to raw coordinates ---- */

/* The step in front of the search for reads whose commonest error is the wrong length of a homopolymer run (what minimap2 -H, Canu's
 * HiFi mode, Flye and hifiasm do): the reads are sketched and searched with every run collapsed to one base, and what is found is
 * carried back through the map, so that the realignment and every stage behind it see raw reads and raw coordinates.
 *
 * The reads.  Read r is its lengths[r] bytes at bases + offsets[r], taken as they are: offsets in any order, overlapping, unaligned
 * (the table of trimmed reads is such a table).  MHAP_E_INVALID, the read named in the message, for a negative length or a read that
 * does not lie in [0, n_bases); lengths above 2^31 - 9 and 2^30 reads or more are refused as every table of reads refuses them.
 *
 * Heads.  Position p of a read is a head iff p = 0 or byte[p] != byte[p - 1].  Equality is equality of bytes: runs of N collapse, a and
 * A differ.  The byte in front of a read's first base never matters (it belongs to another read, or to nobody).
 *
 * Result.  The compressed read is its head bytes in order; clen is their number.  The map start[0 .. clen] holds the raw position of
 * every head, and start[clen] = L, the raw length: compressed position p stands for the raw run [start[p], start[p + 1]).  An empty
 * read compresses to an empty read with start = {0}.  The compressed reads lie back to back in read order, coff[r + 1] = coff[r] +
 * clen[r] with coff[0] = 0, and the map of read r is the clen[r] + 1 int32 at starts + coff[r] + r.  MHAP_HPC_COUNTS int64 counts:
 * reads, raw bases, compressed bases, runs longer than 1, the longest run, empty reads.
 *
 * Records.  Two functions of a read's map, for any int32 p:
 *     p < 0: lo(p) = hi(p) = -1        0 <= p < clen: lo(p) = start[p], hi(p) = start[p + 1] - 1        p >= clen: lo(p) = hi(p) = L
 * A record in compressed coordinates expands to a1' = lo_from(a1), a2' = hi_from(a2), b1' = lo_to(b1), b2' = hi_to(b2), alen' and blen'
 * the raw lengths; ids, score, raw and to_rc are copied.  b1 and b2 are taken as the record holds them, that is after MatchResult's
 * flip (J/impl/MatchResult.java:54-57: b1 = blen - b2 - 1, b2 = blen - b1 - 1 when to_rc), and no case is made of to_rc, because the
 * rule is symmetric under the flip: compression commutes with the reverse complement (a run stays a run), so position p of the
 * reversed compressed read is position clen - p - 1 of the forward one and stands for the raw run [L - hi(p) - 1, L - lo(p) - 1] of the
 * forward read, which reads  L - hi_rc(p) - 1 = lo(clen - p - 1)  and  L - lo_rc(p) - 1 = hi(clen - p - 1).  Expanding the flipped ends
 * on the forward map therefore gives the flip of the ends expanded on the reversed map.  The edge values obey the same equations: the
 * second stage may give a2 or b2 = clen (J/sketch/BottomOverlapSketch.java:131-134), which the flip turns into -1, and lo(-1) = -1 =
 * L - hi(clen) - 1, hi(clen) = L = L - lo(-1) - 1.  tests/hpc_ref.py restates all of it.
 *
 * The calls.  mhap_hpc_compress does it on the GPU (hpc_kernels.hip: two passes over tiles of MHAP_HPC_TILE positions and a scan of the
 * tiles' head counts in blocks of MHAP_HPC_SCAN_BLOCK, for groups of whole reads of at most group_bases raw bases each; 0: 2^28, at
 * most 2^30; a longer read is a group of its own; the result does not depend on it) and leaves the compressed reads and the maps on
 * the device with the object; the handle must outlive the object, whose errors are the handle's (mhap_last_error).  mhap_hpc_info
 * gives the counts, mhap_hpc_copy the arrays (any pointer may be NULL).  mhap_hpc_expand_records expands n records on the device, one
 * lane per record: the `from` reads are looked up by id in from_side, the `to` reads in to_side (NULL: from_side; another object must be
 * of the same device); MHAP_E_INVALID, the record named in the message, for an id that its side does not have or an alen / blen that
 * is not that read's clen; a refused call writes nothing.  mhap_hpc_expand_record is the rule on the host for one record and explicit
 * maps: 0, or -1 for a null pointer or a negative clen.  Device memory of an object: 5 bytes per compressed base and 24 per read;
 * during the compression also the raw bytes, 8 bytes per read and 40 per tile. */
#define MHAP_HPC_TILE 4096         /* positions per workgroup of the two passes: 256 lanes x 16 bytes */
#define MHAP_HPC_SCAN_BLOCK 4096   /* tile counts the scan takes at once: 1024 lanes x 4, a carry from block to block */
#define MHAP_HPC_COUNTS 6
typedef struct mhap_hpc mhap_hpc;
int mhap_hpc_compress(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                      const int32_t* lengths, int64_t n_reads, int64_t group_bases /* 0: default */, mhap_hpc** out);
int mhap_hpc_info(const mhap_hpc* c, int64_t* counts /* MHAP_HPC_COUNTS */);
int mhap_hpc_copy(const mhap_hpc* c, uint8_t* cbases, int64_t* coff /* n + 1 */, int32_t* clen /* n */, int32_t* starts /* compressed + n */);
int mhap_hpc_expand_records(const mhap_hpc* from_side, const mhap_hpc* to_side /* NULL: the same */, const mhap_record* in, int64_t n,
                            mhap_record* out);
int mhap_hpc_expand_record(const mhap_record* in, const int32_t* start_from, int32_t clen_from, const int32_t* start_to, int32_t clen_to,
                           mhap_record* out);   /* host, no GPU */
/* milliseconds of the compression that made the object: the upload of the reads, the two passes with the scan, the kernel that sums the run counts up (all
 * three between HIP events on the handle's stream), and the whole call on the host's clock (tools/hpc_bench.py) */
int mhap_hpc_times(const mhap_hpc* c, double* ms /* 4 */);
void mhap_hpc_free(mhap_hpc* c);

/* KmerStatSimulator's pair statistics on the GPU (J/main/KmerStatSimulator.java:163-196).  pairs: n rows of 4 int64 {a_off, a_len,
 * b_off, b_len}; a = bases[a_off, a_off + a_len) is the first read, b the second.  skip: n_skip k-mers of k bytes each, back to back, in
 * any order (the skip set of loadSkipMers; entries of another length never match and are left out by the caller).  For each pair,
 * out[3 q ..] = {shared, total, intersect}:
 *   shared    = the distinct k-mers of b that are among the distinct k-mers of a not in the skip set (compareKmers' `shared`);
 *   total     = the distinct k-mers of a and b together (compareKmers' `totalSeqs`);
 *   intersect = BottomSketch.jaccard's intersectCount: the bottom sketch of a read is the min(bottom_k, windows) smallest signed
 *               murmur3_x86_32(seed 0) values of its canonical k-mers (String.compareTo of the k-mer against Utils.rc of it), duplicates
 *               kept, and the count comes from Java's merge loop run for min(sketch sizes) steps.
 * Exact for any bytes and any k >= 1 (k-mers are compared byte for byte); a read shorter than k has no windows.  MHAP_E_INVALID for a
 * segment outside the n_bases bases.  The environment variable MHAP_KSIM_HASH_BITS=b (1..64, tests only) narrows the kernel's internal
 * 64-bit window key to b bits, so that different k-mers share keys and the byte comparison decides. */
int mhap_pair_kmer_stats(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t k,
                         int32_t bottom_k, const uint8_t* skip, int64_t n_skip, int32_t* out, int32_t* paths);
/* paths (may be NULL): n int32, the scratch each pair took: 1 = LDS (the pair's keys fit min(device LDS per workgroup, 160 KiB)), 2 = a
 * per-workgroup slice of HBM.  The kernel is chosen by segment length and key kind, never by an option.  The smallest bottom_k hashes of
 * each read come from a full sort of its hashes in that scratch (a radix select of them would do less work; not built).
 * mhap_ksim_dev_create / _destroy: the same statistics with device buffers kept (grow-only) across calls, for a simulation's chunks;
 * mhap_ksim_dev_pair_stats takes mhap_pair_kmer_stats's arguments after the session. */
void* mhap_ksim_dev_create(mhap_handle* h);
void mhap_ksim_dev_destroy(void* dev);
int mhap_ksim_dev_pair_stats(void* dev, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t k, int32_t bottom_k,
                             const uint8_t* skip, int64_t n_skip, int32_t* out, int32_t* paths);
/* KmerStatSimulator's trials generated on the device (--rng device): trials trial0 .. trial0 + n - 1 of the stream `seed`, with
 * mhap_ksim_create's meaning of length, offset, the rates, flags and the reference records.  Java's rules, not its stream:
 *   - every draw is splitmix64 of a counter keyed by (seed, trial, role, index, slot) — seed -> splitmix64; ^ trial -> splitmix64;
 *     ^ (role << 32 | slot) -> splitmix64; ^ index -> splitmix64 — so a trial's reads do not depend on the launch shape or the chunk;
 *   - roles 0 / 1 / 2: the walks of the first read / shared partner / random partner over their 2L source bases (index = source base;
 *     slot 3v, 3v + 1, 3v + 2 = the error test, the error type and the new base of visit v); role 3: base i of a trial's random 4L sequence
 *     (no reference; "ACGT"[r >> 62]); role 4: base i of the random partner without a reference; role 5: the picks (index = draw count);
 *   - per visit: the error test (u < errorRate, u = top 53 bits * 2^-53), then the type in Java's order: substitution (one of the other
 *     three of ACGT; a non-ACGT base: one of all four), insertion (a uniform base, the same source base visited again), deletion;
 *   - per-base emission counts are prefix-summed into positions; the first read keeps the last L bases, the partners the first L;
 *   - picks: a record is redrawn until it has 4L (first read) or 2L (random partner) bases, the random partner's position while it
 *     overlaps the first read on the same record (Utils.getRangeOverlap > 0); without a reference firstPos = 0 and the random partner
 *     is L uniform bases without errors.
 * stats: n x 2 x 3 int32, mhap_pair_kmer_stats of (first, shared partner) and (first, random partner) on the reads where the generator
 * wrote them (not with MHAP_KSIM_SIM_ONLY).  Test hooks (each may be NULL): reads n x roles x L bytes, meta n x 5 as mhap_ksim_next's,
 * events n x roles x 4 int32 = {insertions, deletions, substitutions, visits} of each walk.  A read shorter than L after its errors
 * (Java's StringIndexOutOfBoundsException) gives MHAP_E_INVALID and *failed_trial = the first such trial. */
int mhap_ksim_dev_trials(void* dev, uint64_t seed, int64_t trial0, int64_t n, int32_t length, int32_t offset, double error_rate,
                         double ins_pct, double del_pct, double sub_pct, int32_t flags, const uint8_t* ref_bases,
                         const int64_t* ref_offsets, const int32_t* ref_lengths, int64_t n_ref, int32_t k, int32_t bottom_k,
                         const uint8_t* skip, int64_t n_skip, int32_t* stats, uint8_t* reads, int32_t* meta, int32_t* events,
                         int64_t* failed_trial);
/* Which scratch each pair of mhap_pair_kmer_stats would take with lds_bytes of LDS per workgroup: path[q] = 1 (LDS) or 2 (HBM).
 * hashed != 0: the pair has a non-ACGT byte or k > 31 (its keys carry a position word).  Tests only. */
int mhap_pair_kmer_stats_paths(const int64_t* pairs, int64_t n, int32_t k, int64_t lds_bytes, int32_t hashed, int32_t* path);

/* KmerStatSimulator's trials with its own java.util.Random stream (host only; the stream is sequential).  mhap_ksim_create(seed, L,
 * offset = (int) (2 * requestedLength - overlap), errorRate and the three error percentages, flags, reference records): the records are
 * upper-cased with N removed by the caller; n_ref = 0 simulates without a reference (buildRandomSequence(4L), firstPos = 0).
 * mhap_ksim_next writes the next n_trials trials: reads[t][role][L] with role 0 = first read, 1 = shared partner, 2 = random partner
 * (role 0 only with MHAP_KSIM_SIM_ONLY), and meta[t][5] = {seqID, firstPos, secondPos, random seqID, random pos}.  It returns the
 * number of trials completed; fewer than n_trials means Java threw in the next one: mhap_ksim_error gives the exception text and the
 * role whose getSequence threw ("" when none).  The caller checks that a reference has a record of at least 4L bases first (Java
 * would loop forever) and that the error mix terminates. */
#define MHAP_KSIM_ONE_SIDED 1     /* the second reads are walked at error rate 0 */
#define MHAP_KSIM_SIM_ONLY 2      /* only the first read of each trial (Usage 2, or k < 0) */
void* mhap_ksim_create(int64_t seed, int32_t length, int32_t offset, double error_rate, double ins_pct, double del_pct, double sub_pct,
                       int32_t flags, const uint8_t* ref_bases, const int64_t* ref_offsets, const int32_t* ref_lengths, int64_t n_ref);
int64_t mhap_ksim_next(void* state, int64_t n_trials, uint8_t* reads, int32_t* meta);
const char* mhap_ksim_error(void* state, int32_t* role);
void mhap_ksim_destroy(void* state);

/* Deterministic synthetic PacBio-style reads: xoshiro256** seeded by
 * splitmix64(seed), random genome of n*len/coverage bp, reads at uniform positions/strands with
 * i.i.d. errors (ins:del:sub = 0.1188:0.0183:0.0129 scaled to error_rate), exactly `len` bases each.
 * bases must hold n*len bytes. */
int mhap_synth_reads(uint64_t seed, int64_t n, int32_t len, double coverage, double error_rate, char* bases);
/* Only reads shard, shard+nshards, ... of that same n-read data set (bases holds ceil((n-shard)/nshards)*len bytes). */
int mhap_synth_reads_shard(uint64_t seed, int64_t n, int32_t len, double coverage, double error_rate, int64_t shard,
                           int64_t nshards, char* bases);
/* The same generator with a planted repeat family in the genome (BASELINE configs[4], the workload of the -f k-mer filter,
 * J/sketch/FrequencyCounts.java): one random element of rep_len bases, one copy with per-base substitution rate rep_div in
 * every rep_spacing-base stretch.  rep_len = 0 gives exactly mhap_synth_reads_shard's reads. */
int mhap_synth_reads_repeats(uint64_t seed, int64_t n, int32_t len, double coverage, double error_rate, int64_t shard,
                             int64_t nshards, int32_t rep_len, int32_t rep_spacing, double rep_div, char* bases);
/* Reads of given lengths from a SUPPLIED circular genome (one code 0..3 per byte), same error model; read r is written to
 * bases[offsets[r] .. offsets[r] + lengths[r]).  Test / bench tooling (the E. coli-shaped stand-in of BASELINE configs[2]). */
int mhap_synth_reads_genome(uint64_t seed, const uint8_t* genome, int64_t G, int64_t n, const int32_t* lengths, const int64_t* offsets,
                            double error_rate, char* bases);

/* Where the synthetic reads came from (the truth EstimateROC measures overlaps against), replayed from the same per-read generators
 * without generating a base.  lengths == NULL: the reads of mhap_synth_reads_repeats / _shard / mhap_synth_reads (n reads of `len`
 * bases, genome of n*len/coverage bases; G is ignored; entry q is read shard + q*nshards).  lengths != NULL: the reads of
 * mhap_synth_reads_genome from a genome of G bases (len, coverage, shard and nshards ignored; entry r is read r).  Per read: the genome
 * position of its first consumed base, the genome bases consumed (span; the read may wrap past G on the circular genome), the strand
 * (1 = the read is the reverse complement of genome[start, start + span)), and its inserted, deleted and substituted bases
 * (length = span + ins - del).  A read of length <= 0 gets start -1 and zeros. */
int mhap_synth_truth(uint64_t seed, int64_t n, int32_t len, double coverage, int64_t G, const int32_t* lengths, double error_rate,
                     int64_t shard, int64_t nshards, int64_t* start, int64_t* span, int8_t* strand, int32_t* n_ins, int32_t* n_del,
                     int32_t* n_sub);

/* GetHistogramStats.process() (J/main/GetHistogramStats.java:63-90) on a histogram already read: n rows (count vals[r], number
 * numbers[r]) in the TreeMap's order (ascending, distinct vals).  One Welford step per k-mer, numbers[r] steps per row (a number <= 0
 * steps none), in double with Java's rounding (no contraction): mean, stdev = sqrt(variance / k-mers) (NaN when there are none), and
 * cut = the first count whose running share of all occurrences, sum of (double)val * number over sum of val per k-mer, is above
 * percent (:81-89; 0 when none is). */
int mhap_histogram_stats(const int32_t* vals, const int64_t* numbers, int64_t n, double percent, double* mean, double* stdev, int64_t* cut);

/* murmur3_x64_128(seed 0).h1 of one k-mer line of a `-f` filter file, canonicalised when do_rc != 0
 * (HashUtils.computeSequenceHashesLong(str, len, 0, doRC)[0], J/sketch/FrequencyCounts.java:169). */
int mhap_hash_kmer(const char* kmer, int32_t len, int32_t do_rc, int64_t* out);

/* ---- test hooks: the kernels' __host__ __device__ arithmetic executed on the host (never used by the
 * product path; lets a GPU-less container check the hash and second-stage lane logic) --------------------- */
int mhap_selftest_hash_windows(const char* seq, int32_t len, int32_t k, int32_t k2, int64_t* out64, int32_t* out32);
int mhap_selftest_bloom(const int64_t* hashes, int64_t n, int64_t size_bloom, const int64_t* probes, int64_t np, uint8_t* out_flags,
                        int64_t* out2);
int mhap_selftest_transpose32(uint32_t* a32);
/* the (inter, k) identity table (J/sketch/BottomOverlapSketch.java:391-395; scores[k (k + 1) / 2 + inter], k <= S; may be NULL) and the
 * second stage's early-reject table derived from it: pass_min[k] = smallest inter with score >= threshold for any k' >= k (S + 2 entries) */
int mhap_selftest_pass_min(int32_t S, int32_t k2, double threshold, double* scores, int32_t* pass_min);
/* the sketch driver's host rules on n reads of the given lengths and flags (2 = skipped, 1 = raw bytes; fused = 0: every read's hashes are
 * materialised).  plan8 = {bases per launch group from free_bytes and the override (> 0 wins), groups, max key / 32-bit hash / weight elements,
 * max reads of a group, longest read, slab entries}; per read group_of[i], layout[6 i ..] = {w_off, key_off, h2_off, key_stride, h2_stride,
 * flags out} and order[i] = the i-th read (within its group) handed out, or -1 where the group keeps the input order; per group
 * totals[6 g ..] = {key, hash, weight elements, longest and shortest read not skipped, read bases}.  n = 0: plan8 only. */
int mhap_selftest_sketch_plan(uint64_t free_bytes, int64_t group_bases_override, const int32_t* lengths, const int32_t* flags, int64_t n,
                              int32_t k, int32_t k2, int32_t fused, int64_t* plan8, int64_t* group_of, int64_t* layout, int64_t* totals,
                              int32_t* order);
/* where the ordered kernel runs around the MinHash launch, under the MHAP_ORDERED_* / MHAP_W1_PREFILL switches of the environment:
 * out5 = {strands in front of the launch, no wait, idle gap, prefills, all rows in front} */
int mhap_selftest_ordered_schedule(int64_t group_read_bases, int64_t n_w1, int64_t n_weighted, int64_t nstr, int32_t eager_x, int64_t* out5);
int mhap_selftest_xorshift_jump(uint64_t key, int32_t nsteps, uint64_t* out);
int mhap_selftest_xorshift_unjump(uint64_t x, int32_t nsteps, uint64_t* out);   /* the key nsteps steps before chain value x */
/* the k-mer counter's window values of one read's bytes: out[i] / valid[i] for the window starting at i (len - k + 1 of each) */
int mhap_selftest_kmer_windows(const char* seq, int32_t len, int32_t k, int32_t canonical, uint64_t* out, uint8_t* valid);
/* the lane arithmetic of the sequence evaluation on the host, against a bitmap of 4^k bits in host memory (at least 16 bytes): row[4] =
 * windows, missing, runs, unsupported; umask (may be NULL): 63 words for every 4032 positions, a bit per unsupported position */
int mhap_selftest_kmer_eval(const char* seq, int32_t len, int32_t k, int32_t canonical, const uint32_t* bits, int64_t* row, uint64_t* umask);
/* out8 = {empty, valid(rawScore), a1, a2, b1, b2, inter, k} */
int mhap_selftest_overlap_lane(const int32_t* A, int32_t nA, int32_t lenA, const int32_t* B, int32_t nB, int32_t lenB,
                               double max_shift, int32_t stride, int32_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* MHAP_HIP_H */
