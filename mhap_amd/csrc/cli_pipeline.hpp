// cli_pipeline.hpp — what `mhap-hip --realign` does with every batch of found overlaps and after the last one: the reads' table, a
// realigned batch, one struct per stage (--best-overlaps, --correct, --variant-filter, --repeat-filter, --trim, --gfa) and the Pipeline that wires them.  Host only, over the C ABI of
// libmhaphip.so.  A call made per batch returns the library's code (the sink reports it); what runs before the first or after the last batch dies on an error.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/mhap_hip.h"

namespace cli {

inline double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
[[noreturn]] inline void die(const std::string& m) { fprintf(stderr, "Exception in mhap-hip: %s\n", m.c_str()); exit(1); }
inline void chk(mhap_handle* h, int rc) { if (rc != MHAP_OK) die(std::string(mhap_last_error(h)) + " (code " + std::to_string(rc) + ")"); }
inline long long ll(int64_t v) { return (long long)v; }   // a count as %lld takes it
struct Tick { double& sum; double t0 = now(); ~Tick() { sum += now() - t0; } };   // the seconds of a scope onto a stage's counter
template <class T> std::vector<T> room(int64_t n, int per = 1) { return std::vector<T>((size_t)std::max<int64_t>(n, 1) * per); }   // never empty: data() is not null

struct Headers { std::map<int64_t, std::string> byid; bool full = false; };
inline Headers g_headers;
inline std::string header_of(int64_t id) {   // SequenceId.getHeader (J/impl/SequenceId.java:102-108)
  if (g_headers.full) { auto it = g_headers.byid.find(id); if (it != g_headers.byid.end()) return it->second; }
  return std::to_string(id);
}

// A buffered output file: opened or the driver dies, flushed at 8 MB (Utils.BUFFER_BYTE_SIZE), closed or the driver dies.
struct Writer {
  std::string name, buf;
  FILE* f;
  explicit Writer(FILE* open) : f(open) {}   // stdout: never closed
  explicit Writer(const std::string& n) : name(n), f(fopen(n.c_str(), "wb")) { if (!f) fail(); }
  [[noreturn]] void fail() const { die("cannot write " + name); }
  void flush() { if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), f); buf.clear(); }
  void put(const char* p, size_t n) { buf.append(p, n); if (buf.size() > (8u << 20)) flush(); }
  void put(const std::string& s) { put(s.data(), s.size()); }
  void close() { flush(); if (fclose(f) != 0) fail(); }
};

template <class T> void compact(std::vector<T>& v, const std::vector<uint8_t>& keep) {   // v[q] stays where keep[q] is set
  size_t w = 0;
  for (size_t q = 0; q < v.size(); q++) if (keep[q]) v[w++] = v[q];
  v.resize(w);
}
// r[0..n) appended to what a stage holds; `whole`: they are all of that vector and arrive after the last batch, so it is taken as it is
inline void hold_records(std::vector<mhap_record>& held, const mhap_record* r, int64_t n, std::vector<mhap_record>* whole) {
  if (whole && held.empty()) held.swap(*whole);
  else held.insert(held.end(), r, r + n);
}

// --correct-fastq, --gfa-consensus-fastq: the file, the two parameters, and the one formatter and the one stderr line both stages use
struct Quality {
  std::string fastq; mhap_quality_params p;
  bool on() const { return !fastq.empty(); }
  static void record(Writer& w, const std::string& header, const uint8_t* seq, const uint8_t* quals, size_t n) {   // @header, the bases, +, Phred+33
    w.put("@" + header + "\n");
    w.put((const char*)seq, n);
    w.put("\n+\n", 3);
    std::string q(n, '!');
    for (size_t i = 0; i < n; i++) q[i] = (char)(33 + quals[i]);
    w.put(q + "\n");
  }
  static void line(const int64_t* hist) {
    long long n = 0, below10 = 0, below20 = 0, sum = 0;
    for (int q = 0; q < MHAP_QUALITY_BINS; q++) { n += hist[q]; sum += (long long)q * hist[q]; if (q < 10) below10 += hist[q]; if (q < 20) below20 += hist[q]; }
    fprintf(stderr, "Qualities: %lld bytes, %lld below Q10, %lld below Q20, mean %.1f\n", n, below10, below20, n ? (double)sum / (double)n : 0.0);
  }
};

// A one-byte-per-base copy of every read the search has seen (the index's, then each -q file's) and the table of their ids, places and lengths.
struct Reads {
  std::vector<uint8_t> bases; std::vector<int64_t> ids, offsets; std::vector<int32_t> lengths;
  std::vector<uint8_t> quals;   // --weigh-qualities: one Phred byte per base, parallel to bases (a trimmed read's are the matching slice); else empty
  int64_t n() const { return (int64_t)ids.size(); }
  void add(const mhap_fasta& fa, const uint8_t* q = nullptr) {
    for (int64_t i = 0; i < fa.n; i++) { ids.push_back(fa.ids[i]); offsets.push_back((int64_t)bases.size() + fa.offsets[i]); lengths.push_back(fa.lengths[i]); }
    bases.insert(bases.end(), (const uint8_t*)fa.bases, (const uint8_t*)fa.bases + fa.total_bases);
    if (q) quals.insert(quals.end(), q, q + fa.total_bases);
  }
  // One file of -s into the table.  weigh (--weigh-qualities): with its base qualities, which a FASTA file does not bring.
  void read_file(const std::string& path, bool weigh, const std::function<void(const mhap_fasta&)>& seen = nullptr) {
    char err[512] = {0};
    mhap_fasta fa;
    uint8_t* q = nullptr;
    if ((weigh ? mhap_fasta_read_qualities(path.c_str(), n(), &fa, &q, err, sizeof err) : mhap_fasta_read(path.c_str(), n(), &fa, err, sizeof err)) != MHAP_OK) die(err);
    if (weigh && !q) { printf("--weigh-qualities needs the base qualities of FASTQ reads: %s is FASTA.\n", path.c_str()); exit(1); }
    if (seen) seen(fa);
    add(fa, q);
    mhap_qualities_free(q);
    mhap_fasta_free(&fa);
  }
  // the stderr line of --weigh-qualities: the A, C, G, T bases of the reads per weight class
  void weight_line(const mhap_weight_params& w) const {
    long long c[3] = {0, 0, 0};
    for (size_t i = 0; i < quals.size(); i++) {
      const uint8_t b = bases[i];
      if (b == 'A' || b == 'C' || b == 'G' || b == 'T') c[(quals[i] >= w.q_lo ? 1 : 0) + (quals[i] >= w.q_hi ? 1 : 0)]++;
    }
    fprintf(stderr, "Weights: q_lo = %d, q_hi = %d; %lld bases of weight 1, %lld of weight 2, %lld of weight 3\n", w.q_lo, w.q_hi, c[0], c[1], c[2]);
  }
  // the table rewritten onto the surviving trimmed reads (the bases stay where they are: a trimmed read begins `begin` bytes later)
  void retrim(const std::vector<int32_t>& rows /* n x 4: begin, end, .. */, const std::vector<uint8_t>& flags) {
    size_t live = 0;
    for (size_t r = 0; r < ids.size(); r++) {
      if (flags[r] & MHAP_TRIM_DELETED) continue;
      ids[live] = ids[r];
      offsets[live] = offsets[r] + rows[r * 4];
      lengths[live++] = rows[r * 4 + 1] - rows[r * 4];
    }
    ids.resize(live); offsets.resize(live); lengths.resize(live);
  }
};

// What a stage may look at for one realigned batch.
struct Batch {
  const mhap_record* in = nullptr;             // the records as they were found
  std::vector<mhap_record> out;                // as realigned; the k kept ones in front
  int64_t k = 0;
  std::vector<int64_t> row;                    // row[i]: the batch row of kept record i
  std::vector<int32_t> detail; std::vector<int64_t> op_offsets; std::vector<uint32_t> ops;   // asked for with paths: every row's columns and runs
  mhap_align_paths* paths = nullptr; std::vector<int64_t> kept_offsets; std::vector<uint32_t> kept_ops;   // the kept records' paths (Realigner::gather), from their runs side by side
  const mhap_record* cut = nullptr; std::vector<mhap_record> refined;   // the kept records as the pile-ups take them: out, or (TrimStage::refine) each cut to the best stretch of its path
  ~Batch() { mhap_align_paths_free(paths); }
};

// --realign: the banded aligner over a batch; what has no alignment or too low an identity is dropped
struct Realigner {
  mhap_handle* h = nullptr; const Reads* reads = nullptr; int32_t band = 0; double min_identity = 0.0;
  int64_t dropped = 0, kept = 0; double seconds = 0.0;
  int run(const mhap_record* r, int64_t n, bool with_paths, Batch& b) {
    Tick t{seconds};
    const Reads& R = *reads;
    b.in = r;
    b.out.resize((size_t)n);
    if (with_paths) b.detail.resize((size_t)n * 3);
    mhap_align_paths* all = nullptr;
    const int rc = with_paths ? mhap_realign_records_paths(h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(), R.lengths.data(), R.n(), r, n,
                                                           band, b.out.data(), b.detail.data(), &all)
                              : mhap_realign_records(h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(), R.lengths.data(), R.n(), r, n, band,
                                                     b.out.data(), nullptr);
    if (rc != MHAP_OK) return rc;
    if (with_paths) {
      int64_t n_ops = 0;
      mhap_align_paths_info(all, nullptr, &n_ops);
      b.op_offsets.resize((size_t)n + 1); b.ops.resize((size_t)std::max<int64_t>(n_ops, 1));
      mhap_align_paths_copy(all, b.op_offsets.data(), b.ops.data());
      mhap_align_paths_free(all);
    }
    b.k = 0;
    b.row.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const mhap_record& o = b.out[(size_t)i];
      const bool none = o.score == 0.0 && o.a1 == 0 && o.a2 == 0 && o.b1 == 0 && o.b2 == 0;
      if (none || o.score < min_identity) continue;
      b.row[(size_t)b.k] = i;
      b.out[(size_t)b.k++] = o;
    }
    dropped += n - b.k; kept += b.k;
    b.cut = b.out.data();
    return MHAP_OK;
  }
  int gather(Batch& b) const {   // the kept records' runs into paths of their own (the dropped ones cast no vote)
    b.kept_offsets.assign(1, 0); b.kept_ops.clear();
    for (int64_t i = 0; i < b.k; i++) {
      const int64_t q = b.row[(size_t)i];
      b.kept_ops.insert(b.kept_ops.end(), b.ops.begin() + b.op_offsets[(size_t)q], b.ops.begin() + b.op_offsets[(size_t)q + 1]);
      b.kept_offsets.push_back((int64_t)b.kept_ops.size());
    }
    mhap_align_paths_free(b.paths);
    return mhap_align_paths_from_runs(b.kept_offsets.data(), b.k, b.kept_ops.data(), &b.paths);
  }
};

struct Stage { mhap_handle* h = nullptr; bool on = false; double seconds = 0.0; };   // what every stage has: the handle, its flag, its own seconds

// --hpc, in front of the search and of everything behind it: the reads of one side (the index's, or one -q file's) homopolymer-compressed
// on the GPU and copied back for the sketching under the same ids; the object keeps the maps on the device for the records' way back
struct HpcSide {
  mhap_hpc* c = nullptr; int64_t first = 0, n = 0;   // reads [first, first + n) of the table
  std::vector<uint8_t> bases; std::vector<int64_t> offsets; std::vector<int32_t> lengths;
};
struct HpcStage : Stage {
  Reads own;                      // the raw reads when no pipeline keeps them
  Reads* reads = &own;
  HpcSide index, query;
  bool querying = false;          // the records coming are a -q file's against the index
  int64_t counts[MHAP_HPC_COUNTS] = {0, 0, 0, 0, 0, 0}, records = 0;
  std::vector<mhap_record> raw;
  // reads first .. of the table compressed into s (what s held is freed)
  void compress(int64_t first, HpcSide& s) {
    Tick t{seconds};
    const Reads& R = *reads;
    mhap_hpc_free(s.c);
    s.c = nullptr; s.first = first; s.n = R.n() - first;
    chk(h, mhap_hpc_compress(h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data() + first, R.offsets.data() + first, R.lengths.data() + first, s.n, 0, &s.c));
    int64_t c[MHAP_HPC_COUNTS];
    mhap_hpc_info(s.c, c);
    for (int k = 0; k < MHAP_HPC_COUNTS; k++) counts[k] = k == 4 ? std::max(counts[k], c[k]) : counts[k] + c[k];   // (4: the longest run)
    s.bases = room<uint8_t>(c[2]); s.offsets = room<int64_t>(s.n + 1); s.lengths = room<int32_t>(s.n);
    chk(h, mhap_hpc_copy(s.c, s.bases.data(), s.offsets.data(), s.lengths.data(), nullptr));
  }
  const int64_t* ids(const HpcSide& s) const { return reads->ids.data() + s.first; }
  // a batch of found records onto the raw reads, before anything else sees it
  int expand(const mhap_record*& r, int64_t n) {
    Tick t{seconds};
    raw.resize((size_t)n);
    const int rc = querying ? mhap_hpc_expand_records(query.c, index.c, r, n, raw.data()) : mhap_hpc_expand_records(index.c, nullptr, r, n, raw.data());
    if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(h), rc); return rc; }
    records += n;
    r = raw.data();
    return MHAP_OK;
  }
  void finish() {
    mhap_hpc_free(index.c); mhap_hpc_free(query.c);
    index.c = query.c = nullptr;
    fprintf(stderr, "Homopolymer compression: %lld reads (%lld empty), %lld bases compressed to %lld; %lld runs longer than 1, the longest of %lld\n", ll(counts[0]),
            ll(counts[5]), ll(counts[1]), ll(counts[2]), ll(counts[3]), ll(counts[4]));
    fprintf(stderr, "Time (s) to compress the reads and expand %lld overlaps: %g\n", ll(records), seconds);
  }
};

// --correct: every kept record votes on both of its reads, or (add_selected) with the views the selection kept
struct CorrectStage : Stage {
  std::string fasta; int32_t min_cov = 0; mhap_correct_session* s = nullptr; Quality quality;
  bool weigh = false; mhap_weight_params wp;   // --weigh-qualities: the votes weigh the reads' own base qualities
  void begin(const Reads& R) {
    chk(h, mhap_correct_begin_weighted(h, R.bases.data(), weigh ? R.quals.data() : nullptr, (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(),
                                       R.lengths.data(), R.n(), &wp, &s));
  }
  int add(const Batch& b) { Tick t{seconds}; return mhap_correct_add(s, b.out.data(), b.k, b.paths); }
  // the records as they came give the alignments of the first pass again (the aligner is deterministic), now with their paths, 65 536 at a time
  void add_selected(const std::vector<mhap_record>& found, const std::vector<uint8_t>& views, Realigner& A) {
    Tick t{seconds};
    Batch b;
    std::vector<uint8_t> kv;
    const int64_t total = (int64_t)found.size(), step = 1 << 16;
    for (int64_t q0 = 0; q0 < total; q0 += step) {
      chk(h, A.run(found.data() + q0, std::min(step, total - q0), true, b));   // (the first pass's rule once more: nothing is dropped unless the aligner differs)
      if (A.gather(b) != MHAP_OK) die("the paths of the selected overlaps");
      kv.resize((size_t)b.k);
      for (int64_t i = 0; i < b.k; i++) kv[(size_t)i] = views[(size_t)(q0 + b.row[(size_t)i])];
      chk(h, mhap_correct_add_views(s, b.out.data(), b.k, b.paths, kv.data()));
    }
  }
  void finish(const Reads& R) {   // the call for every read, after the last vote; the FASTA file, and with --correct-fastq the FASTQ file, is all it writes
    const double t0 = now();
    const int64_t nr = R.n();
    std::vector<int64_t> off((size_t)nr + 1); std::vector<int32_t> st = room<int32_t>(nr, 6);
    int64_t skipped = 0;
    chk(h, mhap_correct_finish(s, min_cov, off.data(), st.data(), &skipped));
    std::vector<uint8_t> bytes = room<uint8_t>(off[(size_t)nr]);
    chk(h, mhap_correct_copy(s, bytes.data()));
    std::vector<uint8_t> quals = room<uint8_t>(quality.on() ? off[(size_t)nr] : 0);
    int64_t hist[MHAP_QUALITY_BINS];
    if (quality.on()) chk(h, mhap_correct_quality(s, &quality.p, quals.data(), hist));
    mhap_correct_free(s);
    Writer w(fasta);
    long long tot[6] = {0, 0, 0, 0, 0, 0};
    std::vector<std::string> fields((size_t)nr);   // what follows '>' and, in the FASTQ file, '@'
    for (int64_t r = 0; r < nr; r++) {
      const int32_t* c = st.data() + 6 * r;
      for (int u = 0; u < 6; u++) tot[u] += c[u];
      fields[(size_t)r] = header_of(R.ids[(size_t)r]) + " len=" + std::to_string(c[1]) + " sub=" + std::to_string(c[2]) + " del=" + std::to_string(c[3]) + " ins=" + std::to_string(c[4]) +
                          " low=" + std::to_string(c[5]);
      w.put(">" + fields[(size_t)r] + "\n");
      w.put((const char*)bytes.data() + off[(size_t)r], (size_t)(off[(size_t)r + 1] - off[(size_t)r]));
      w.put("\n", 1);
    }
    w.close();
    if (quality.on()) {
      Writer wq(quality.fastq);
      for (int64_t r = 0; r < nr; r++) Quality::record(wq, fields[(size_t)r], bytes.data() + off[(size_t)r], quals.data() + off[(size_t)r], (size_t)(off[(size_t)r + 1] - off[(size_t)r]));
      wq.close();
    }
    seconds += now() - t0;
    fprintf(stderr, "Corrected %lld reads: %lld bases in, %lld out; %lld substitutions, %lld deletions, %lld insertions, %lld positions of low coverage; skipped_views = %lld\n",
            ll(nr), tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], ll(skipped));
    if (quality.on()) Quality::line(hist);
    fprintf(stderr, "Time (s) to vote and correct: %g\n", seconds);
  }
};

// --best-overlaps: every kept record gives its two views to the selection (queued: nothing waits)
struct SelectStage : Stage {
  mhap_select_params p; std::string table; mhap_select_session* s = nullptr;
  bool hold = false;                          // someone votes with the kept views: the records as found and as realigned wait for the thresholds
  std::vector<mhap_record> found, realigned; std::vector<uint8_t> views;   // after finish: found holds the records that keep a view, views their view bits
  void begin(const Reads& R) { chk(h, mhap_select_begin(h, R.ids.data(), R.lengths.data(), R.n(), &p, &s)); }
  int add(const Batch& b) {
    Tick t{seconds};
    for (int64_t i = 0; hold && i < b.k; i++) found.push_back(b.in[b.row[(size_t)i]]);
    if (hold) realigned.insert(realigned.end(), b.out.data(), b.out.data() + b.k);
    return mhap_select_add(s, b.out.data(), b.k);
  }
  void finish(const Reads& R) {   // every read's threshold after the last batch, and the views the held records keep
    const double t0 = now();
    const int64_t nr = R.n(), nh = (int64_t)realigned.size();
    int64_t c[MHAP_SELECT_COUNTS];
    chk(h, mhap_select_finish(s, c));
    if (!table.empty()) {
      std::vector<int32_t> rows = room<int32_t>(nr, 4);
      chk(h, mhap_select_copy(s, rows.data()));
      Writer w(table);
      for (size_t r = 0; r < (size_t)nr; r++)
        w.put(header_of(R.ids[r]) + " " + std::to_string(rows[4 * r]) + " " + std::to_string(rows[4 * r + 1]) + " " + std::to_string(rows[4 * r + 2]) + "\n");
      w.close();
    }
    views = room<uint8_t>(nh);
    if (hold) chk(h, mhap_select_apply(s, realigned.data(), nh, views.data()));
    mhap_select_free(s);
    compact(found, views);
    views.erase(std::remove(views.begin(), views.end(), 0), views.end());
    std::vector<mhap_record>().swap(realigned);
    seconds += now() - t0;
    fprintf(stderr, "Best overlaps: %lld reads, %lld with a view, %lld cut; %lld of %lld views kept; %lld eligible overlaps\n", ll(c[0]), ll(c[1]), ll(c[2]), ll(c[4]), ll(c[3]), ll(c[5]));
    fprintf(stderr, "Time (s) to select the best overlaps: %g\n", seconds);
  }
};

// --variant-filter: every kept record votes with its path, batch by batch, and waits as it was found; after the last batch the sites are
// made, the held records are realigned a second time (the aligner is deterministic: CorrectStage::add_selected), judged against the
// sites, and each step's survivors go on to the stages behind.  The paths are not kept between the passes: about 12 kB per 10 kb overlap.
struct VariantStage : Stage {
  mhap_variant_params p; std::string table; mhap_variant_session* s = nullptr;
  std::vector<mhap_record> found;             // the kept records as found
  double second_pass = 0.0;                   // of `seconds`, the realignment of the second pass
  void begin(const Reads& R) { chk(h, mhap_variant_begin(h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(), R.lengths.data(), R.n(), &p, &s)); }
  int add(const Batch& b) {
    Tick t{seconds};
    for (int64_t i = 0; i < b.k; i++) found.push_back(b.in[b.row[(size_t)i]]);
    return mhap_variant_add(s, b.out.data(), b.k, b.paths);
  }
  // the sites of every read, the table, and the judgement of the held records in steps of 65 536; feed(b): the stages behind take b's kept records
  template <class Feed> void finish(const Reads& R, Realigner& A, Batch& b, Feed feed) {
    double t0 = now();
    const int64_t nr = R.n(), total = (int64_t)found.size(), step = 1 << 16;
    int64_t c[MHAP_VARIANT_COUNTS], judged = 0, aside = 0;
    chk(h, mhap_variant_finish(s, c));
    if (!table.empty()) {
      std::vector<int32_t> rows = room<int32_t>(nr, 2), sites = room<int32_t>(c[2], 6);
      std::vector<int64_t> off((size_t)nr + 1);
      chk(h, mhap_variant_copy(s, rows.data(), off.data(), sites.data()));
      Writer w(table);
      for (int64_t r = 0; r < nr; r++)
        for (int64_t i = off[(size_t)r]; i < off[(size_t)r + 1]; i++) {
          const int32_t* x = sites.data() + 6 * i;
          w.put(std::to_string(R.ids[(size_t)r]) + "\t" + std::to_string(x[0]) + "\t" + "ACGT"[x[1] & 3] + "\t" + "ACGT"[x[2] & 3] + "\t" + std::to_string(x[3]) + "\t" + std::to_string(x[4]) + "\t" +
                std::to_string(x[5]) + "\n");
        }
      w.close();
    }
    std::vector<uint8_t> keep; std::vector<int32_t> tallies;
    for (int64_t q0 = 0; q0 < total; q0 += step) {
      const double t1 = now();
      chk(h, A.run(found.data() + q0, std::min(step, total - q0), true, b));   // (the first pass's rule once more: nothing is dropped unless the aligner differs)
      if (A.gather(b) != MHAP_OK) die("the paths of the overlaps to judge");
      second_pass += now() - t1;
      keep = room<uint8_t>(b.k); tallies = room<int32_t>(b.k, 4);
      chk(h, mhap_variant_apply(s, b.out.data(), b.k, b.paths, keep.data(), tallies.data()));
      int64_t w = 0;   // the batch compacted to the survivors: the records, their rows and, from those, their paths
      for (int64_t i = 0; i < b.k; i++)
        if (keep[(size_t)i]) { b.out[(size_t)w] = b.out[(size_t)i]; b.row[(size_t)w++] = b.row[(size_t)i]; }
      judged += b.k; aside += b.k - w;
      b.k = w;
      if (A.gather(b) != MHAP_OK) die("the paths of the overlaps that stay");
      seconds += now() - t0;   // (the stages behind count their own)
      chk(h, feed(b));
      t0 = now();
    }
    mhap_variant_free(s);
    std::vector<mhap_record>().swap(found);
    seconds += now() - t0;
    fprintf(stderr, "Variant sites: %lld reads, %lld with a site; %lld sites, %lld of %lld positions deep; %lld views, skipped_views = %lld; %lld of %lld overlaps set aside\n",
            ll(c[0]), ll(c[1]), ll(c[2]), ll(c[3]), ll(c[4]), ll(c[5]), ll(c[6]), ll(aside), ll(judged));
    fprintf(stderr, "Time (s) to mark variant sites and judge: %g (%g to realign a second time)\n", seconds, second_pass);
  }
};

// --repeat-filter: the cut copies are piled up (queued: nothing waits); every kept record waits to be judged after the last batch
struct RepeatStage : Stage {
  mhap_repeat_params p; std::string table; mhap_repeat_session* s = nullptr;
  bool hold_out = false;                      // someone takes the survivors as realigned: those copies wait too
  std::vector<mhap_record> cut, out;          // after finish: the survivors, cut and (held) as realigned
  void begin(const Reads& R) { chk(h, mhap_repeat_begin(h, R.ids.data(), R.lengths.data(), R.n(), &p, &s)); }
  int add(const Batch& b) {
    Tick t{seconds};
    cut.insert(cut.end(), b.cut, b.cut + b.k);
    if (hold_out) out.insert(out.end(), b.out.data(), b.out.data() + b.k);
    return mhap_repeat_add(s, b.cut, b.k);
  }
  void finish(const Reads& R) {   // the intervals of every read and the judgement of every held record
    const double t0 = now();
    const int64_t nr = R.n(), nk = (int64_t)cut.size();
    int64_t c[MHAP_REPEAT_COUNTS];
    chk(h, mhap_repeat_finish(s, c));
    if (!table.empty()) {
      std::vector<int32_t> rows = room<int32_t>(nr, 4), iv = room<int32_t>(c[3], 2);
      std::vector<uint8_t> flags = room<uint8_t>(nr);
      std::vector<int64_t> off((size_t)nr + 1);
      chk(h, mhap_repeat_copy(s, rows.data(), flags.data(), off.data(), iv.data()));
      Writer w(table);
      for (int64_t r = 0; r < nr; r++)
        for (int64_t i = off[(size_t)r]; i < off[(size_t)r + 1]; i++) w.put(std::to_string(R.ids[(size_t)r]) + "\t" + std::to_string(iv[(size_t)i * 2]) + "\t" + std::to_string(iv[(size_t)i * 2 + 1]) + "\n");
      w.close();
    }
    std::vector<uint8_t> keep = room<uint8_t>(nk); std::vector<int32_t> unique = room<int32_t>(nk, 2);
    chk(h, mhap_repeat_apply(s, cut.data(), nk, keep.data(), unique.data()));
    mhap_repeat_free(s);   // (its device arrays go before the next stage allocates its own)
    compact(cut, keep);
    compact(out, keep);
    seconds += now() - t0;
    fprintf(stderr, "Repeats: %lld reads, %lld with a repeat, %lld repeat throughout; %lld intervals, %lld of %lld bases; %lld eligible overlaps, depth %lld, threshold %lld\n",
            ll(c[0]), ll(c[1]), ll(c[2]), ll(c[3]), ll(c[4]), ll(c[5]), ll(c[6]), ll(c[7]), ll(c[8]));
    fprintf(stderr, "Time (s) to mark repeats: %g (%lld of %lld overlaps set aside)\n", seconds, ll(nk - (int64_t)cut.size()), ll(nk));
  }
};

// --gfa: every record it is given is classed for the string graph (queued: nothing waits); finish cleans, compacts into unitigs, spells them or calls their consensus
struct GraphStage : Stage {
  mhap_graph_params p; std::string gfa, unitigs, consensus_fasta; mhap_graph_session* s = nullptr;
  bool weigh = false; mhap_weight_params wp;   // --weigh-qualities, for the consensus
  bool clean = false, consensus = false; mhap_clean_params cp; mhap_consensus_params kp; Quality quality; int64_t qhist[MHAP_QUALITY_BINS];
  std::vector<mhap_record> held;              // --gfa-consensus: the consensus takes what the graph took
  int64_t uc[MHAP_UNITIG_COUNTS], kc[MHAP_CONSENSUS_COUNTS];
  void begin(const Reads& R) { Tick t{seconds}; chk(h, mhap_graph_begin(h, R.ids.data(), R.lengths.data(), R.n(), &p, &s)); }
  int add(const mhap_record* r, int64_t n, std::vector<mhap_record>* whole = nullptr) {
    Tick t{seconds};
    const int rc = mhap_graph_add(s, r, n);
    if (rc == MHAP_OK && consensus) hold_records(held, r, n, whole);
    return rc;
  }
  // the chains of the final arcs and their bases, while the graph is on the device: the --gfa-unitigs file and the consensus FASTA
  void write_unitigs(const Reads& R) {
    chk(h, clean ? mhap_graph_unitigs_counts(s, uc) : mhap_graph_unitigs(s, uc));   // (the clean has built the unitigs of the cleaned graph)
    const size_t nu = (size_t)uc[0], nm = (size_t)uc[2], nl = (size_t)uc[4];
    std::vector<int64_t> ustart(nu + 1), ulen(nu + 1), moff(nm + 1);
    std::vector<uint8_t> circ(nu + 1), seq((size_t)uc[6] + 1);
    std::vector<int32_t> mv(nm + 1), msp(nm + 1), links(6 * nl + 6);
    chk(h, mhap_graph_copy_unitigs(s, ustart.data(), ulen.data(), circ.data()));
    chk(h, mhap_graph_copy_layout(s, mv.data(), moff.data(), msp.data()));
    chk(h, mhap_graph_copy_links(s, links.data()));
    std::vector<int64_t> cons_off(nu + 1, 0), cons_map;   // --gfa-consensus: unitig k's bytes in seq, the position map of all unitigs
    std::vector<uint8_t> cons_quals;                       // --gfa-consensus-fastq: one quality per byte of seq
    if (!consensus) chk(h, mhap_graph_spell(s, R.bases.data(), (int64_t)R.bases.size(), R.offsets.data(), seq.data()));
    else {   // the held records, fed now that the unitigs are served; the consensus takes the place of the spelling
      mhap_consensus_session* cs = nullptr;
      chk(h, mhap_consensus_begin_weighted(s, R.bases.data(), weigh ? R.quals.data() : nullptr, (int64_t)R.bases.size(), R.offsets.data(), &kp, &wp, &cs));
      chk(h, mhap_consensus_add(cs, held.data(), (int64_t)held.size()));
      chk(h, mhap_consensus_run(cs, kc));
      int64_t n_draft = 0, n_out = 0;
      chk(h, mhap_consensus_info(cs, nullptr, nullptr, &n_draft, &n_out));
      std::vector<int64_t> stats(6 * nu + 6);
      seq.assign((size_t)n_out + 1, 0);
      cons_map.assign((size_t)n_draft + 1, 0);
      chk(h, mhap_consensus_copy(cs, seq.data(), cons_off.data(), stats.data()));
      chk(h, mhap_consensus_copy_map(cs, cons_map.data()));
      if (quality.on()) { cons_quals.assign((size_t)n_out + 1, 0); chk(h, mhap_consensus_quality(cs, &quality.p, cons_quals.data(), qhist)); }
      mhap_consensus_free(cs);
      std::vector<mhap_record>().swap(held);
    }
    Writer w(unitigs);
    w.put("H\tVN:Z:1.0\n");
    char name[32], line[128];
    size_t at = 0, draft_at = 0;   // unitig k's sequence in seq, its first position in the map
    for (size_t k = 0; k < nu; k++) {
      snprintf(name, sizeof name, "utg%06lld%c", (long long)k + 1, circ[k] ? 'c' : 'l');
      const size_t slen = consensus ? (size_t)(cons_off[k + 1] - cons_off[k]) : (size_t)ulen[k];
      w.put(std::string("S\t") + name + "\t");
      w.put((const char*)seq.data() + at, slen);
      at += slen;
      w.put("\tLN:i:" + std::to_string(slen) + "\tnr:i:" + std::to_string(ustart[k + 1] - ustart[k]) + "\n");
      for (int64_t m = ustart[k]; m < ustart[k + 1]; m++) {
        const std::string sp = std::to_string(msp[(size_t)m]);
        const int64_t off = consensus ? cons_map[draft_at + (size_t)moff[(size_t)m]] : moff[(size_t)m];
        w.put(std::string("a\t") + name + "\t" + std::to_string(off) + "\t" + std::to_string(R.ids[(size_t)(mv[(size_t)m] >> 1)]) + ":1-" + sp + "\t" +
              ((mv[(size_t)m] & 1) ? "-" : "+") + "\t" + sp + "\n");
      }
      draft_at += (size_t)ulen[k];
    }
    for (size_t i = 0; i < nl; i++) {
      const int len = mhap_format_gfa_unitig_link(links.data() + 6 * i, line, sizeof line);
      if (len < 0 || (size_t)len >= sizeof line) die("mhap_format_gfa_unitig_link failed");
      w.put(std::string(line, (size_t)len) + "\n");
    }
    w.close();
    if (consensus && quality.on()) {
      Writer wq(quality.fastq);
      for (size_t k = 0; k < nu; k++) {
        snprintf(name, sizeof name, "utg%06lld%c", (long long)k + 1, circ[k] ? 'c' : 'l');
        Quality::record(wq, name, seq.data() + cons_off[k], cons_quals.data() + cons_off[k], (size_t)(cons_off[k + 1] - cons_off[k]));
      }
      wq.close();
    }
    if (!consensus || consensus_fasta.empty()) return;
    Writer wf(consensus_fasta);
    for (size_t k = 0; k < nu; k++) {
      snprintf(name, sizeof name, ">utg%06lld%c\n", (long long)k + 1, circ[k] ? 'c' : 'l');
      wf.put(name + std::string((const char*)seq.data() + cons_off[k], (size_t)(cons_off[k + 1] - cons_off[k])) + "\n");
    }
    wf.close();
  }
  void finish(const Reads& R) {   // the list and its reduction, after the last record has been classed
    const double t0 = now();
    const int64_t nr = R.n();
    int64_t gc[MHAP_GRAPH_COUNTS], cc[MHAP_CLEAN_COUNTS];
    chk(h, mhap_graph_finish(s, gc));
    const int64_t na = gc[8];
    std::vector<int32_t> rows = room<int32_t>(na, 7);
    std::vector<uint8_t> contained = room<uint8_t>(nr), removed = room<uint8_t>(na);
    chk(h, mhap_graph_copy_arcs(s, rows.data()));
    chk(h, mhap_graph_copy_read_flags(s, contained.data()));
    if (clean) {   // tips and bubbles go before either file is written: a dropped read counts as a contained one does, a removed arc is not final
      std::vector<uint8_t> dropped = room<uint8_t>(nr);
      chk(h, mhap_graph_clean(s, &cp, cc));
      chk(h, mhap_graph_copy_dropped(s, dropped.data()));
      chk(h, mhap_graph_copy_removed(s, removed.data()));
      for (int64_t r = 0; r < nr; r++) if (dropped[(size_t)r]) contained[(size_t)r] = 1;
    }
    if (!unitigs.empty()) write_unitigs(R);
    mhap_graph_free(s);
    Writer w(gfa);
    w.put("H\tVN:Z:1.0\n");
    char line[128];
    for (int64_t r = 0; r < nr; r++)
      if (!contained[(size_t)r]) w.put("S\t" + std::to_string(R.ids[(size_t)r]) + "\t*\tLN:i:" + std::to_string(R.lengths[(size_t)r]) + "\n");
    for (int64_t i = 0; i < na; i++) {
      if (!rows[(size_t)i * 7 + 6] || removed[(size_t)i]) continue;
      const int len = mhap_format_gfa_link(rows.data() + 7 * i, R.ids.data(), line, sizeof line);
      if (len < 0 || (size_t)len >= sizeof line) die("mhap_format_gfa_link failed");
      w.put(std::string(line, (size_t)len) + "\n");
    }
    w.close();
    seconds += now() - t0;
    fprintf(stderr, "String graph of %lld overlaps: %lld none, %lld internal, %lld contained (from), %lld contained (to), %lld short, %lld dovetail; %lld contained reads, %lld arcs, %lld reduced, %lld final\n",
            ll(gc[0]), ll(gc[1]), ll(gc[2]), ll(gc[3]), ll(gc[4]), ll(gc[5]), ll(gc[6]), ll(gc[7]), ll(gc[8]), ll(gc[9]), ll(gc[10]));
    if (clean)
      fprintf(stderr, "Cleaned in %lld rounds: %lld tips (%lld reads), %lld bubbles (%lld reads), %lld arcs removed\n", ll(cc[0]), ll(cc[1]), ll(cc[2]), ll(cc[3]), ll(cc[4]), ll(cc[5]));
    if (!unitigs.empty())
      fprintf(stderr, "Unitigs: %lld unitigs (%lld circular) of %lld reads, %lld joined arcs, %lld links; longest %lld bases, %lld bases in all\n",
              ll(uc[0]), ll(uc[1]), ll(uc[2]), ll(uc[3]), ll(uc[4]), ll(uc[5]), ll(uc[6]));
    if (consensus)
      fprintf(stderr, "Consensus: %lld members, %lld reads placed by an overlap, %lld unplaced; %lld aligned, %lld without alignment; %lld bases in, %lld out: %lld substitutions, %lld deletions, %lld insertions, %lld low positions\n",
              ll(kc[0]), ll(kc[1]), ll(kc[2]), ll(kc[3]), ll(kc[4]), ll(kc[5]), ll(kc[6]), ll(kc[7]), ll(kc[8]), ll(kc[9]), ll(kc[10]));
    if (consensus && quality.on()) Quality::line(qhist);
    fprintf(stderr, "Time (s) to class, build and reduce the graph: %g\n", seconds);
  }
};

// --trim: every record it is given is piled up on its two reads (queued: nothing waits); refine is the cut both pile-ups take their records through when --trim-penalty > 0
struct TrimStage : Stage {
  mhap_trim_params p; int32_t penalty = 0; std::string fasta, table; mhap_trim_session* s = nullptr;
  bool hold = false;                          // someone builds on the trimmed reads: the records wait to be rewritten onto them
  std::vector<mhap_record> held;
  int refine(Batch& b) {   // b.cut: every kept record cut to the best stretch of its path
    Tick t{seconds};
    b.refined.resize((size_t)std::max<int64_t>(b.k, 1));
    b.cut = b.refined.data();
    return mhap_trim_refine(h, b.out.data(), b.k, b.paths, penalty, b.refined.data());
  }
  void begin(const Reads& R) { Tick t{seconds}; chk(h, mhap_trim_begin(h, R.ids.data(), R.lengths.data(), R.n(), &p, &s)); }
  int add(const mhap_record* r, int64_t n, std::vector<mhap_record>* whole = nullptr) {
    Tick t{seconds};
    const int rc = mhap_trim_add(s, r, n);
    if (rc == MHAP_OK && hold) hold_records(held, r, n, whole);
    return rc;
  }
  // every read's clear range; with a graph to feed, the held records are rewritten onto the trimmed reads, R becomes the table of those reads, and the graph begins on them
  void finish(Reads& R, GraphStage& graph) {
    const double t0 = now();
    const int64_t nr = R.n();
    int64_t c[MHAP_TRIM_COUNTS];
    chk(h, mhap_trim_finish(s, c));
    std::vector<int32_t> rows = room<int32_t>(nr, 4); std::vector<uint8_t> flags = room<uint8_t>(nr);
    chk(h, mhap_trim_copy(s, rows.data(), flags.data()));
    if (!fasta.empty()) {
      Writer w(fasta);
      for (int64_t r = 0; r < nr; r++) {
        if (flags[(size_t)r] & MHAP_TRIM_DELETED) continue;
        const int32_t* t = rows.data() + 4 * r;
        w.put(">" + header_of(R.ids[(size_t)r]) + " len=" + std::to_string(t[1] - t[0]) + " begin=" + std::to_string(t[0]) + " end=" + std::to_string(t[1]) + " runs=" + std::to_string(t[2]) + "\n");
        w.put((const char*)R.bases.data() + R.offsets[(size_t)r] + t[0], (size_t)(t[1] - t[0]));
        w.put("\n", 1);
      }
      w.close();
    }
    if (!table.empty()) {
      Writer w(table);
      for (int64_t r = 0; r < nr; r++) {
        std::string line = std::to_string(R.ids[(size_t)r]) + "\t" + std::to_string(R.lengths[(size_t)r]);
        for (int u = 0; u < 4; u++) line += "\t" + std::to_string(rows[4 * (size_t)r + u]);
        w.put(line + "\t" + std::to_string((int)flags[(size_t)r]) + "\n");
      }
      w.close();
    }
    if (hold) {
      const int64_t nk = (int64_t)held.size();
      std::vector<mhap_record> applied = room<mhap_record>(nk); std::vector<uint8_t> keep = room<uint8_t>(nk);
      chk(h, mhap_trim_apply(s, held.data(), nk, applied.data(), keep.data()));
      compact(applied, keep);
      std::vector<mhap_record>().swap(held);
      R.retrim(rows, flags);
      graph.begin(R);
      chk(h, graph.add(applied.data(), (int64_t)applied.size(), &applied));
    }
    mhap_trim_free(s);
    seconds += now() - t0;
    fprintf(stderr, "Trim: %lld reads, %lld deleted, %lld cut at 5', %lld cut at 3', %lld gapped; %lld of %lld bases kept, %lld eligible overlaps\n",
            ll(c[0]), ll(c[1]), ll(c[2]), ll(c[3]), ll(c[4]), ll(c[6]), ll(c[5]), ll(c[7]));
    fprintf(stderr, "Time (s) to pile up and trim: %g\n", seconds);
  }
};

// The stages of one run and which feeds which.  The three functions below are the only place that says so.
struct Pipeline {
  Reads reads; Realigner realign; bool paf = false;   // paf: --realign-paf, the sink prints the batch's paths
  SelectStage select; CorrectStage correct; VariantStage variant; RepeatStage repeat; TrimStage trim; GraphStage graph;
  Batch b; bool refine = false, kept_paths = false, all_paths = false;
  void begin() {   // the stages' parameters and `on` are set: the sessions that can begin before the search do
    refine = (trim.on || repeat.on) && trim.penalty > 0;      // the pile-ups take each record cut to the best stretch of its path
    kept_paths = (correct.on && !select.on) || refine || variant.on;   // the correction votes batch by batch unless the selection feeds it
    all_paths = paf || kept_paths;
    select.hold = correct.on;                                 // the correction's votes: the selection's kept views, else each batch
    repeat.hold_out = graph.on && !trim.on;                   // the graph's records: the trimming's rewritten ones, else the repeat stage's survivors as realigned, else each batch
    trim.hold = graph.on;                                     // the trimming's records: the repeat stage's survivors (cut), else each batch's cut
    if (select.on) select.begin(reads);
    if (correct.on) correct.begin(reads);
    if (variant.on) variant.begin(reads);
    if (repeat.on) repeat.begin(reads);                       // (the trimming begins once the repeat stage has freed its device arrays)
    else if (trim.on) trim.begin(reads);
    if (graph.on && !trim.on) graph.begin(reads);             // (with the trimming the graph begins after it, on the trimmed reads)
  }
  // the kept records of a batch, with their paths, to the pile-ups and the graph: each batch as it is realigned, or with --variant-filter the survivors of each step of its second pass
  int feed(Batch& x) {
    int rc = refine ? trim.refine(x) : MHAP_OK;
    if (rc == MHAP_OK && repeat.on) rc = repeat.add(x);
    else if (rc == MHAP_OK && trim.on) rc = trim.add(x.cut, x.k);
    if (rc == MHAP_OK && graph.on && !trim.on && !repeat.on) rc = graph.add(x.out.data(), x.k);
    return rc;
  }
  // r[0..n) realigned and through every stage that takes its records batch by batch; what is to be printed comes back, or null after an error
  const Batch* batch(const mhap_record* r, int64_t n) {
    int rc = realign.run(r, n, all_paths, b);
    if (rc == MHAP_OK && kept_paths) rc = realign.gather(b);
    if (rc == MHAP_OK && select.on) rc = select.add(b);
    if (rc == MHAP_OK && correct.on && !select.on) rc = correct.add(b);
    if (rc == MHAP_OK) rc = variant.on ? variant.add(b) : feed(b);   // the variant filter holds every batch back: the stages behind it take its survivors after the last one
    if (rc == MHAP_OK) return &b;
    fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(realign.h), rc);
    return nullptr;
  }
  void finish() {   // after the last batch, in this order
    fprintf(stderr, "Time (s) to realign: %g (%lld overlaps kept, %lld dropped: no alignment or identity below %g)\n", realign.seconds, ll(realign.kept), ll(realign.dropped), realign.min_identity);
    if (select.on) select.finish(reads);
    if (select.on && correct.on) correct.add_selected(select.found, select.views, realign);
    if (correct.on) correct.finish(reads);
    if (variant.on) variant.finish(reads, realign, b, [&](Batch& x) { return feed(x); });
    if (repeat.on) {
      repeat.finish(reads);
      if (trim.on) { trim.begin(reads); chk(trim.h, trim.add(repeat.cut.data(), (int64_t)repeat.cut.size(), &repeat.cut)); }
      else if (graph.on) chk(graph.h, graph.add(repeat.out.data(), (int64_t)repeat.out.size(), &repeat.out));
      repeat.cut = {}; repeat.out = {};   // (what nobody took is freed)
    }
    if (trim.on) trim.finish(reads, graph);
    if (graph.on) graph.finish(reads);
  }
};

}  // namespace cli
