// mhap_cli.cpp — `mhap-hip`: native host driver over libmhaphip.so that keeps MHAP's command line, stdout
// record format, stderr timing lines and `.dat` sketch files (J/main/MhapMain.java:93-590,
// J/utils/ParseOptions.java, J/impl/SequenceSketchStreamer.java:278-395, J/impl/SequenceSketch.java:61-148).
// The reference host is Java; this image has no JVM, so the host side above the C ABI is C++ (see INTEGRATION.md
// for the JNI stub that lets the stock Java host call the same library).
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mhap_hip.h"

namespace {

struct Opt { std::string help; bool is_flag; std::string value; bool set = false; };
struct Options {
  std::vector<std::string> order;
  std::map<std::string, Opt> m;
  void add(const std::string& name, const std::string& help, const std::string& def, bool flag = false) { order.push_back(name); m[name] = Opt{help, flag, def, false}; }
  std::string s(const std::string& n) const { return m.at(n).value; }
  int i(const std::string& n) const { return atoi(m.at(n).value.c_str()); }
  double d(const std::string& n) const { return atof(m.at(n).value.c_str()); }
  bool b(const std::string& n) const { return m.at(n).value == "true"; }
  bool isset(const std::string& n) const { return m.at(n).set; }
  void setdef(const std::string& n, const std::string& v) { if (!m[n].set) m[n].value = v; }
  std::string helpText() const {
    std::string t = "MHAP: MinHash Alignment Protocol. A tool for finding overlaps of long-read sequences (such as PacBio or Nanopore) in bioinformatics.\n"
                    "\tmhap-hip: MI355X (gfx950) implementation of the MHAP overlap path.\n"
                    "\tUsage 1 (direct execution): mhap-hip -s<fasta/dat from/self file> [-q<fasta/dat to file>] [-f<kmer filter list, must be sorted>]\n"
                    "\tUsage 2 (generate precomputed binaries): mhap-hip -p<directory of fasta files> -q <output directory> [-f<kmer filter list, must be sorted>]\n";
    for (auto& n : order) { const Opt& o = m.at(n); t += "\t" + n + ", default = " + (o.is_flag ? "false" : o.value) + "\n\t\t" + o.help + "\n"; }
    return t;
  }
  // (the realignment flags are listed only when --realign is given, the correction flags only when --correct is, the graph's only
  // when --gfa is, the cleaning's only when --gfa-clean is, the consensus' only when --gfa-consensus is, the trimming's only when --trim is, the repeat stage's only when --repeat-filter is, the selection's only when --best-overlaps is: without them every line the driver writes is what it was before them)
  std::string dump() const {
    std::string t;
    for (auto& n : order) {
      if (n.compare(0, 9, "--realign") == 0 && !b("--realign")) continue;
      if (n.compare(0, 9, "--correct") == 0 && !isset("--correct")) continue;
      if (n.compare(0, 5, "--gfa") == 0 && !isset("--gfa")) continue;
      if ((n == "--gfa-clean" || n == "--gfa-tip-reads" || n == "--gfa-bubble-bases" || n == "--gfa-clean-rounds") && !b("--gfa-clean")) continue;
      if (n.compare(0, 15, "--gfa-consensus") == 0 && !b("--gfa-consensus")) continue;
      if (n.compare(0, 6, "--trim") == 0 && !b("--trim")) continue;
      if (n.compare(0, 8, "--repeat") == 0 && !b("--repeat-filter")) continue;
      if (n.compare(0, 6, "--best") == 0 && !isset("--best-overlaps")) continue;
      t += n + " = " + m.at(n).value + "\n";
    }
    return t;
  }
  // ParseOptions.process (J/utils/ParseOptions.java:209-236,327-368): flags are presence flags, others consume the next arg
  bool parse(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
      std::string k = argv[a];
      if (k == "-h" || k == "--help") { printf("%s", helpText().c_str()); return false; }
      auto it = m.find(k);
      if (it == m.end()) { printf("Unknown parameter %s, please see help menu below.\n%s", k.c_str(), helpText().c_str()); return false; }
      it->second.set = true;
      if (it->second.is_flag) it->second.value = "true";
      else { if (a + 1 >= argc) { printf("Parameter %s requires a value.\n", k.c_str()); return false; } it->second.value = argv[++a]; }
    }
    return true;
  }
};

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }
bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

std::vector<std::string> list_files(const std::string& path) {   // non-hidden entries, sorted (MhapMain.java:403-420,489-512)
  std::vector<std::string> out;
  if (!is_dir(path)) { out.push_back(path); return out; }
  DIR* d = opendir(path.c_str());
  if (!d) return out;
  while (dirent* e = readdir(d)) { std::string n = e->d_name; if (n.empty() || n[0] == '.') continue; out.push_back(path + "/" + n); }
  closedir(d);
  std::sort(out.begin(), out.end());
  return out;
}

[[noreturn]] void die(const std::string& m) { fprintf(stderr, "Exception in mhap-hip: %s\n", m.c_str()); exit(1); }
void chk(mhap_handle* h, int rc) { if (rc != MHAP_OK) die(std::string(mhap_last_error(h)) + " (code " + std::to_string(rc) + ")"); }

// One GPU (a handle) or several (a group: one rank per device, reads dealt round-robin, the exchange inside the library).
struct Engine {
  mhap_handle* h = nullptr;
  mhap_group* g = nullptr;
  int n = 1;
  mhap_handle* rank(int r) const { return g ? mhap_group_rank(g, r) : h; }
  void check(int rc) const {
    if (rc == MHAP_OK) return;
    die(std::string(g ? mhap_group_last_error(g) : mhap_last_error(h)) + " (code " + std::to_string(rc) + ")");
  }
  void add_reads(const mhap_fasta& fa) const {
    if (fa.n <= 0) return;
    check(g ? mhap_group_add_reads(g, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n) : mhap_index_add_reads(h, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n));
  }
  void add_scan(const mhap_fasta_scan* sc) const { check(g ? mhap_group_add_scan(g, sc) : mhap_index_add_scan(h, sc)); }
  void find_self(mhap_record_sink sink, void* user) const { check(g ? mhap_group_find_matches_self(g, sink, user) : mhap_find_matches_self(h, 0, -1, sink, user)); }
  void find_reads(const mhap_fasta& fa, mhap_record_sink sink, void* user) const {
    if (fa.n <= 0) return;
    check(g ? mhap_group_find_matches_reads(g, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n, sink, user)
            : mhap_find_matches_reads(h, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n, sink, user));
  }
  mhap_stats stats() const { mhap_stats st; check(g ? mhap_group_get_stats(g, &st) : mhap_get_stats(h, &st)); return st; }
  void clear() const { check(g ? mhap_group_clear(g) : mhap_index_clear(h)); }
  void destroy() { if (g) mhap_group_destroy(g); else if (h) mhap_destroy(h); g = nullptr; h = nullptr; }
};

// ---- big-endian `.dat` primitives (DataOutputStream / ByteBuffer) ----
void put8(std::string& b, uint8_t v) { b.push_back((char)v); }
void put32(std::string& b, int32_t v) { for (int s = 24; s >= 0; s -= 8) b.push_back((char)((uint32_t)v >> s)); }
void put64(std::string& b, int64_t v) { for (int s = 56; s >= 0; s -= 8) b.push_back((char)((uint64_t)v >> s)); }
void putUTF(std::string& b, const std::string& s) { b.push_back((char)(s.size() >> 8)); b.push_back((char)s.size()); b += s; }   // ASCII headers only
struct Rd {
  const uint8_t* p; size_t n, o = 0; bool ok = true;
  uint8_t u8() { if (o + 1 > n) { ok = false; return 0; } return p[o++]; }
  int32_t i32() { if (o + 4 > n) { ok = false; return 0; } uint32_t v = 0; for (int i = 0; i < 4; i++) v = (v << 8) | p[o++]; return (int32_t)v; }
  int64_t i64() { if (o + 8 > n) { ok = false; return 0; } uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[o++]; return (int64_t)v; }
  std::string utf() { if (o + 2 > n) { ok = false; return ""; } size_t l = ((size_t)p[o] << 8) | p[o + 1]; o += 2; if (o + l > n) { ok = false; return ""; } std::string s((const char*)p + o, l); o += l; return s; }
};

struct Headers { std::map<int64_t, std::string> byid; bool full = false; };
Headers g_headers;

std::string header_of(int64_t id) {   // SequenceId.getHeader (J/impl/SequenceId.java:102-108)
  if (g_headers.full) { auto it = g_headers.byid.find(id); if (it != g_headers.byid.end()) return it->second; }
  return std::to_string(id);
}

// --store-full-id: header = first token after '>' split on [\s,]+ (FastaData.java:155-156)
// --store-full-id: names of the records just read (mhap_fasta.headers), keyed by the ids they were given
void collect_headers(const mhap_fasta& fa) {
  const char* p = fa.headers;
  for (int64_t i = 0; i < fa.n && p && p < fa.headers + fa.headers_bytes; i++) {
    g_headers.byid[fa.ids[i]] = std::string(p);
    p += strlen(p) + 1;
  }
}

// --store-full-id: the names of a scanned file, keyed by the ids its records were given
void collect_headers(mhap_fasta_scan* sc) {
  const int64_t n = mhap_fasta_scan_reads(sc);
  std::vector<int64_t> ids((size_t)std::max<int64_t>(n, 1));
  const char* p = nullptr; int64_t bytes = 0;
  if (mhap_fasta_scan_info(sc, ids.data(), nullptr, &p, &bytes) != MHAP_OK) return;
  const char* e = p + bytes;
  for (int64_t i = 0; i < n && p && p < e; i++) { g_headers.byid[ids[(size_t)i]] = std::string(p); p += strlen(p) + 1; }
}

// the file the index is built from is mapped and scanned while the HIP runtime comes up
struct Preload { std::string path; mhap_fasta_scan* scan = nullptr; } g_preload;
// --realign: a one-byte-per-base copy of every read the search has seen (the index's, then each -q file's), and the handle that aligns
struct Realign {
  mhap_handle* h = nullptr;
  int32_t band = 0; double min_identity = 0.0;
  std::vector<uint8_t> bases; std::vector<int64_t> ids, offsets; std::vector<int32_t> lengths;
  std::vector<mhap_record> out;
  bool paf = false;                                   // --realign-paf: the alignments' paths too, printed as PAF lines
  std::vector<int32_t> detail; std::vector<int64_t> op_offsets, row; std::vector<uint32_t> ops;   // row[k]: the batch row of kept record k
  int64_t dropped = 0, kept = 0;
  double seconds = 0.0;
  mhap_correct_session* correct = nullptr;            // --correct: every kept record votes on both of its reads
  std::vector<int64_t> vote_offsets; std::vector<uint32_t> vote_ops;
  double correct_seconds = 0.0;
  mhap_graph_session* graph = nullptr;                // --gfa: every kept record is classed for the string graph
  double graph_seconds = 0.0;
  bool keep_records = false;                          // --gfa-consensus: the kept records wait here until the graph is finished
  std::vector<mhap_record> kept_records;
  mhap_trim_session* trim = nullptr;                  // --trim: every kept record's intervals are piled up on its two reads
  int32_t trim_penalty = 0;                           // > 0: each record is first cut to the best stretch of its path
  std::vector<mhap_record> refined;
  double trim_seconds = 0.0;
  mhap_repeat_session* repeat = nullptr;              // --repeat-filter: the refined copies are piled up; every kept record waits to be judged
  bool hold_plain = false;                            // the graph takes the survivors as realigned: those copies wait too
  std::vector<mhap_record> held_refined, held_plain;
  double repeat_seconds = 0.0;
  mhap_select_session* select = nullptr;              // --best-overlaps: every kept record gives its two views to the selection
  bool hold_select = false;                           // with --correct the votes wait: the records as they came and as realigned are held
  std::vector<mhap_record> held_in, held_out;
  double select_seconds = 0.0;
  void add(const mhap_fasta& fa) {
    for (int64_t i = 0; i < fa.n; i++) { ids.push_back(fa.ids[i]); offsets.push_back((int64_t)bases.size() + fa.offsets[i]); lengths.push_back(fa.lengths[i]); }
    bases.insert(bases.end(), (const uint8_t*)fa.bases, (const uint8_t*)fa.bases + fa.total_bases);
  }
};
struct Sink { FILE* out; std::string buf; int64_t n = 0; Realign* realign = nullptr; };
int sink_cb(const mhap_record* r, int64_t n, void* user) {
  Sink* s = (Sink*)user;
  char line[512];
  if (s->realign && n > 0) {   // the batch through the banded aligner; what has no alignment or too low an identity is dropped
    Realign& R = *s->realign;
    const double t = now();
    R.out.resize((size_t)n);
    int rc;
    const bool vote_now = R.correct && !R.select;   // (with --best-overlaps the votes are cast after the last batch)
    if (R.paf || vote_now || ((R.trim || R.repeat) && R.trim_penalty > 0)) {
      R.detail.resize((size_t)n * 3);
      mhap_align_paths* paths = nullptr;
      rc = mhap_realign_records_paths(R.h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(), R.lengths.data(),
                                      (int64_t)R.ids.size(), r, n, R.band, R.out.data(), R.detail.data(), &paths);
      if (rc == MHAP_OK) {
        int64_t n_ops = 0;
        mhap_align_paths_info(paths, nullptr, &n_ops);
        R.op_offsets.resize((size_t)n + 1); R.ops.resize((size_t)std::max<int64_t>(n_ops, 1));
        mhap_align_paths_copy(paths, R.op_offsets.data(), R.ops.data());
        mhap_align_paths_free(paths);
      }
    } else {
      rc = mhap_realign_records(R.h, R.bases.data(), (int64_t)R.bases.size(), R.ids.data(), R.offsets.data(), R.lengths.data(),
                                (int64_t)R.ids.size(), r, n, R.band, R.out.data(), nullptr);
    }
    if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
    int64_t k = 0;
    R.row.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const mhap_record& o = R.out[(size_t)i];
      const bool none = o.score == 0.0 && o.a1 == 0 && o.a2 == 0 && o.b1 == 0 && o.b2 == 0;
      if (none || o.score < R.min_identity) continue;
      R.row[(size_t)k] = i;
      if (R.hold_select) R.held_in.push_back(r[i]);
      R.out[(size_t)k++] = o;
    }
    R.dropped += n - k; R.kept += k;
    R.seconds += now() - t;
    const bool refine = (R.trim || R.repeat) && R.trim_penalty > 0;
    if (R.select) {   // the kept records' views into the selection (queued: nothing waits)
      const double ts = now();
      rc = mhap_select_add(R.select, R.out.data(), k);
      if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
      if (R.hold_select) R.held_out.insert(R.held_out.end(), R.out.data(), R.out.data() + k);
      R.select_seconds += now() - ts;
    }
    if (vote_now || refine) {   // the kept records and their runs: into the vote table, and cut to their best stretch for the trimming
      const double tc = now();
      R.vote_offsets.assign(1, 0); R.vote_ops.clear();
      for (int64_t i = 0; i < k; i++) {
        const int64_t q = R.row[(size_t)i];
        R.vote_ops.insert(R.vote_ops.end(), R.ops.begin() + R.op_offsets[(size_t)q], R.ops.begin() + R.op_offsets[(size_t)q + 1]);
        R.vote_offsets.push_back((int64_t)R.vote_ops.size());
      }
      mhap_align_paths* kept_paths = nullptr;
      rc = mhap_align_paths_from_runs(R.vote_offsets.data(), k, R.vote_ops.data(), &kept_paths);
      if (rc == MHAP_OK && vote_now) rc = mhap_correct_add(R.correct, R.out.data(), k, kept_paths);   // (the dropped ones cast no vote)
      if (vote_now) R.correct_seconds += now() - tc;
      if (rc == MHAP_OK && refine) {
        const double tt = now();
        R.refined.resize((size_t)std::max<int64_t>(k, 1));
        rc = mhap_trim_refine(R.h, R.out.data(), k, kept_paths, R.trim_penalty, R.refined.data());
        R.trim_seconds += now() - tt;
      }
      mhap_align_paths_free(kept_paths);
      if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
    }
    const mhap_record* for_trim = refine ? R.refined.data() : R.out.data();
    if (R.repeat) {   // the refined copies onto the pile-up (queued: nothing waits); trimming and graph take the survivors after the last batch
      const double tr = now();
      rc = mhap_repeat_add(R.repeat, for_trim, k);
      if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
      R.held_refined.insert(R.held_refined.end(), for_trim, for_trim + k);
      if (R.hold_plain) R.held_plain.insert(R.held_plain.end(), R.out.data(), R.out.data() + k);
      R.repeat_seconds += now() - tr;
    } else if (R.trim) {   // the kept records onto the coverage of their reads (queued: nothing waits)
      const double tt = now();
      rc = mhap_trim_add(R.trim, for_trim, k);
      if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
      R.trim_seconds += now() - tt;
    }
    if (R.graph && !R.repeat) {   // the kept records into the string graph (queued: nothing waits)
      const double tg = now();
      rc = mhap_graph_add(R.graph, R.out.data(), k);
      if (rc != MHAP_OK) { fprintf(stderr, "Exception in mhap-hip: %s (code %d)\n", mhap_last_error(R.h), rc); return 1; }
      R.graph_seconds += now() - tg;
    }
    if (R.keep_records && !R.repeat) R.kept_records.insert(R.kept_records.end(), for_trim, for_trim + k);   // (with --trim the graph takes what the trimming took)
    r = R.out.data(); n = k;
  }
  if (s->realign && s->realign->paf) {   // one PAF line per kept record; the names are columns 1 and 2 of the 12-column line
    const Realign& R = *s->realign;
    std::string pl;
    for (int64_t i = 0; i < n; i++) {
      const int64_t q = R.row[(size_t)i], o0 = R.op_offsets[(size_t)q], o1 = R.op_offsets[(size_t)q + 1];
      const std::string qn = header_of(r[i].from_id), tn = header_of(r[i].to_id);
      pl.resize(256 + qn.size() + tn.size() + 12 * (size_t)(o1 - o0));
      const int len = mhap_format_paf(&r[i], R.detail.data() + 3 * q, R.ops.data() + o0, o1 - o0, qn.c_str(), tn.c_str(), &pl[0], pl.size());
      if (len < 0 || (size_t)len >= pl.size()) { fprintf(stderr, "Exception in mhap-hip: mhap_format_paf failed\n"); return 1; }
      s->buf.append(pl.data(), (size_t)len);
      s->buf.push_back('\n');
      if (s->buf.size() > (8u << 20)) { fwrite(s->buf.data(), 1, s->buf.size(), s->out); s->buf.clear(); }
    }
    s->n += n;
    return 0;
  }
  for (int64_t i = 0; i < n; i++) {
    if (!g_headers.full) { int len = mhap_format_record(&r[i], line, sizeof line); s->buf.append(line, (size_t)len); }
    else {
      // same formatter, headers swapped in for the two id columns
      int len = mhap_format_record(&r[i], line, sizeof line);
      const char* p = line; int sp = 0; while (*p && sp < 2) { if (*p == ' ') sp++; p++; }
      s->buf += header_of(r[i].from_id) + " " + header_of(r[i].to_id) + " "; s->buf.append(p, (size_t)(line + len - p));
    }
    s->buf.push_back('\n');
    if (s->buf.size() > (8u << 20)) { fwrite(s->buf.data(), 1, s->buf.size(), s->out); s->buf.clear(); }   // 8 MB buffer (Utils.BUFFER_BYTE_SIZE)
  }
  s->n += n;
  return 0;
}
void sink_flush(Sink& s) { if (!s.buf.empty()) fwrite(s.buf.data(), 1, s.buf.size(), s.out); s.buf.clear(); fflush(s.out); }

// FrequencyCounts file -> (hash, fraction) arrays (J/sketch/FrequencyCounts.java:63-229)
void load_filter(const Engine& E, const Options& o) {
  const double rw = o.d("--repeat-weight");
  const double offset = (rw >= 0.0 && rw < 1.0) ? rw : 0.0;   // MhapMain.java:346-350
  char sizes[256];
  for (int r = 0; r < E.n; r++) {   // every rank applies the filter to the reads it sketches
    mhap_handle* h = E.rank(r);
    const int rc = mhap_set_filter_file(h, o.s("-f").c_str(), o.d("--filter-threshold"), offset, o.i("--supress-noise"), o.b("--no-tf") ? 1 : 0,
                                        o.d("--repeat-idf-scale"), o.b("--no-rc") ? 0 : 1, sizes, sizeof sizes);
    if (rc == MHAP_E_IO) die("Could not parse k-mer filter file.");
    if (rc == MHAP_E_INVALID && !*mhap_last_error(h)) die("K-mer filter file first line must contain estimated number of k-mers in the file (long).");
    chk(h, rc);
  }
  fprintf(stderr, "Read in k-mer filter for sizes: [%s]\n", sizes);
}

// `.dat` reader (SequenceSketchStreamer.readFromBinary :278-320 + SequenceSketch.fromByteStream :61-96)
struct DatEntries { std::vector<int64_t> ids; std::vector<uint8_t> fwd; std::vector<int32_t> seqlen, mh, ord, osz, olen; std::vector<std::string> hdr; };
void read_dat(const std::string& path, int64_t offset, int H, int S, bool fwd_only, DatEntries& d) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die("cannot open " + path);
  std::vector<uint8_t> data; uint8_t buf[1 << 16]; size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(f);
  Rd r{data.data(), data.size()};
  while (r.o < r.n) {
    uint8_t isFwd = r.u8(); int32_t size = r.i32();
    if (!r.ok || size < 0 || r.o + (size_t)size > r.n) break;
    Rd p{data.data() + r.o, (size_t)size}; r.o += (size_t)size;
    if (fwd_only && isFwd != 1) continue;
    uint8_t pf = p.u8(); int64_t id = p.i64() + offset; std::string hdr = p.utf(); int32_t sl = p.i32();
    int32_t hn = p.i32();
    if (!p.ok || hn != H) die("Number of MinHashes of the sequence does not match current settings.");
    d.ids.push_back(id); d.fwd.push_back(pf ? 1 : 0); d.seqlen.push_back(sl); d.hdr.push_back(hdr);
    for (int i = 0; i < H; i++) d.mh.push_back(p.i32());
    int32_t n = p.i32(); (void)p.i32(); int32_t sz = p.i32();
    if (!p.ok || sz < 0 || sz > S) die("ordered sketch in .dat larger than --ordered-sketch-size");
    d.olen.push_back(n); d.osz.push_back(sz);
    size_t base = d.ord.size(); d.ord.resize(base + (size_t)S * 2, 0);
    for (int i = 0; i < sz; i++) { d.ord[base + 2 * i] = p.i32(); d.ord[base + 2 * i + 1] = p.i32(); }
    if (!p.ok) die("Unexpected data read error.");
  }
}

// `.dat` writer (SequenceSketchStreamer.writeToBinary :322-395; SequenceSketch.getAsByteArray :123-148)
void write_dat(mhap_handle* h, const std::string& path, int H, int S, int k2) {
  int64_t n = 0; chk(h, mhap_index_size(h, &n));
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die("cannot write " + path);
  const int64_t CH = 4096;
  std::vector<int64_t> ids(CH); std::vector<uint8_t> fwd(CH), st(CH); std::vector<int32_t> sl(CH), mh(CH * H), od(CH * (size_t)S * 2), osz(CH), olen(CH);
  for (int64_t e0 = 0; e0 < n; e0 += CH) {
    const int64_t c = std::min(CH, n - e0);
    chk(h, mhap_index_export(h, e0, c, ids.data(), fwd.data(), sl.data(), mh.data(), od.data(), osz.data(), olen.data(), st.data()));
    std::string out;
    for (int64_t e = 0; e < c; e++) {
      if (st[e] != 0) continue;
      std::string pay;
      put8(pay, fwd[e]); put64(pay, ids[e]); putUTF(pay, header_of(ids[e])); put32(pay, sl[e]);
      put32(pay, H); for (int i = 0; i < H; i++) put32(pay, mh[(size_t)e * H + i]);
      put32(pay, olen[e]); put32(pay, k2); put32(pay, osz[e]);
      for (int i = 0; i < osz[e]; i++) { put32(pay, od[((size_t)e * S + i) * 2]); put32(pay, od[((size_t)e * S + i) * 2 + 1]); }
      put8(out, fwd[e]); put32(out, (int32_t)pay.size()); out += pay;
    }
    fwrite(out.data(), 1, out.size(), f);
  }
  fclose(f);
}

int64_t add_file_to_index(const Engine& E, const std::string& path, int64_t id_offset, const Options& o, int64_t* strands) {
  const int H = o.i("--num-hashes"), S = o.i("--ordered-sketch-size");
  if (ends_with(path, ".dat")) {   // MhapMain.java:563-564
    if (E.g) die("--gpus N takes FASTA input (precomputed .dat sketches are searched on one GPU)");
    mhap_handle* h = E.h;
    DatEntries d; read_dat(path, id_offset, H, S, false, d);
    if (!d.ids.empty()) chk(h, mhap_index_add_sketches(h, d.ids.data(), d.fwd.data(), d.seqlen.data(), d.mh.data(), d.ord.data(), d.osz.data(), d.olen.data(), (int64_t)d.ids.size()));
    if (g_headers.full) for (size_t i = 0; i < d.ids.size(); i++) g_headers.byid[d.ids[i]] = d.hdr[i];
    *strands = (int64_t)d.ids.size();
    return (int64_t)d.ids.size() / 2;
  }
  // FASTA: the file is mapped and scanned (record boundaries, lengths, on all host threads), then fed to the index in groups — host
  // threads pack the next group from the text while the GPU sketches the previous one (mhap_index_add_scan)
  mhap_fasta_scan* sc = nullptr; char err[512];
  const double t_read = now();
  if (g_preload.scan && g_preload.path == path && id_offset == 0) { sc = g_preload.scan; g_preload.scan = nullptr; }   // scanned while the runtime came up
  else if (mhap_fasta_scan_open(path.c_str(), id_offset, &sc, err, sizeof err) != MHAP_OK) die(err);
  if (g_headers.full) collect_headers(sc);
  const double t_add = now();
  E.add_scan(sc);
  if (getenv("MHAP_HOST_PROF")) fprintf(stderr, "[cli] fasta scan %.3f s, add (pack + upload + sketch + index, pipelined) %.3f s\n", t_add - t_read, now() - t_add);
  // (the mapping is released at exit: unmapping gigabytes holds the address-space lock the search's allocations need)
  const mhap_stats st = E.stats();
  *strands = st.strands_indexed;
  // seqNumberProcessed += seqStreamer.getNumberProcessed()/2 (MhapMain.java:462): the streamer counts the sketches it
  // produced (SequenceSketchStreamer.java:145,155,268-271), so reads below --min-olap-length and reads without a valid
  // n-gram do not advance the id offset of the -q files
  return st.strands_indexed / 2;
}

}  // namespace

int main(int argc, char** argv) {
  Options o;
  // --num-threads defaults to the CPUs the process may use: the hardware threads, capped by the container's CPU quota (cgroup v2)
  unsigned hc = std::max(1u, std::thread::hardware_concurrency());
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[64] = {0}; long long per = 0;
    if (fscanf(f, "%63s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) { const long long c = (atoll(q) + per - 1) / per; if (c > 0 && (unsigned long long)c < hc) hc = (unsigned)c; }
    fclose(f);
  }
  o.add("-s", "Usage 1 only. The FASTA or binary dat file (see Usage 2) of reads that will be stored in a box, and that all subsequent reads will be compared to.", "");
  o.add("-q", "Usage 1: The FASTA file of reads, or a directory of files, that will be compared to the set of reads in the box (see -s). Usage 2: The output directory for the binary formatted dat files.", "");
  o.add("-p", "Usage 2 only. The directory containing FASTA files that should be converted to binary format for storage.", "");
  o.add("-f", "k-mer filter file used for filtering out highly repetative k-mers. Must be sorted in descending order of frequency (second column).", "");
  o.add("-k", "[int], k-mer size used for MinHashing. The k-mer size for second stage filter is seperate, and can also be modified.", "16");
  o.add("--num-hashes", "[int], Number of min-mers to be used in MinHashing.", "512");
  o.add("--threshold", "[double], The threshold cutoff for the second stage sort-merge filter.", "0.78");
  o.add("--filter-threshold", "[double], The cutoff at which the k-mer in the k-mer filter file is considered repetitive.", "1.0E-5");
  o.add("--max-shift", "[double], Region size to the left and right of the estimated overlap where k-mer matches are still considered valid. Second stage filter only.", "0.2");
  o.add("--num-min-matches", "[int], Minimum # min-mer that must be shared before computing second stage filter.", "3");
  o.add("--num-threads", "[int], Number of host threads (FASTA packing / record conversion); the compute runs on the GPU.", std::to_string(hc));
  o.add("--repeat-weight", "[double] Repeat suppression strength for tf-idf weighing. <0.0 do unweighted MinHash (version 1.0), >=1.0 do only the tf weighing.", "0.9");
  o.add("--repeat-idf-scale", "[double] The upper range of the idf (from tf-idf) scale. The full scale will be [1,X].", "3.0");
  o.add("--ordered-kmer-size", "[int] The size of k-mers used in the ordered second stage filter.", "12");
  o.add("--ordered-sketch-size", "[int] The sketch size for second stage filter.", "1536");
  o.add("--min-store-length", "[int], The minimum length of the read that is stored in the box.", "0");
  o.add("--min-olap-length", "[int], The minimum length of the read that used for overlapping.", "116");
  o.add("--no-self", "Do not compute the overlaps between sequences inside a box.", "false", true);
  o.add("--store-full-id", "Store full IDs as seen in FASTA files, rather than storing just the sequence position in the file.", "false", true);
  o.add("--supress-noise", "[int] 0) Does nothing, 1) completely removes any k-mers not specified in the filter file, 2) supresses k-mers not specified in the filter file, similar to repeats.", "0");
  o.add("--no-tf", "Do not perform the tf weighing, in the tf-idf weighing.", "false", true);
  o.add("--no-rc", "Do not store or do comparison of the reverse compliment strings (in this MHAP version it only changes how -f k-mers are hashed).", "false", true);
  o.add("--settings", "Set all unset parameters for the default settings. 0) None, 1) Default, 2) Fast, 3) Sensitive.", "0");
  o.add("--device", "[int] HIP device ordinal (the first one with --gpus N).", "0");
  o.add("--gpus", "[int] Number of GPUs: the reads are dealt round-robin over devices --device .. --device+N-1, every GPU sketches and indexes its share, and a search gathers the forward query sketches of all GPUs (over xGMI) against every share.", "1");
  o.add("--devices", "Comma-separated HIP device ordinals, one per rank (overrides --device/--gpus; an ordinal may repeat).", "");
  o.add("--realign", "Realign every overlap on the GPU before it is printed: a banded local alignment of the two reads around the diagonal the overlap implies replaces its interval, and column 3 becomes 1 - aligned identity. FASTA input, one GPU.", "false", true);
  o.add("--realign-band", "[int] Half-width of the realignment band in bases. 0) the overlap's length times --max-shift.", "0");
  o.add("--realign-min-identity", "[double] With --realign, drop overlaps whose aligned identity is below this value (overlaps without an alignment are always dropped).", "0.0");
  o.add("--realign-paf", "With --realign, print one PAF line per overlap instead of the 12 columns: the alignment's interval, its matches and columns, and its path as a cg:Z CIGAR with = X I D.", "false", true);
  o.add("--correct", "With --realign: correct every read of -s from the realigned overlaps and write the corrected reads to this FASTA file. Each overlap votes column by column on both of its reads and every position takes the majority; overlaps that --realign drops cast no vote. Self overlaps only (no -q), one GPU.", "");
  o.add("--correct-min-coverage", "[int] With --correct, the votes a read position needs before it is changed.", "4");
  o.add("--gfa", "With --realign: build the string graph of the realigned overlaps on the GPU (dovetails, contained reads set aside, transitive arcs reduced) and write it to this file as GFA 1: an S line per read that is not contained, an L line per final arc. Self overlaps only (no -q), one GPU.", "");
  o.add("--gfa-unitigs", "With --gfa: compact the final arcs of the string graph into unitigs on the GPU and write them to this second file as GFA 1: an S line with the sequence per unitig, spelled from the reads as stored, an a line per read of it, an L line per arc between unitigs.", "");
  o.add("--gfa-max-hang", "[int] With --gfa, the longest unaligned end an overlap may leave on both reads before it counts as an internal match.", "1000");
  o.add("--gfa-min-overlap", "[int] With --gfa, the shortest overlap that becomes an arc.", "2000");
  o.add("--gfa-fuzz", "[int] With --gfa, the slack of the transitive reduction in bases.", "1000");
  o.add("--gfa-clean", "With --gfa: clean the string graph on the GPU before the files are written: tips are clipped and simple bubbles popped, in rounds. The --gfa file is then the cleaned graph and the --gfa-unitigs file holds the unitigs of the cleaned graph.", "false", true);
  o.add("--gfa-tip-reads", "[int] With --gfa-clean, the most reads a tip may have.", "4");
  o.add("--gfa-bubble-bases", "[int] With --gfa-clean, the most bases a popped bubble branch may have.", "50000");
  o.add("--gfa-clean-rounds", "[int] With --gfa-clean, the most rounds of cleaning.", "16");
  o.add("--gfa-consensus", "With --gfa-unitigs: place every read on a unitig, align it to the unitig and let the reads vote on the GPU; the --gfa-unitigs file then carries the consensus sequences, their lengths, and a-line offsets mapped into them.", "false", true);
  o.add("--gfa-consensus-fasta", "With --gfa-consensus, also write the consensus sequences to this FASTA file.", "");
  o.add("--gfa-consensus-min-cov", "[int] With --gfa-consensus, the depth below which a position keeps the unitig's own base.", "4");
  o.add("--trim", "With --realign: trim every read of -s on the GPU to the longest stretch that enough realigned overlaps cover, which also splits chimeric reads at their junction. The overlaps printed stay the untrimmed ones; with --gfa the graph, its unitigs and their consensus are built on the trimmed reads and the overlaps rewritten onto them. Self overlaps only (no -q), one GPU.", "false", true);
  o.add("--trim-min-cov", "[int] With --trim, the shrunk overlaps a position needs to be kept.", "3");
  o.add("--trim-end-clip", "[int] With --trim, the bases every aligned interval is shrunk by at both ends.", "500");
  o.add("--trim-min-span", "[int] With --trim, the shortest aligned interval that counts.", "2000");
  o.add("--trim-penalty", "[int] With --trim, every overlap is first cut to the best stretch of its alignment under +1 per match and this cost per error column, so that an overlap the aligner ran through a chimeric junction ends there. 0) overlaps as realigned.", "2");
  o.add("--repeat-filter", "With --realign: mark the repeats of every read of -s on the GPU from the pile-up of the realigned overlaps, each cut to the best stretch of its alignment (--trim-penalty), and set aside the overlaps that lie in nothing but repeat on either read: they reach neither --trim nor --gfa. The overlaps printed, --correct and --realign-paf stay on all overlaps. A repeat of two copies at ordinary depth is not reliably found. Self overlaps only (no -q), one GPU.", "false", true);
  o.add("--repeat-factor", "[int] With --repeat-filter, a position is repeat when its depth exceeds the typical depth times this, in percent.", "200");
  o.add("--repeat-max-cov", "[int] With --repeat-filter, the depth above which a position is repeat. 0) derive it from the typical depth.", "0");
  o.add("--repeat-min-run", "[int] With --repeat-filter, the shortest stretch of repeat positions that is marked.", "500");
  o.add("--repeat-min-unique", "[int] With --repeat-filter, the aligned bases outside repeats an overlap needs on both reads.", "500");
  o.add("--repeat-table", "With --repeat-filter, write one line per repeat interval to this file: read_id begin end.", "");
  o.add("--best-overlaps", "[int] With --realign: select each read's N best overlaps on the GPU, by the matches counted on that read, ties at the last place included; with --correct only the selected views of an overlap vote. The overlaps printed, --realign-paf, --gfa and --trim stay on all overlaps. 0) off. Self overlaps only (no -q), one GPU.", "0");
  o.add("--best-min-span", "[int] With --best-overlaps, the shortest aligned interval on a read that counts as evidence for it.", "500");
  o.add("--best-table", "With --best-overlaps, write one line per read to this file: read_id entries kept threshold.", "");
  o.add("--trim-fasta", "With --trim, write the trimmed reads to this FASTA file; deleted reads are left out.", "");
  o.add("--trim-table", "With --trim, write one line per read to this file: id length begin end runs covered flags.", "");
  if (!o.parse(argc, argv)) return 0;

  auto bad = [&](const char* m) { printf("%s\n", m); exit(1); };
  const int settings = o.i("--settings");
  if (settings < 0 || settings > 3) { printf("Please enter valid --settings flag. See options below:\n%s", o.helpText().c_str()); return 1; }
  if (settings == 1) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "3"); o.setdef("--num-hashes", "512"); o.setdef("--threshold", "0.78"); o.setdef("--ordered-sketch-size", "1536"); o.setdef("--ordered-kmer-size", "12"); }
  if (settings == 2) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "3"); o.setdef("--num-hashes", "256"); o.setdef("--threshold", "0.80"); o.setdef("--ordered-sketch-size", "1000"); o.setdef("--ordered-kmer-size", "14"); }
  if (settings == 3) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "2"); o.setdef("--num-hashes", "768"); o.setdef("--threshold", "0.73"); o.setdef("--ordered-sketch-size", "1536"); o.setdef("--ordered-kmer-size", "12"); }
  if (o.s("-s").empty() && o.s("-p").empty()) { printf("Please set the -s or the -p options. See options below:\n%s", o.helpText().c_str()); return 1; }
  if (!o.s("-p").empty() && o.s("-q").empty()) { printf("Please set the -q option. See options below:\n%s", o.helpText().c_str()); return 1; }
  for (const char* k : {"-p", "-s", "-q", "-f"}) if (!o.s(k).empty() && !exists(o.s(k))) { printf("Could not find requested file/folder: %s\n", o.s(k).c_str()); return 1; }
  if (o.i("--num-threads") <= 0) bad("Number of threads must be positive.");
  if (o.i("-k") <= 0) bad("k-mer size must be positive.");
  if (o.i("--num-min-matches") <= 0) bad("Minimum number of matches must be positive.");
  if (o.i("--min-store-length") < 0) bad("The minimum read length stored must be >=0.");
  if (o.d("--repeat-idf-scale") < 1.0) bad("The minimum repeat idf scale must be >=1.0.");
  if (o.d("--max-shift") < -1.0) bad("The minimum shift must be greater than -1.");
  if (o.d("--threshold") < 0.0 || o.d("--threshold") > 1.0) bad("The second stage filter threshold must be 0<=threshold<=1.0.");
  if (o.i("--supress-noise") < 0 || o.i("--supress-noise") > 2) bad("The --supress-noise parameter must be in [0,2].");
  g_headers.full = o.b("--store-full-id");
  setenv("MHAP_HOST_THREADS", o.s("--num-threads").c_str(), 0);
  fprintf(stderr, "Running with these settings:\n%s", o.dump().c_str());

  mhap_params P; mhap_default_params(&P);
  P.kmer_size = o.i("-k"); P.num_hashes = o.i("--num-hashes"); P.ordered_kmer_size = o.i("--ordered-kmer-size");
  P.ordered_sketch_size = o.i("--ordered-sketch-size"); P.num_min_matches = o.i("--num-min-matches");
  P.min_store_length = o.i("--min-store-length"); P.min_olap_length = o.i("--min-olap-length"); P.device = o.i("--device");
  P.threshold = o.d("--threshold"); P.max_shift = o.d("--max-shift"); P.repeat_weight = o.d("--repeat-weight");
  // ranks: --devices a,b,c  |  --gpus N from --device on  |  one handle
  std::vector<int32_t> devs;
  if (!o.s("--devices").empty()) {
    const std::string dl = o.s("--devices");
    for (size_t i = 0; i < dl.size();) { size_t j = dl.find(',', i); if (j == std::string::npos) j = dl.size(); if (j > i) devs.push_back(atoi(dl.substr(i, j - i).c_str())); i = j + 1; }
  } else {
    if (o.i("--gpus") < 1) bad("The number of GPUs must be positive.");
    for (int r = 0; r < o.i("--gpus"); r++) devs.push_back(o.i("--device") + r);
  }
  if (devs.empty()) bad("No device given.");
  const bool precompute = !o.s("-p").empty();
  const bool realign = o.b("--realign") && !precompute;
  if (o.b("--realign-paf") && !o.b("--realign")) bad("--realign-paf prints the alignments of --realign: give --realign too.");
  const bool correct = o.isset("--correct");
  if (correct) {   // refused before a handle exists
    if (!o.b("--realign")) bad("--correct votes with the alignments of --realign: give --realign too.");
    if (!o.s("-q").empty()) bad("--correct corrects the reads of -s from their overlaps with each other: it takes no -q.");
    if (ends_with(o.s("-s"), ".dat")) bad("--correct needs the reads' bases: give FASTA files, not .dat sketches.");
    if (devs.size() > 1) bad("--correct runs on one GPU: give one device (--gpus 1).");
    if (o.s("--correct").empty()) bad("--correct needs the name of the FASTA file to write.");
    if (o.i("--correct-min-coverage") < 1) bad("The correction's minimum coverage must be >=1.");
  }
  const bool best = o.isset("--best-overlaps") && o.i("--best-overlaps") != 0;
  for (const char* n : {"--best-min-span", "--best-table"})   // refused before a handle exists
    if (o.isset(n) && !best) bad((std::string(n) + " belongs to --best-overlaps: give --best-overlaps too.").c_str());
  if (best) {   // refused before a handle exists
    if (o.i("--best-overlaps") < 0) bad("The value of --best-overlaps must be >=0.");
    if (!o.b("--realign")) bad("--best-overlaps selects among the alignments of --realign: give --realign too.");
    if (!o.s("-q").empty()) bad("--best-overlaps selects for the reads of -s from their overlaps with each other: it takes no -q.");
    if (ends_with(o.s("-s"), ".dat")) bad("--best-overlaps needs the overlaps realigned on the reads' bases: give FASTA files, not .dat sketches.");
    if (devs.size() > 1) bad("--best-overlaps runs on one GPU: give one device (--gpus 1).");
    if (o.i("--best-min-span") < 0) bad("The value of --best-min-span must be >=0.");
    if (o.isset("--best-table") && o.s("--best-table").empty()) bad("--best-table needs the name of the file to write.");
  }
  const bool gfa = o.isset("--gfa");
  if (o.isset("--gfa-unitigs")) {   // refused before a handle exists
    if (!gfa) bad("--gfa-unitigs compacts the graph of --gfa: give --gfa too.");
    if (o.s("--gfa-unitigs").empty()) bad("--gfa-unitigs needs the name of the GFA file to write.");
  }
  for (const char* n : {"--gfa-clean", "--gfa-tip-reads", "--gfa-bubble-bases", "--gfa-clean-rounds"})   // refused before a handle exists
    if (o.isset(n) && !gfa) bad((std::string(n) + " cleans the graph of --gfa: give --gfa too.").c_str());
  if (o.i("--gfa-tip-reads") < 0 || o.i("--gfa-bubble-bases") < 0 || o.i("--gfa-clean-rounds") < 1)
    bad("The values of --gfa-tip-reads and --gfa-bubble-bases must be >=0 and that of --gfa-clean-rounds >=1.");
  for (const char* n : {"--gfa-consensus", "--gfa-consensus-fasta", "--gfa-consensus-min-cov"})   // refused before a handle exists
    if (o.isset(n) && !o.isset("--gfa-unitigs")) bad((std::string(n) + " works on the unitigs of --gfa-unitigs: give --gfa-unitigs too.").c_str());
  for (const char* n : {"--gfa-consensus-fasta", "--gfa-consensus-min-cov"})
    if (o.isset(n) && !o.b("--gfa-consensus")) bad((std::string(n) + " belongs to --gfa-consensus: give --gfa-consensus too.").c_str());
  if (o.isset("--gfa-consensus-fasta") && o.s("--gfa-consensus-fasta").empty()) bad("--gfa-consensus-fasta needs the name of the FASTA file to write.");
  if (o.i("--gfa-consensus-min-cov") < 1) bad("The value of --gfa-consensus-min-cov must be >=1.");
  if (gfa) {   // refused before a handle exists
    if (!o.b("--realign")) bad("--gfa builds the graph from the alignments of --realign: give --realign too.");
    if (!o.s("-q").empty()) bad("--gfa lays out the reads of -s from their overlaps with each other: it takes no -q.");
    if (ends_with(o.s("-s"), ".dat")) bad("--gfa needs the overlaps realigned on the reads' bases: give FASTA files, not .dat sketches.");
    if (devs.size() > 1) bad("--gfa runs on one GPU: give one device (--gpus 1).");
    if (o.s("--gfa").empty()) bad("--gfa needs the name of the GFA file to write.");
    if (o.i("--gfa-max-hang") < 0 || o.i("--gfa-min-overlap") < 0 || o.i("--gfa-fuzz") < 0) bad("The values of --gfa-max-hang, --gfa-min-overlap and --gfa-fuzz must be >=0.");
  }
  const bool trim = o.b("--trim");
  const bool repeat = o.b("--repeat-filter");
  for (const char* n : {"--trim-min-cov", "--trim-end-clip", "--trim-min-span", "--trim-fasta", "--trim-table"})   // refused before a handle exists
    if (o.isset(n) && !trim) bad((std::string(n) + " belongs to --trim: give --trim too.").c_str());
  if (o.isset("--trim-penalty") && !trim && !repeat) bad("--trim-penalty belongs to --trim: give --trim too.");
  for (const char* n : {"--repeat-factor", "--repeat-max-cov", "--repeat-min-run", "--repeat-min-unique", "--repeat-table"})
    if (o.isset(n) && !repeat) bad((std::string(n) + " belongs to --repeat-filter: give --repeat-filter too.").c_str());
  if (repeat) {   // refused wherever --trim is, before a handle exists
    if (!o.b("--realign")) bad("--repeat-filter piles up the alignments of --realign: give --realign too.");
    if (!o.s("-q").empty()) bad("--repeat-filter marks the reads of -s from their overlaps with each other: it takes no -q.");
    if (ends_with(o.s("-s"), ".dat")) bad("--repeat-filter needs the overlaps realigned on the reads' bases: give FASTA files, not .dat sketches.");
    if (devs.size() > 1) bad("--repeat-filter runs on one GPU: give one device (--gpus 1).");
    if (o.i("--repeat-factor") < 100 || o.i("--repeat-max-cov") < 0 || o.i("--repeat-min-run") < 1 || o.i("--repeat-min-unique") < 0 || o.i("--trim-penalty") < 0)
      bad("The value of --repeat-factor must be >=100, that of --repeat-min-run >=1 and those of --repeat-max-cov, --repeat-min-unique and --trim-penalty >=0.");
    if (o.isset("--repeat-table") && o.s("--repeat-table").empty()) bad("--repeat-table needs the name of the file to write.");
  }
  if (trim) {   // refused before a handle exists
    if (!o.b("--realign")) bad("--trim piles up the alignments of --realign: give --realign too.");
    if (!o.s("-q").empty()) bad("--trim trims the reads of -s from their overlaps with each other: it takes no -q.");
    if (ends_with(o.s("-s"), ".dat")) bad("--trim needs the overlaps realigned on the reads' bases: give FASTA files, not .dat sketches.");
    if (devs.size() > 1) bad("--trim runs on one GPU: give one device (--gpus 1).");
    if (o.i("--trim-min-cov") < 1 || o.i("--trim-end-clip") < 0 || o.i("--trim-min-span") < 0 || o.i("--trim-penalty") < 0)
      bad("The value of --trim-min-cov must be >=1 and those of --trim-end-clip, --trim-min-span and --trim-penalty >=0.");
    for (const char* n : {"--trim-fasta", "--trim-table"})
      if (o.isset(n) && o.s(n).empty()) bad((std::string(n) + " needs the name of the file to write.").c_str());
  }
  if (realign) {   // refused before a handle exists
    if (o.i("--realign-band") < 0) bad("The realignment band must be >=0.");
    if (devs.size() > 1) bad("--realign runs on one GPU: give one device (--gpus 1).");
    bool dat = ends_with(o.s("-s"), ".dat");
    if (!o.s("-q").empty()) for (const std::string& cf : list_files(o.s("-q"))) dat = dat || ends_with(cf, ".dat");
    if (dat) bad("--realign needs the reads' bases: give FASTA files, not .dat sketches.");
  }
  if (precompute && devs.size() > 1) { fprintf(stderr, "Usage 2 (-p) writes its .dat files from one GPU: using device %d only.\n", devs[0]); devs.resize(1); }
  Engine E; E.n = (int)devs.size();
  char err[512] = {0};
  const double t_create = now();
  // mhap_create is mostly the HIP runtime coming up (~0.25 s): it runs on its own thread while this one reads and parses the
  // FASTA file the index is built from
  int rc_create = MHAP_OK;
  std::thread creator([&]() {
    if (devs.size() == 1) { P.device = devs[0]; rc_create = mhap_create(&P, &E.h, err, sizeof err); }
    else rc_create = mhap_group_create(&P, devs.data(), (int32_t)devs.size(), &E.g, err, sizeof err);
  });
  if (!precompute && !is_dir(o.s("-s")) && !ends_with(o.s("-s"), ".dat")) {
    char perr[512] = {0};
    if (mhap_fasta_scan_open(o.s("-s").c_str(), 0, &g_preload.scan, perr, sizeof perr) == MHAP_OK) g_preload.path = o.s("-s");
    else g_preload.scan = nullptr;
    // (a failure is reported by the regular scan below)
  }
  creator.join();
  if (rc_create != MHAP_OK) die(err);
  if (getenv("MHAP_HOST_PROF")) fprintf(stderr, "[cli] mhap_create + first FASTA scan %.3f s\n", now() - t_create);
  if (E.g) fprintf(stderr, "Using %d GPU ranks (reads dealt round-robin; every rank indexes its share).\n", E.n);

  const double t_total = now();
  if (!o.s("-f").empty()) {
    const double t = now();
    fprintf(stderr, "Reading in filter file %s.\n", o.s("-f").c_str());
    load_filter(E, o);
    fprintf(stderr, "Time (s) to read filter file: %g\n", now() - t);
  }

  if (precompute) {   // Usage 2: precompute `.dat` (MhapMain.java:384-451)
    mhap_handle* h = E.h;
    fprintf(stderr, "Processing FASTA files for binary compression...\n");
    if (!is_dir(o.s("-q"))) die("Target directory doesn't exit.");
    for (const std::string& pf : list_files(o.s("-p"))) {
      const double t = now();
      chk(h, mhap_index_clear(h));
      int64_t strands = 0;
      add_file_to_index(E, pf, 0, o, &strands);
      std::string name = pf.substr(pf.find_last_of('/') + 1);
      size_t dot = name.find_last_of('.'); if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
      const std::string out = o.s("-q") + "/" + name + ".dat";
      write_dat(h, out, P.num_hashes, P.ordered_sketch_size, P.ordered_kmer_size);
      fprintf(stderr, "Processed %lld sequences (fwd and rev).\n", (long long)strands);
      fprintf(stderr, "Read, hashed, and stored file %s to %s.\n", pf.c_str(), out.c_str());
      fprintf(stderr, "Time (s): %g\n", now() - t);
    }
    fprintf(stderr, "Total time (s): %g\n", now() - t_total);
    E.destroy();
    return 0;
  }

  fprintf(stderr, "Processing files for storage in reverse index...\n");
  const double t_proc = now();
  int64_t strands = 0;
  int64_t seq_processed = add_file_to_index(E, o.s("-s"), 0, o, &strands);
  fprintf(stderr, "Stored %lld sequences in the index.\n", (long long)strands);
  fprintf(stderr, "Processed %lld unique sequences (fwd and rev).\n", (long long)strands);
  fprintf(stderr, "Time (s) to read and hash from file: %g\n", now() - t_proc);

  Sink sink{stdout};
  Realign RA;
  mhap_graph_params gp;
  mhap_graph_default_params(&gp);
  gp.max_hang = o.i("--gfa-max-hang"); gp.min_ovlp = o.i("--gfa-min-overlap"); gp.fuzz = o.i("--gfa-fuzz");
  mhap_trim_params tp;
  mhap_trim_default_params(&tp);
  if (realign) {
    RA.h = E.h; RA.band = o.i("--realign-band"); RA.min_identity = o.d("--realign-min-identity"); RA.paf = o.b("--realign-paf");
    for (const std::string& sf : list_files(o.s("-s"))) {   // (ids as the index assigned them: FastaData's running count)
      mhap_fasta fa;
      if (mhap_fasta_read(sf.c_str(), (int64_t)RA.ids.size(), &fa, err, sizeof err) != MHAP_OK) die(err);
      RA.add(fa);
      mhap_fasta_free(&fa);
    }
    sink.realign = &RA;
    if (correct) chk(E.h, mhap_correct_begin(E.h, RA.bases.data(), (int64_t)RA.bases.size(), RA.ids.data(), RA.offsets.data(), RA.lengths.data(),
                                             (int64_t)RA.ids.size(), &RA.correct));
    if (best) {
      mhap_select_params sp;
      mhap_select_default_params(&sp);
      sp.best_n = o.i("--best-overlaps"); sp.min_span = o.i("--best-min-span");
      chk(E.h, mhap_select_begin(E.h, RA.ids.data(), RA.lengths.data(), (int64_t)RA.ids.size(), &sp, &RA.select));
      RA.hold_select = correct;
    }
    if (trim) { tp.min_cov = o.i("--trim-min-cov"); tp.end_clip = o.i("--trim-end-clip"); tp.min_span = o.i("--trim-min-span"); }
    if (trim || repeat) RA.trim_penalty = o.i("--trim-penalty");
    if (repeat) {   // (with --trim too, the trimming begins once the repeat stage has freed its device arrays)
      mhap_repeat_params rp;
      mhap_repeat_default_params(&rp);
      rp.factor_pct = o.i("--repeat-factor"); rp.max_cov = o.i("--repeat-max-cov"); rp.min_run = o.i("--repeat-min-run"); rp.min_unique = o.i("--repeat-min-unique");
      chk(E.h, mhap_repeat_begin(E.h, RA.ids.data(), RA.lengths.data(), (int64_t)RA.ids.size(), &rp, &RA.repeat));
      RA.hold_plain = gfa && !trim;
    } else if (trim) chk(E.h, mhap_trim_begin(E.h, RA.ids.data(), RA.lengths.data(), (int64_t)RA.ids.size(), &tp, &RA.trim));
    if (gfa && trim) RA.keep_records = true;   // the graph begins after the trimming, on the trimmed reads: the records wait for it
    else if (gfa) {
      chk(E.h, mhap_graph_begin(E.h, RA.ids.data(), RA.lengths.data(), (int64_t)RA.ids.size(), &gp, &RA.graph));
      RA.keep_records = o.b("--gfa-consensus");
    }
  }
  const double t_score = now();
  if (o.s("-q").empty()) {
    const double t = now();
    E.find_self(sink_cb, &sink);
    sink_flush(sink);
    fprintf(stderr, "Time (s) to score and output to self: %g\n", now() - t);
  } else {
    double t = now();
    if (!o.b("--no-self")) {
      E.find_self(sink_cb, &sink);
      sink_flush(sink);
      fprintf(stderr, "Time (s) to score and output to self: %g\n", now() - t);
    }
    for (const std::string& cf : list_files(o.s("-q"))) {
      t = now();
      fprintf(stderr, "Opened fasta file %s.\n", cf.c_str());
      int64_t nq = 0;
      if (ends_with(cf, ".dat")) {   // precomputed query sketches: forward entries only (SequenceSketchStreamer.java:291-303)
        if (E.g) die("--gpus N takes FASTA input (precomputed .dat sketches are searched on one GPU)");
        mhap_handle* h = E.h;
        DatEntries d;
        read_dat(cf, seq_processed, P.num_hashes, P.ordered_sketch_size, true, d);
        if (g_headers.full) for (size_t i = 0; i < d.ids.size(); i++) g_headers.byid[d.ids[i]] = d.hdr[i];
        if (!d.ids.empty())
          chk(h, mhap_find_matches_sketches(h, d.ids.data(), d.seqlen.data(), d.mh.data(), d.ord.data(), d.osz.data(), d.olen.data(),
                                            (int64_t)d.ids.size(), sink_cb, &sink));
        sink_flush(sink);
        seq_processed += (int64_t)d.ids.size();
        fprintf(stderr, "Processed %lld to sequences.\n", (long long)d.ids.size());
        fprintf(stderr, "Time (s) to score, hash to-file, and output: %g\n", now() - t);
        continue;
      }
      mhap_fasta fa;
      if (mhap_fasta_read(cf.c_str(), seq_processed, &fa, err, sizeof err) != MHAP_OK) die(err);   // id offset = reads so far (MhapMain.java:527)
      if (g_headers.full) collect_headers(fa);
      if (realign) RA.add(fa);
      const mhap_stats s0 = E.stats();
      E.find_reads(fa, sink_cb, &sink);
      const mhap_stats s1 = E.stats();
      nq = s1.queries_searched - s0.queries_searched;   // forward sketches produced = getNumberProcessed() (MhapMain.java:537)
      mhap_fasta_free(&fa);
      sink_flush(sink);
      seq_processed += nq;
      fprintf(stderr, "Processed %lld to sequences.\n", (long long)nq);
      fprintf(stderr, "Time (s) to score, hash to-file, and output: %g\n", now() - t);
    }
  }
  sink_flush(sink);
  fprintf(stderr, "Total scoring time (s): %g\n", now() - t_score);
  if (realign) fprintf(stderr, "Time (s) to realign: %g (%lld overlaps kept, %lld dropped: no alignment or identity below %g)\n", RA.seconds, (long long)RA.kept, (long long)RA.dropped, RA.min_identity);
  if (RA.select) {   // every read's threshold after the last batch; with --correct the held records that keep a view are realigned again, with paths, and vote
    const double ts = now();
    const int64_t nr = (int64_t)RA.ids.size(), nh = (int64_t)RA.held_out.size();
    int64_t sc[MHAP_SELECT_COUNTS];
    chk(E.h, mhap_select_finish(RA.select, sc));
    if (o.isset("--best-table")) {
      std::vector<int32_t> srows((size_t)std::max<int64_t>(nr, 1) * 4);
      chk(E.h, mhap_select_copy(RA.select, srows.data()));
      FILE* f = fopen(o.s("--best-table").c_str(), "wb");
      if (!f) die("cannot write " + o.s("--best-table"));
      std::string text;
      for (int64_t r = 0; r < nr; r++)
        text += header_of(RA.ids[(size_t)r]) + " " + std::to_string(srows[4 * (size_t)r]) + " " + std::to_string(srows[4 * (size_t)r + 1]) + " " +
                std::to_string(srows[4 * (size_t)r + 2]) + "\n";
      fwrite(text.data(), 1, text.size(), f);
      if (fclose(f) != 0) die("cannot write " + o.s("--best-table"));
    }
    std::vector<uint8_t> views((size_t)std::max<int64_t>(nh, 1));
    if (RA.correct) chk(E.h, mhap_select_apply(RA.select, RA.held_out.data(), nh, views.data()));
    mhap_select_free(RA.select);
    RA.select = nullptr;
    RA.select_seconds += now() - ts;
    fprintf(stderr, "Best overlaps: %lld reads, %lld with a view, %lld cut; %lld of %lld views kept; %lld eligible overlaps\n", (long long)sc[0],
            (long long)sc[1], (long long)sc[2], (long long)sc[4], (long long)sc[3], (long long)sc[5]);
    fprintf(stderr, "Time (s) to select the best overlaps: %g\n", RA.select_seconds);
    if (RA.correct) {   // the aligner is deterministic: the records as they came give the alignments of the first pass again, now with their paths
      const double tc = now();
      std::vector<mhap_record> in, out, kept;
      std::vector<uint8_t> vb, kv;
      for (int64_t q = 0; q < nh; q++)
        if (views[(size_t)q]) { in.push_back(RA.held_in[(size_t)q]); vb.push_back(views[(size_t)q]); }
      std::vector<mhap_record>().swap(RA.held_in);
      std::vector<mhap_record>().swap(RA.held_out);
      const int64_t total = (int64_t)in.size(), step = 1 << 16;
      for (int64_t q0 = 0; q0 < total; q0 += step) {
        const int64_t n = std::min(step, total - q0);
        out.resize((size_t)n);
        RA.detail.resize((size_t)n * 3);
        mhap_align_paths* paths = nullptr;
        chk(E.h, mhap_realign_records_paths(E.h, RA.bases.data(), (int64_t)RA.bases.size(), RA.ids.data(), RA.offsets.data(), RA.lengths.data(),
                                            (int64_t)RA.ids.size(), in.data() + q0, n, RA.band, out.data(), RA.detail.data(), &paths));
        int64_t n_ops = 0;
        mhap_align_paths_info(paths, nullptr, &n_ops);
        RA.op_offsets.resize((size_t)n + 1); RA.ops.resize((size_t)std::max<int64_t>(n_ops, 1));
        mhap_align_paths_copy(paths, RA.op_offsets.data(), RA.ops.data());
        mhap_align_paths_free(paths);
        kept.clear(); kv.clear();
        RA.vote_offsets.assign(1, 0); RA.vote_ops.clear();
        for (int64_t i = 0; i < n; i++) {   // (the first pass's rule once more: nothing is dropped here unless the aligner differs)
          const mhap_record& r = out[(size_t)i];
          const bool none = r.score == 0.0 && r.a1 == 0 && r.a2 == 0 && r.b1 == 0 && r.b2 == 0;
          if (none || r.score < RA.min_identity) continue;
          kept.push_back(r); kv.push_back(vb[(size_t)(q0 + i)]);
          RA.vote_ops.insert(RA.vote_ops.end(), RA.ops.begin() + RA.op_offsets[(size_t)i], RA.ops.begin() + RA.op_offsets[(size_t)i + 1]);
          RA.vote_offsets.push_back((int64_t)RA.vote_ops.size());
        }
        mhap_align_paths* kept_paths = nullptr;
        if (mhap_align_paths_from_runs(RA.vote_offsets.data(), (int64_t)kept.size(), RA.vote_ops.data(), &kept_paths) != MHAP_OK) die("the paths of the selected overlaps");
        const int rc = mhap_correct_add_views(RA.correct, kept.data(), (int64_t)kept.size(), kept_paths, kv.empty() ? views.data() : kv.data());
        mhap_align_paths_free(kept_paths);
        chk(E.h, rc);
      }
      RA.correct_seconds += now() - tc;
    }
  }
  if (RA.correct) {   // the call for every read, after the last batch has voted; the FASTA file is all it writes
    const double tc = now();
    const int64_t nr = (int64_t)RA.ids.size();
    std::vector<int64_t> off((size_t)nr + 1);
    std::vector<int32_t> st((size_t)std::max<int64_t>(nr, 1) * 6);
    int64_t skipped = 0;
    chk(E.h, mhap_correct_finish(RA.correct, o.i("--correct-min-coverage"), off.data(), st.data(), &skipped));
    std::vector<uint8_t> bytes((size_t)std::max<int64_t>(off[(size_t)nr], 1));
    chk(E.h, mhap_correct_copy(RA.correct, bytes.data()));
    mhap_correct_free(RA.correct);
    RA.correct = nullptr;
    FILE* f = fopen(o.s("--correct").c_str(), "wb");
    if (!f) die("cannot write " + o.s("--correct"));
    long long tot[6] = {0, 0, 0, 0, 0, 0};
    std::string text;
    for (int64_t r = 0; r < nr; r++) {
      const int32_t* c = st.data() + 6 * r;
      for (int u = 0; u < 6; u++) tot[u] += c[u];
      text += ">" + header_of(RA.ids[(size_t)r]) + " len=" + std::to_string(c[1]) + " sub=" + std::to_string(c[2]) + " del=" + std::to_string(c[3]) +
              " ins=" + std::to_string(c[4]) + " low=" + std::to_string(c[5]) + "\n";
      text.append((const char*)bytes.data() + off[(size_t)r], (size_t)(off[(size_t)r + 1] - off[(size_t)r]));
      text.push_back('\n');
      if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
    }
    fwrite(text.data(), 1, text.size(), f);
    if (fclose(f) != 0) die("cannot write " + o.s("--correct"));
    RA.correct_seconds += now() - tc;
    fprintf(stderr, "Corrected %lld reads: %lld bases in, %lld out; %lld substitutions, %lld deletions, %lld insertions, %lld positions of low coverage; skipped_views = %lld\n",
            (long long)nr, tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], (long long)skipped);
    fprintf(stderr, "Time (s) to vote and correct: %g\n", RA.correct_seconds);
  }
  if (RA.repeat) {   // the intervals of every read and the judgement of every held record, after the last batch; trimming and graph take the survivors
    const double tr = now();
    const int64_t nr = (int64_t)RA.ids.size(), nk = (int64_t)RA.held_refined.size();
    int64_t rcn[MHAP_REPEAT_COUNTS];
    chk(E.h, mhap_repeat_finish(RA.repeat, rcn));
    if (o.isset("--repeat-table")) {
      std::vector<int32_t> rrows((size_t)std::max<int64_t>(nr, 1) * 4), riv((size_t)std::max<int64_t>(rcn[3], 1) * 2);
      std::vector<uint8_t> rflags((size_t)std::max<int64_t>(nr, 1));
      std::vector<int64_t> roff((size_t)nr + 1);
      chk(E.h, mhap_repeat_copy(RA.repeat, rrows.data(), rflags.data(), roff.data(), riv.data()));
      FILE* f = fopen(o.s("--repeat-table").c_str(), "wb");
      if (!f) die("cannot write " + o.s("--repeat-table"));
      for (int64_t r = 0; r < nr; r++)
        for (int64_t i = roff[(size_t)r]; i < roff[(size_t)r + 1]; i++)
          fprintf(f, "%lld\t%d\t%d\n", (long long)RA.ids[(size_t)r], riv[(size_t)i * 2], riv[(size_t)i * 2 + 1]);
      if (fclose(f) != 0) die("cannot write " + o.s("--repeat-table"));
    }
    std::vector<uint8_t> keep((size_t)std::max<int64_t>(nk, 1));
    std::vector<int32_t> unique((size_t)std::max<int64_t>(nk, 1) * 2);
    chk(E.h, mhap_repeat_apply(RA.repeat, RA.held_refined.data(), nk, keep.data(), unique.data()));
    mhap_repeat_free(RA.repeat);   // (its device arrays go before the trimming allocates its own)
    RA.repeat = nullptr;
    std::vector<mhap_record>& survivors = RA.hold_plain ? RA.held_plain : RA.held_refined;   // the graph: as realigned; the trimming: refined
    size_t w = 0;
    for (int64_t q = 0; q < nk; q++) if (keep[(size_t)q]) survivors[w++] = survivors[(size_t)q];
    survivors.resize(w);
    RA.repeat_seconds += now() - tr;
    fprintf(stderr, "Repeats: %lld reads, %lld with a repeat, %lld repeat throughout; %lld intervals, %lld of %lld bases; %lld eligible overlaps, depth %lld, threshold %lld\n",
            (long long)rcn[0], (long long)rcn[1], (long long)rcn[2], (long long)rcn[3], (long long)rcn[4], (long long)rcn[5], (long long)rcn[6],
            (long long)rcn[7], (long long)rcn[8]);
    fprintf(stderr, "Time (s) to mark repeats: %g (%lld of %lld overlaps set aside)\n", RA.repeat_seconds, (long long)(nk - (int64_t)w), (long long)nk);
    if (trim) {
      const double tt = now();
      chk(E.h, mhap_trim_begin(E.h, RA.ids.data(), RA.lengths.data(), nr, &tp, &RA.trim));
      chk(E.h, mhap_trim_add(RA.trim, survivors.data(), (int64_t)w));
      RA.trim_seconds += now() - tt;
    } else if (RA.graph) {
      const double tg = now();
      chk(E.h, mhap_graph_add(RA.graph, survivors.data(), (int64_t)w));
      RA.graph_seconds += now() - tg;
    }
    if (RA.keep_records) RA.kept_records.swap(survivors);
    std::vector<mhap_record>().swap(RA.held_refined);
    std::vector<mhap_record>().swap(RA.held_plain);
  }
  if (RA.trim) {   // every read's clear range, after the last batch has been piled up; with --gfa the graph begins here, on the trimmed reads
    const double tt = now();
    const int64_t nr = (int64_t)RA.ids.size();
    int64_t tc[MHAP_TRIM_COUNTS];
    chk(E.h, mhap_trim_finish(RA.trim, tc));
    std::vector<int32_t> trows((size_t)std::max<int64_t>(nr, 1) * 4);
    std::vector<uint8_t> tflags((size_t)std::max<int64_t>(nr, 1));
    chk(E.h, mhap_trim_copy(RA.trim, trows.data(), tflags.data()));
    if (o.isset("--trim-fasta")) {
      FILE* f = fopen(o.s("--trim-fasta").c_str(), "wb");
      if (!f) die("cannot write " + o.s("--trim-fasta"));
      std::string text;
      for (int64_t r = 0; r < nr; r++) {
        if (tflags[(size_t)r] & MHAP_TRIM_DELETED) continue;
        const int32_t* c = trows.data() + 4 * r;
        text += ">" + header_of(RA.ids[(size_t)r]) + " len=" + std::to_string(c[1] - c[0]) + " begin=" + std::to_string(c[0]) + " end=" + std::to_string(c[1]) +
                " runs=" + std::to_string(c[2]) + "\n";
        text.append((const char*)RA.bases.data() + RA.offsets[(size_t)r] + c[0], (size_t)(c[1] - c[0]));
        text.push_back('\n');
        if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
      }
      fwrite(text.data(), 1, text.size(), f);
      if (fclose(f) != 0) die("cannot write " + o.s("--trim-fasta"));
    }
    if (o.isset("--trim-table")) {
      FILE* f = fopen(o.s("--trim-table").c_str(), "wb");
      if (!f) die("cannot write " + o.s("--trim-table"));
      for (int64_t r = 0; r < nr; r++) {
        const int32_t* c = trows.data() + 4 * r;
        fprintf(f, "%lld\t%d\t%d\t%d\t%d\t%d\t%d\n", (long long)RA.ids[(size_t)r], RA.lengths[(size_t)r], c[0], c[1], c[2], c[3], (int)tflags[(size_t)r]);
      }
      if (fclose(f) != 0) die("cannot write " + o.s("--trim-table"));
    }
    if (gfa) {   // the records rewritten and compacted, the table of the surviving reads, and the graph over both
      const int64_t nk = (int64_t)RA.kept_records.size();
      std::vector<mhap_record> applied((size_t)std::max<int64_t>(nk, 1));
      std::vector<uint8_t> keep((size_t)std::max<int64_t>(nk, 1));
      chk(E.h, mhap_trim_apply(RA.trim, RA.kept_records.data(), nk, applied.data(), keep.data()));
      size_t w = 0;
      for (int64_t q = 0; q < nk; q++) if (keep[(size_t)q]) applied[w++] = applied[(size_t)q];
      applied.resize(w);
      RA.kept_records.swap(applied);
      size_t live = 0;
      for (int64_t r = 0; r < nr; r++) {   // (the bases stay where they are: a trimmed read begins `begin` bytes later)
        if (tflags[(size_t)r] & MHAP_TRIM_DELETED) continue;
        RA.ids[live] = RA.ids[(size_t)r];
        RA.offsets[live] = RA.offsets[(size_t)r] + trows[(size_t)r * 4];
        RA.lengths[live++] = trows[(size_t)r * 4 + 1] - trows[(size_t)r * 4];
      }
      RA.ids.resize(live); RA.offsets.resize(live); RA.lengths.resize(live);
      const double tg = now();
      chk(E.h, mhap_graph_begin(E.h, RA.ids.data(), RA.lengths.data(), (int64_t)live, &gp, &RA.graph));
      chk(E.h, mhap_graph_add(RA.graph, RA.kept_records.data(), (int64_t)RA.kept_records.size()));
      RA.graph_seconds += now() - tg;
      if (!o.b("--gfa-consensus")) std::vector<mhap_record>().swap(RA.kept_records);
    }
    mhap_trim_free(RA.trim);
    RA.trim = nullptr;
    RA.trim_seconds += now() - tt;
    fprintf(stderr, "Trim: %lld reads, %lld deleted, %lld cut at 5', %lld cut at 3', %lld gapped; %lld of %lld bases kept, %lld eligible overlaps\n",
            (long long)tc[0], (long long)tc[1], (long long)tc[2], (long long)tc[3], (long long)tc[4], (long long)tc[6], (long long)tc[5], (long long)tc[7]);
    fprintf(stderr, "Time (s) to pile up and trim: %g\n", RA.trim_seconds);
  }
  if (RA.graph) {   // the list and its reduction, after the last batch has been classed; the GFA file is all it writes
    const double tg = now();
    const int64_t nr = (int64_t)RA.ids.size();
    int64_t gc[MHAP_GRAPH_COUNTS];
    chk(E.h, mhap_graph_finish(RA.graph, gc));
    const int64_t na = gc[8];
    std::vector<int32_t> rows((size_t)std::max<int64_t>(na, 1) * 7);
    std::vector<uint8_t> contained((size_t)std::max<int64_t>(nr, 1));
    chk(E.h, mhap_graph_copy_arcs(RA.graph, rows.data()));
    chk(E.h, mhap_graph_copy_read_flags(RA.graph, contained.data()));
    int64_t uc[MHAP_UNITIG_COUNTS], cc[MHAP_CLEAN_COUNTS], kc[MHAP_CONSENSUS_COUNTS];
    const bool unitigs = o.isset("--gfa-unitigs"), clean = o.b("--gfa-clean"), consensus = o.b("--gfa-consensus");
    std::vector<uint8_t> removed((size_t)std::max<int64_t>(na, 1), 0);
    if (clean) {   // tips and bubbles go before either file is written: a dropped read counts as a contained one does, a removed arc is not final
      mhap_clean_params cp;
      cp.tip_reads = o.i("--gfa-tip-reads"); cp.bubble_bases = o.i("--gfa-bubble-bases"); cp.max_rounds = o.i("--gfa-clean-rounds");
      std::vector<uint8_t> dropped((size_t)std::max<int64_t>(nr, 1));
      chk(E.h, mhap_graph_clean(RA.graph, &cp, cc));
      chk(E.h, mhap_graph_copy_dropped(RA.graph, dropped.data()));
      chk(E.h, mhap_graph_copy_removed(RA.graph, removed.data()));
      for (int64_t r = 0; r < nr; r++) if (dropped[(size_t)r]) contained[(size_t)r] = 1;
    }
    if (unitigs) {   // the chains of the final arcs and their bases, while the graph is on the device; the second file is all it writes
      if (clean) chk(E.h, mhap_graph_unitigs_counts(RA.graph, uc));   // (the clean has built the unitigs of the cleaned graph)
      else chk(E.h, mhap_graph_unitigs(RA.graph, uc));
      const size_t nu = (size_t)uc[0], nm = (size_t)uc[2], nl = (size_t)uc[4];
      std::vector<int64_t> ustart(nu + 1), ulen(nu + 1), moff(nm + 1);
      std::vector<uint8_t> circ(nu + 1), seq((size_t)uc[6] + 1);
      std::vector<int32_t> mv(nm + 1), msp(nm + 1), links(6 * nl + 6);
      chk(E.h, mhap_graph_copy_unitigs(RA.graph, ustart.data(), ulen.data(), circ.data()));
      chk(E.h, mhap_graph_copy_layout(RA.graph, mv.data(), moff.data(), msp.data()));
      chk(E.h, mhap_graph_copy_links(RA.graph, links.data()));
      std::vector<int64_t> cons_off(nu + 1, 0), cons_map;   // --gfa-consensus: unitig k's bytes in seq, the position map of all unitigs
      if (!consensus) chk(E.h, mhap_graph_spell(RA.graph, RA.bases.data(), (int64_t)RA.bases.size(), RA.offsets.data(), seq.data()));
      else {   // the kept records, fed now that the unitigs are served; the consensus takes the place of the spelling
        mhap_consensus_params kp;
        mhap_consensus_default_params(&kp);
        kp.min_cov = o.i("--gfa-consensus-min-cov");
        mhap_consensus_session* cs = nullptr;
        chk(E.h, mhap_consensus_begin(RA.graph, (const uint8_t*)RA.bases.data(), (int64_t)RA.bases.size(), RA.offsets.data(), &kp, &cs));
        chk(E.h, mhap_consensus_add(cs, RA.kept_records.data(), (int64_t)RA.kept_records.size()));
        chk(E.h, mhap_consensus_run(cs, kc));
        int64_t n_draft = 0, n_out = 0;
        chk(E.h, mhap_consensus_info(cs, nullptr, nullptr, &n_draft, &n_out));
        std::vector<int64_t> stats(6 * nu + 6);
        seq.assign((size_t)n_out + 1, 0);
        cons_map.assign((size_t)n_draft + 1, 0);
        chk(E.h, mhap_consensus_copy(cs, seq.data(), cons_off.data(), stats.data()));
        chk(E.h, mhap_consensus_copy_map(cs, cons_map.data()));
        mhap_consensus_free(cs);
        std::vector<mhap_record>().swap(RA.kept_records);
      }
      FILE* f = fopen(o.s("--gfa-unitigs").c_str(), "wb");
      if (!f) die("cannot write " + o.s("--gfa-unitigs"));
      std::string text = "H\tVN:Z:1.0\n";
      char name[32], line[128];
      size_t at = 0, draft_at = 0;   // unitig k's sequence in seq, its first position in the map
      for (size_t k = 0; k < nu; k++) {
        snprintf(name, sizeof name, "utg%06lld%c", (long long)k + 1, circ[k] ? 'c' : 'l');
        const size_t slen = consensus ? (size_t)(cons_off[k + 1] - cons_off[k]) : (size_t)ulen[k];
        text += std::string("S\t") + name + "\t";
        text.append((const char*)seq.data() + at, slen);
        at += slen;
        text += "\tLN:i:" + std::to_string(slen) + "\tnr:i:" + std::to_string(ustart[k + 1] - ustart[k]) + "\n";
        for (int64_t m = ustart[k]; m < ustart[k + 1]; m++) {
          const std::string sp = std::to_string(msp[(size_t)m]);
          const int64_t off = consensus ? cons_map[draft_at + (size_t)moff[(size_t)m]] : moff[(size_t)m];
          text += std::string("a\t") + name + "\t" + std::to_string(off) + "\t" + std::to_string(RA.ids[(size_t)(mv[(size_t)m] >> 1)]) + ":1-" + sp +
                  "\t" + ((mv[(size_t)m] & 1) ? "-" : "+") + "\t" + sp + "\n";
        }
        draft_at += (size_t)ulen[k];
        if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
      }
      for (size_t i = 0; i < nl; i++) {
        const int len = mhap_format_gfa_unitig_link(links.data() + 6 * i, line, sizeof line);
        if (len < 0 || (size_t)len >= sizeof line) die("mhap_format_gfa_unitig_link failed");
        text.append(line, (size_t)len);
        text.push_back('\n');
        if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
      }
      fwrite(text.data(), 1, text.size(), f);
      if (fclose(f) != 0) die("cannot write " + o.s("--gfa-unitigs"));
      if (consensus && o.isset("--gfa-consensus-fasta")) {
        FILE* ff = fopen(o.s("--gfa-consensus-fasta").c_str(), "wb");
        if (!ff) die("cannot write " + o.s("--gfa-consensus-fasta"));
        for (size_t k = 0; k < nu; k++) {
          fprintf(ff, ">utg%06lld%c\n", (long long)k + 1, circ[k] ? 'c' : 'l');
          fwrite(seq.data() + cons_off[k], 1, (size_t)(cons_off[k + 1] - cons_off[k]), ff);
          fputc('\n', ff);
        }
        if (fclose(ff) != 0) die("cannot write " + o.s("--gfa-consensus-fasta"));
      }
    }
    mhap_graph_free(RA.graph);
    RA.graph = nullptr;
    FILE* f = fopen(o.s("--gfa").c_str(), "wb");
    if (!f) die("cannot write " + o.s("--gfa"));
    std::string text = "H\tVN:Z:1.0\n";
    char line[128];
    for (int64_t r = 0; r < nr; r++) {
      if (contained[(size_t)r]) continue;
      text += "S\t" + std::to_string(RA.ids[(size_t)r]) + "\t*\tLN:i:" + std::to_string(RA.lengths[(size_t)r]) + "\n";
      if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
    }
    for (int64_t i = 0; i < na; i++) {
      if (!rows[(size_t)i * 7 + 6] || removed[(size_t)i]) continue;
      const int len = mhap_format_gfa_link(rows.data() + 7 * i, RA.ids.data(), line, sizeof line);
      if (len < 0 || (size_t)len >= sizeof line) die("mhap_format_gfa_link failed");
      text.append(line, (size_t)len);
      text.push_back('\n');
      if (text.size() > (8u << 20)) { fwrite(text.data(), 1, text.size(), f); text.clear(); }
    }
    fwrite(text.data(), 1, text.size(), f);
    if (fclose(f) != 0) die("cannot write " + o.s("--gfa"));
    RA.graph_seconds += now() - tg;
    fprintf(stderr, "String graph of %lld overlaps: %lld none, %lld internal, %lld contained (from), %lld contained (to), %lld short, %lld dovetail; "
                    "%lld contained reads, %lld arcs, %lld reduced, %lld final\n",
            (long long)gc[0], (long long)gc[1], (long long)gc[2], (long long)gc[3], (long long)gc[4], (long long)gc[5], (long long)gc[6],
            (long long)gc[7], (long long)gc[8], (long long)gc[9], (long long)gc[10]);
    if (clean)
      fprintf(stderr, "Cleaned in %lld rounds: %lld tips (%lld reads), %lld bubbles (%lld reads), %lld arcs removed\n", (long long)cc[0], (long long)cc[1],
              (long long)cc[2], (long long)cc[3], (long long)cc[4], (long long)cc[5]);
    if (unitigs)
      fprintf(stderr, "Unitigs: %lld unitigs (%lld circular) of %lld reads, %lld joined arcs, %lld links; longest %lld bases, %lld bases in all\n",
              (long long)uc[0], (long long)uc[1], (long long)uc[2], (long long)uc[3], (long long)uc[4], (long long)uc[5], (long long)uc[6]);
    if (consensus)
      fprintf(stderr, "Consensus: %lld members, %lld reads placed by an overlap, %lld unplaced; %lld aligned, %lld without alignment; %lld bases in, "
                      "%lld out: %lld substitutions, %lld deletions, %lld insertions, %lld low positions\n",
              (long long)kc[0], (long long)kc[1], (long long)kc[2], (long long)kc[3], (long long)kc[4], (long long)kc[5], (long long)kc[6],
              (long long)kc[7], (long long)kc[8], (long long)kc[9], (long long)kc[10]);
    fprintf(stderr, "Time (s) to class, build and reduce the graph: %g\n", RA.graph_seconds);
  }
  fprintf(stderr, "Total time (s): %g\n", now() - t_total);
  // outputFinalStat (MhapMain.java:572-590); the inverted-index counters have no brute-force analogue
  const mhap_stats st = E.stats();
  mhap_kernel_times kt; memset(&kt, 0, sizeof kt);
  for (int r = 0; r < E.n; r++) {   // kernel time summed over the ranks (they run concurrently)
    mhap_kernel_times k1; chk(E.rank(r), mhap_get_kernel_times(E.rank(r), &k1));
    for (int i = 0; i < MHAP_K_COUNT; i++) { kt.ms[i] += k1.ms[i]; kt.launches[i] += k1.launches[i]; }
  }
  fprintf(stderr, "MinHash search time (s): %g\n", (kt.ms[MHAP_K_CANDIDATE] + kt.ms[MHAP_K_INDEX_QUERY]) * 1e-3);
  fprintf(stderr, "Total matches found: %lld\n", (long long)st.matches_found);
  fprintf(stderr, "Average number of matches per lookup: %g\n", (double)st.matches_found / (double)std::max<int64_t>(1, st.queries_searched));
  fprintf(stderr, "Average %% of hashed sequences fully compared that are matches: %g\n", (double)st.matches_found / (double)std::max<int64_t>(1, st.candidates_compared) * 100.0);
  fprintf(stderr, "GPU kernel time (ms): hash %.3f, weights %.3f, minhash %.3f, ordered %.3f, index build %.3f, index query %.3f, candidates %.3f, overlap %.3f\n",
          kt.ms[MHAP_K_HASH], kt.ms[MHAP_K_WEIGHT], kt.ms[MHAP_K_MINHASH], kt.ms[MHAP_K_ORDERED], kt.ms[MHAP_K_INDEX_BUILD], kt.ms[MHAP_K_INDEX_QUERY],
          kt.ms[MHAP_K_CANDIDATE], kt.ms[MHAP_K_OVERLAP]);
  // everything is written: leave without tearing down gigabytes of device and host mappings one by one (the kernel does it faster)
  fflush(nullptr);
  _exit(0);
}
