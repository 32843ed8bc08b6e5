// mhap_cli.cpp — `mhap-hip`: native host driver over libmhaphip.so that keeps MHAP's command line, stdout
// record format, stderr timing lines and `.dat` sketch files (J/main/MhapMain.java:93-590,
// J/utils/ParseOptions.java, J/impl/SequenceSketchStreamer.java:278-395, J/impl/SequenceSketch.java:61-148).
// The reference host is Java; this image has no JVM, so the host side above the C ABI is C++ (see INTEGRATION.md
// for the JNI stub that lets the stock Java host call the same library).
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <thread>

#include "cli_pipeline.hpp"   // everything behind --realign (the realigned batch, the stages, their wiring), and the standard headers both files use

namespace {
using namespace cli;

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
  // when --gfa is, the cleaning's only when --gfa-clean is, the consensus' only when --gfa-consensus is, the trimming's only when --trim is, the repeat stage's only when --repeat-filter is, the variant stage's only when --variant-filter is, the selection's only when --best-overlaps is: without them every line the driver writes is what it was before them)
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
      if (n.compare(0, 9, "--variant") == 0 && !b("--variant-filter")) continue;
      if (n.compare(0, 6, "--best") == 0 && !isset("--best-overlaps")) continue;
      if (n == "--hpc" && !b("--hpc")) continue;
      if ((n == "--correct-fastq" || n == "--gfa-consensus-fastq") && !isset(n)) continue;   // (and the quality flags only with a FASTQ file to write)
      if (n.compare(0, 9, "--quality") == 0 && !isset("--correct-fastq") && !isset("--gfa-consensus-fastq")) continue;
      if (n.compare(0, 7, "--weigh") == 0 && !b("--weigh-qualities")) continue;
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
  void add_scan(const mhap_fasta_scan* sc) const { check(g ? mhap_group_add_scan(g, sc) : mhap_index_add_scan(h, sc)); }
  void find_self(mhap_record_sink sink, void* user) const { check(g ? mhap_group_find_matches_self(g, sink, user) : mhap_find_matches_self(h, 0, -1, sink, user)); }
  void find_reads(const mhap_fasta& fa, mhap_record_sink sink, void* user) const {
    if (fa.n <= 0) return;
    check(g ? mhap_group_find_matches_reads(g, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n, sink, user)
            : mhap_find_matches_reads(h, fa.bases, fa.offsets, fa.lengths, fa.ids, fa.n, sink, user));
  }
  mhap_stats stats() const { mhap_stats st; check(g ? mhap_group_get_stats(g, &st) : mhap_get_stats(h, &st)); return st; }
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
// stdout: with --realign every batch goes through the pipeline first and what it keeps is printed, as 12 columns or as PAF
// with --hpc every batch is first carried from compressed to raw coordinates
struct Sink { Writer out{stdout}; Pipeline* pipeline = nullptr; HpcStage* hpc = nullptr; };
int sink_cb(const mhap_record* r, int64_t n, void* user) {
  Sink* s = (Sink*)user;
  const Batch* b = nullptr;
  if (s->hpc && n > 0 && s->hpc->expand(r, n) != MHAP_OK) return 1;
  if (s->pipeline && n > 0) {
    if (!(b = s->pipeline->batch(r, n))) return 1;
    r = b->out.data(); n = b->k;
  }
  char line[512];
  std::string pl;
  for (int64_t i = 0; i < n; i++) {
    if (b && s->pipeline->paf) {   // one PAF line per kept record; the names are columns 1 and 2 of the 12-column line
      const int64_t q = b->row[(size_t)i], o0 = b->op_offsets[(size_t)q], o1 = b->op_offsets[(size_t)q + 1];
      const std::string qn = header_of(r[i].from_id), tn = header_of(r[i].to_id);
      pl.resize(256 + qn.size() + tn.size() + 12 * (size_t)(o1 - o0));
      const int len = mhap_format_paf(&r[i], b->detail.data() + 3 * q, b->ops.data() + o0, o1 - o0, qn.c_str(), tn.c_str(), &pl[0], pl.size());
      if (len < 0 || (size_t)len >= pl.size()) { fprintf(stderr, "Exception in mhap-hip: mhap_format_paf failed\n"); return 1; }
      s->out.put(pl.data(), (size_t)len);
    } else {
      const int len = mhap_format_record(&r[i], line, sizeof line);
      const char* p = line;
      if (g_headers.full) {   // same formatter, headers swapped in for the two id columns
        int sp = 0; while (*p && sp < 2) { if (*p == ' ') sp++; p++; }
        s->out.put(header_of(r[i].from_id) + " " + header_of(r[i].to_id) + " ");
      }
      s->out.put(p, (size_t)(line + len - p));
    }
    s->out.put("\n", 1);
  }
  return 0;
}
void sink_flush(Sink& s) { s.out.flush(); fflush(stdout); }

// FrequencyCounts file -> (hash, fraction) arrays (J/sketch/FrequencyCounts.java:63-229)
void load_filter(const Engine& E, const Options& o) {
  const double t = now();
  fprintf(stderr, "Reading in filter file %s.\n", o.s("-f").c_str());
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
  fprintf(stderr, "Time (s) to read filter file: %g\n", now() - t);
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
  Writer w(path);
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
    w.put(out);
  }
  w.close();
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

void declare_options(Options& o) {
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
  o.add("--correct-fastq", "With --correct, also write the corrected reads to this FASTQ file, with one quality per base from the votes that decided it (Phred+33).", "");
  o.add("--quality-per-vote", "[int] With --correct-fastq or --gfa-consensus-fastq, tenths of a Phred unit per net vote, 1 to 1000.", "15");
  o.add("--weigh-qualities", "With --correct or --gfa-consensus on FASTQ reads: every vote weighs the base quality of the read it comes from, 1 below --weight-q-lo, 2 up to --weight-q-hi, 3 from there on.", "false", true);
  o.add("--weight-q-lo", "[int] With --weigh-qualities, the Phred value below which a base votes with weight 1, 0 to 93.", "7");
  o.add("--weight-q-hi", "[int] With --weigh-qualities, the Phred value from which a base votes with weight 3, --weight-q-lo to 93.", "20");
  o.add("--quality-cap", "[int] With --correct-fastq or --gfa-consensus-fastq, the highest quality written, 1 to 93.", "60");
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
  o.add("--gfa-consensus-fastq", "With --gfa-consensus, also write the consensus sequences to this FASTQ file, with one quality per base from the votes that decided it (Phred+33).", "");
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
  o.add("--variant-filter", "With --realign: mark the variant sites of every read of -s on the GPU from the pile-up votes of the realigned overlaps (positions where a second allele is well supported), and set aside the overlaps whose two reads disagree across them: the two haplotypes of a diploid sample, or the copies of a diverged repeat. They reach neither --repeat-filter nor --trim nor --gfa; the overlaps are realigned a second time for the judgement. The overlaps printed, --correct and --realign-paf stay on all overlaps. Self overlaps only (no -q), one GPU.", "false", true);
  o.add("--variant-min-depth", "[int] With --variant-filter, the depth, own base included, a position needs to be a site.", "8");
  o.add("--variant-min-minor", "[int] With --variant-filter, the votes the second allele of a site needs.", "3");
  o.add("--variant-min-pct", "[int] With --variant-filter, the share of the depth the second allele of a site needs, in percent.", "25");
  o.add("--variant-max-del-pct", "[int] With --variant-filter, the greatest share of deletions in the depth of a site, in percent.", "25");
  o.add("--variant-min-diff", "[int] With --variant-filter, the disagreeing site columns an overlap needs to be set aside.", "2");
  o.add("--variant-diff-pct", "[int] With --variant-filter, the share of disagreeing among the agreeing and disagreeing site columns an overlap needs to be set aside, in percent.", "50");
  o.add("--variant-table", "With --variant-filter, write one line per site to this file: read_id pos major minor n_major n_minor depth.", "");
  o.add("--best-overlaps", "[int] With --realign: select each read's N best overlaps on the GPU, by the matches counted on that read, ties at the last place included; with --correct only the selected views of an overlap vote. The overlaps printed, --realign-paf, --gfa and --trim stay on all overlaps. 0) off. Self overlaps only (no -q), one GPU.", "0");
  o.add("--best-min-span", "[int] With --best-overlaps, the shortest aligned interval on a read that counts as evidence for it.", "500");
  o.add("--best-table", "With --best-overlaps, write one line per read to this file: read_id entries kept threshold.", "");
  o.add("--hpc", "Search with homopolymer-compressed reads: every read of -s and -q is read whole, each run of equal bases is collapsed to one on the GPU, the compressed reads are sketched and searched, and every overlap found is carried back to the raw reads before it is printed or handed to --realign. Columns 5 to 12 are raw coordinates and raw lengths; columns 3 and 4 are the compressed sketches'. -k, --min-olap-length, --min-store-length and the -f file apply to the compressed reads: make the -f file with mhap-hip-kmers --hpc. FASTA input, one GPU.", "false", true);
  o.add("--trim-fasta", "With --trim, write the trimmed reads to this FASTA file; deleted reads are left out.", "");
  o.add("--trim-table", "With --trim, write one line per read to this file: id length begin end runs covered flags.", "");
}

[[noreturn]] void bad(const std::string& m) { printf("%s\n", m.c_str()); exit(1); }
// `rest` of "NAME belongs to ...: give ... too." for every given name whose owner is not
void owned(const Options& o, std::initializer_list<const char*> names, bool owner, const char* rest) {
  for (const char* n : names) if (o.isset(n) && !owner) bad(std::string(n) + rest);
}
// what every stage flag asks for: --realign, self overlaps, the reads' bases, one GPU
void stage_flag(const Options& o, size_t n_devs, const std::string& flag, const char* uses, const char* does, const char* needs) {
  if (!o.b("--realign")) bad(flag + " " + uses + " the alignments of --realign: give --realign too.");
  if (!o.s("-q").empty()) bad(flag + " " + does + " the reads of -s from their overlaps with each other: it takes no -q.");
  if (ends_with(o.s("-s"), ".dat")) bad(flag + " needs " + needs + ": give FASTA files, not .dat sketches.");
  if (n_devs > 1) bad(flag + " runs on one GPU: give one device (--gpus 1).");
}

// Every refusal happens here, before a handle exists: the MHAP-compatible options (MhapMain.java:93-380) and the settings line on stderr,
// the ranks, then the flags of the stages behind --realign in the order they were added (the first failing check is the one the user sees).
std::vector<int32_t> check_options(Options& o) {
  const int settings = o.i("--settings");
  if (settings < 0 || settings > 3) { printf("Please enter valid --settings flag. See options below:\n%s", o.helpText().c_str()); exit(1); }
  if (settings == 1) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "3"); o.setdef("--num-hashes", "512"); o.setdef("--threshold", "0.78"); o.setdef("--ordered-sketch-size", "1536"); o.setdef("--ordered-kmer-size", "12"); }
  if (settings == 2) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "3"); o.setdef("--num-hashes", "256"); o.setdef("--threshold", "0.80"); o.setdef("--ordered-sketch-size", "1000"); o.setdef("--ordered-kmer-size", "14"); }
  if (settings == 3) { o.setdef("-k", "16"); o.setdef("--num-min-matches", "2"); o.setdef("--num-hashes", "768"); o.setdef("--threshold", "0.73"); o.setdef("--ordered-sketch-size", "1536"); o.setdef("--ordered-kmer-size", "12"); }
  if (o.s("-s").empty() && o.s("-p").empty()) { printf("Please set the -s or the -p options. See options below:\n%s", o.helpText().c_str()); exit(1); }
  if (!o.s("-p").empty() && o.s("-q").empty()) { printf("Please set the -q option. See options below:\n%s", o.helpText().c_str()); exit(1); }
  for (const char* k : {"-p", "-s", "-q", "-f"}) if (!o.s(k).empty() && !exists(o.s(k))) { printf("Could not find requested file/folder: %s\n", o.s(k).c_str()); exit(1); }
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
  std::vector<int32_t> devs;   // ranks: --devices a,b,c  |  --gpus N from --device on  |  one handle
  if (!o.s("--devices").empty()) {
    const std::string dl = o.s("--devices");
    for (size_t i = 0; i < dl.size();) { size_t j = dl.find(',', i); if (j == std::string::npos) j = dl.size(); if (j > i) devs.push_back(atoi(dl.substr(i, j - i).c_str())); i = j + 1; }
  } else {
    if (o.i("--gpus") < 1) bad("The number of GPUs must be positive.");
    for (int r = 0; r < o.i("--gpus"); r++) devs.push_back(o.i("--device") + r);
  }
  if (devs.empty()) bad("No device given.");
  const size_t n_devs = devs.size();
  owned(o, {"--realign-paf"}, o.b("--realign"), " prints the alignments of --realign: give --realign too.");
  if (o.isset("--correct")) {
    stage_flag(o, n_devs, "--correct", "votes with", "corrects", "the reads' bases");
    if (o.s("--correct").empty()) bad("--correct needs the name of the FASTA file to write.");
    if (o.i("--correct-min-coverage") < 1) bad("The correction's minimum coverage must be >=1.");
  }
  owned(o, {"--correct-fastq"}, o.isset("--correct"), " belongs to --correct: give --correct too.");
  if (o.isset("--correct-fastq") && o.s("--correct-fastq").empty()) bad("--correct-fastq needs the name of the FASTQ file to write.");
  const char* realigned = "the overlaps realigned on the reads' bases";
  const bool best = o.isset("--best-overlaps") && o.i("--best-overlaps") != 0;
  owned(o, {"--best-min-span", "--best-table"}, best, " belongs to --best-overlaps: give --best-overlaps too.");
  if (best) {
    if (o.i("--best-overlaps") < 0) bad("The value of --best-overlaps must be >=0.");
    stage_flag(o, n_devs, "--best-overlaps", "selects among", "selects for", realigned);
    if (o.i("--best-min-span") < 0) bad("The value of --best-min-span must be >=0.");
    if (o.isset("--best-table") && o.s("--best-table").empty()) bad("--best-table needs the name of the file to write.");
  }
  const bool gfa = o.isset("--gfa");
  owned(o, {"--gfa-unitigs"}, gfa, " compacts the graph of --gfa: give --gfa too.");
  if (o.isset("--gfa-unitigs") && o.s("--gfa-unitigs").empty()) bad("--gfa-unitigs needs the name of the GFA file to write.");
  owned(o, {"--gfa-clean", "--gfa-tip-reads", "--gfa-bubble-bases", "--gfa-clean-rounds"}, gfa, " cleans the graph of --gfa: give --gfa too.");
  if (o.i("--gfa-tip-reads") < 0 || o.i("--gfa-bubble-bases") < 0 || o.i("--gfa-clean-rounds") < 1)
    bad("The values of --gfa-tip-reads and --gfa-bubble-bases must be >=0 and that of --gfa-clean-rounds >=1.");
  owned(o, {"--gfa-consensus", "--gfa-consensus-fasta", "--gfa-consensus-min-cov"}, o.isset("--gfa-unitigs"), " works on the unitigs of --gfa-unitigs: give --gfa-unitigs too.");
  owned(o, {"--gfa-consensus-fasta", "--gfa-consensus-min-cov"}, o.b("--gfa-consensus"), " belongs to --gfa-consensus: give --gfa-consensus too.");
  if (o.isset("--gfa-consensus-fasta") && o.s("--gfa-consensus-fasta").empty()) bad("--gfa-consensus-fasta needs the name of the FASTA file to write.");
  if (o.i("--gfa-consensus-min-cov") < 1) bad("The value of --gfa-consensus-min-cov must be >=1.");
  owned(o, {"--gfa-consensus-fastq"}, o.b("--gfa-consensus"), " belongs to --gfa-consensus: give --gfa-consensus too.");
  if (o.isset("--gfa-consensus-fastq") && o.s("--gfa-consensus-fastq").empty()) bad("--gfa-consensus-fastq needs the name of the FASTQ file to write.");
  owned(o, {"--quality-per-vote", "--quality-cap"}, o.isset("--correct-fastq") || o.isset("--gfa-consensus-fastq"), " belongs to --correct-fastq or --gfa-consensus-fastq: give one of them too.");
  if (o.i("--quality-per-vote") < 1 || o.i("--quality-per-vote") > 1000 || o.i("--quality-cap") < 1 || o.i("--quality-cap") > 93)
    bad("The value of --quality-per-vote must be 1 to 1000 and that of --quality-cap 1 to 93.");
  owned(o, {"--weigh-qualities"}, o.isset("--correct") || o.b("--gfa-consensus"), " weighs the votes of --correct or --gfa-consensus: give one of them too.");
  owned(o, {"--weight-q-lo", "--weight-q-hi"}, o.b("--weigh-qualities"), " belongs to --weigh-qualities: give --weigh-qualities too.");
  if (o.i("--weight-q-lo") < 0 || o.i("--weight-q-lo") > o.i("--weight-q-hi") || o.i("--weight-q-hi") > 93)
    bad("The values of --weight-q-lo and --weight-q-hi must be 0 <= --weight-q-lo <= --weight-q-hi <= 93.");
  if (gfa) {
    stage_flag(o, n_devs, "--gfa", "builds the graph from", "lays out", realigned);
    if (o.s("--gfa").empty()) bad("--gfa needs the name of the GFA file to write.");
    if (o.i("--gfa-max-hang") < 0 || o.i("--gfa-min-overlap") < 0 || o.i("--gfa-fuzz") < 0) bad("The values of --gfa-max-hang, --gfa-min-overlap and --gfa-fuzz must be >=0.");
  }
  const bool trim = o.b("--trim"), repeat = o.b("--repeat-filter");
  owned(o, {"--trim-min-cov", "--trim-end-clip", "--trim-min-span", "--trim-fasta", "--trim-table"}, trim, " belongs to --trim: give --trim too.");
  owned(o, {"--trim-penalty"}, trim || repeat, " belongs to --trim: give --trim too.");
  owned(o, {"--repeat-factor", "--repeat-max-cov", "--repeat-min-run", "--repeat-min-unique", "--repeat-table"}, repeat, " belongs to --repeat-filter: give --repeat-filter too.");
  owned(o, {"--variant-min-depth", "--variant-min-minor", "--variant-min-pct", "--variant-max-del-pct", "--variant-min-diff", "--variant-diff-pct", "--variant-table"}, o.b("--variant-filter"),
        " belongs to --variant-filter: give --variant-filter too.");
  if (o.b("--variant-filter")) {
    stage_flag(o, n_devs, "--variant-filter", "votes with", "marks", "the reads' bases");
    const auto pct = [&](const char* n) { return o.i(n) >= 0 && o.i(n) <= 100; };
    if (o.i("--variant-min-depth") < 1 || o.i("--variant-min-minor") < 1 || o.i("--variant-min-diff") < 1 || !pct("--variant-min-pct") || !pct("--variant-max-del-pct") || !pct("--variant-diff-pct"))
      bad("The values of --variant-min-depth, --variant-min-minor and --variant-min-diff must be >=1 and those of --variant-min-pct, --variant-max-del-pct and --variant-diff-pct 0 to 100.");
    if (o.isset("--variant-table") && o.s("--variant-table").empty()) bad("--variant-table needs the name of the file to write.");
  }
  if (repeat) {
    stage_flag(o, n_devs, "--repeat-filter", "piles up", "marks", realigned);
    if (o.i("--repeat-factor") < 100 || o.i("--repeat-max-cov") < 0 || o.i("--repeat-min-run") < 1 || o.i("--repeat-min-unique") < 0 || o.i("--trim-penalty") < 0)
      bad("The value of --repeat-factor must be >=100, that of --repeat-min-run >=1 and those of --repeat-max-cov, --repeat-min-unique and --trim-penalty >=0.");
    if (o.isset("--repeat-table") && o.s("--repeat-table").empty()) bad("--repeat-table needs the name of the file to write.");
  }
  if (trim) {
    stage_flag(o, n_devs, "--trim", "piles up", "trims", realigned);
    if (o.i("--trim-min-cov") < 1 || o.i("--trim-end-clip") < 0 || o.i("--trim-min-span") < 0 || o.i("--trim-penalty") < 0)
      bad("The value of --trim-min-cov must be >=1 and those of --trim-end-clip, --trim-min-span and --trim-penalty >=0.");
    for (const char* n : {"--trim-fasta", "--trim-table"})
      if (o.isset(n) && o.s(n).empty()) bad(std::string(n) + " needs the name of the file to write.");
  }
  if (o.b("--hpc")) {
    if (!o.s("-p").empty()) bad("--hpc compresses the reads of a search: it does not go with -p.");
    bool dat = ends_with(o.s("-s"), ".dat");
    if (!o.s("-q").empty()) for (const std::string& cf : list_files(o.s("-q"))) dat = dat || ends_with(cf, ".dat");
    if (dat) bad("--hpc needs the reads' bases: give FASTA files, not .dat sketches.");
    if (n_devs > 1) bad("--hpc runs on one GPU: give one device (--gpus 1).");
  }
  if (o.b("--realign") && o.s("-p").empty()) {
    if (o.i("--realign-band") < 0) bad("The realignment band must be >=0.");
    if (n_devs > 1) bad("--realign runs on one GPU: give one device (--gpus 1).");
    bool dat = ends_with(o.s("-s"), ".dat");
    if (!o.s("-q").empty()) for (const std::string& cf : list_files(o.s("-q"))) dat = dat || ends_with(cf, ".dat");
    if (dat) bad("--realign needs the reads' bases: give FASTA files, not .dat sketches.");
  }
  return devs;
}

// mhap_create is mostly the HIP runtime coming up (~0.25 s): it runs on its own thread while this one maps and scans the FASTA file the index is built from
Engine create_engine(const Options& o, mhap_params& P, std::vector<int32_t>& devs, bool precompute) {
  if (precompute && devs.size() > 1) { fprintf(stderr, "Usage 2 (-p) writes its .dat files from one GPU: using device %d only.\n", devs[0]); devs.resize(1); }
  Engine E; E.n = (int)devs.size();
  char err[512] = {0};
  const double t_create = now();
  int rc_create = MHAP_OK;
  std::thread creator([&]() {
    if (devs.size() == 1) { P.device = devs[0]; rc_create = mhap_create(&P, &E.h, err, sizeof err); }
    else rc_create = mhap_group_create(&P, devs.data(), (int32_t)devs.size(), &E.g, err, sizeof err);
  });
  if (!precompute && !o.b("--hpc") && !is_dir(o.s("-s")) && !ends_with(o.s("-s"), ".dat")) {
    char perr[512] = {0};
    if (mhap_fasta_scan_open(o.s("-s").c_str(), 0, &g_preload.scan, perr, sizeof perr) == MHAP_OK) g_preload.path = o.s("-s");
    else g_preload.scan = nullptr;
    // (a failure is reported by the regular scan below)
  }
  creator.join();
  if (rc_create != MHAP_OK) die(err);
  if (getenv("MHAP_HOST_PROF")) fprintf(stderr, "[cli] mhap_create + first FASTA scan %.3f s\n", now() - t_create);
  if (E.g) fprintf(stderr, "Using %d GPU ranks (reads dealt round-robin; every rank indexes its share).\n", E.n);
  return E;
}

// Usage 2: precompute `.dat` (MhapMain.java:384-451)
void precompute_dat(const Engine& E, const Options& o, const mhap_params& P) {
  fprintf(stderr, "Processing FASTA files for binary compression...\n");
  if (!is_dir(o.s("-q"))) die("Target directory doesn't exit.");
  for (const std::string& pf : list_files(o.s("-p"))) {
    const double t = now();
    chk(E.h, mhap_index_clear(E.h));
    int64_t strands = 0;
    add_file_to_index(E, pf, 0, o, &strands);
    std::string name = pf.substr(pf.find_last_of('/') + 1);
    size_t dot = name.find_last_of('.'); if (dot != std::string::npos && dot > 0) name = name.substr(0, dot);
    const std::string out = o.s("-q") + "/" + name + ".dat";
    write_dat(E.h, out, P.num_hashes, P.ordered_sketch_size, P.ordered_kmer_size);
    fprintf(stderr, "Processed %lld sequences (fwd and rev).\n", (long long)strands);
    fprintf(stderr, "Read, hashed, and stored file %s to %s.\n", pf.c_str(), out.c_str());
    fprintf(stderr, "Time (s): %g\n", now() - t);
  }
}

// --realign: the reads of -s (ids as the index assigned them: FastaData's running count), every stage's parameters from its flags, and the sessions that begin before the search
void begin_pipeline(const Options& o, mhap_handle* h, Pipeline& p) {
  const bool weigh = o.b("--weigh-qualities");
  for (const std::string& sf : p.reads.n() > 0 ? std::vector<std::string>() : list_files(o.s("-s"))) p.reads.read_file(sf, weigh);   // (--hpc has read them already)
  p.correct.weigh = p.graph.weigh = weigh;
  p.correct.wp = p.graph.wp = mhap_weight_params{o.i("--weight-q-lo"), o.i("--weight-q-hi")};
  if (weigh) p.reads.weight_line(p.correct.wp);
  p.realign.h = p.select.h = p.correct.h = p.variant.h = p.repeat.h = p.trim.h = p.graph.h = h;
  p.realign.reads = &p.reads; p.realign.band = o.i("--realign-band"); p.realign.min_identity = o.d("--realign-min-identity");
  p.paf = o.b("--realign-paf");
  p.correct.on = o.isset("--correct"); p.correct.fasta = o.s("--correct"); p.correct.min_cov = o.i("--correct-min-coverage");
  p.correct.quality.fastq = o.s("--correct-fastq"); p.graph.quality.fastq = o.s("--gfa-consensus-fastq");
  p.correct.quality.p = p.graph.quality.p = mhap_quality_params{o.i("--quality-per-vote"), o.i("--quality-cap")};
  p.select.on = o.isset("--best-overlaps") && o.i("--best-overlaps") != 0; p.select.table = o.s("--best-table");
  mhap_select_default_params(&p.select.p);
  p.select.p.best_n = o.i("--best-overlaps"); p.select.p.min_span = o.i("--best-min-span");
  p.variant.on = o.b("--variant-filter"); p.variant.table = o.s("--variant-table");
  p.variant.p = mhap_variant_params{o.i("--variant-min-depth"), o.i("--variant-min-minor"), o.i("--variant-min-pct"), o.i("--variant-max-del-pct"), o.i("--variant-min-diff"), o.i("--variant-diff-pct")};
  p.repeat.on = o.b("--repeat-filter"); p.repeat.table = o.s("--repeat-table");
  mhap_repeat_default_params(&p.repeat.p);
  p.repeat.p.factor_pct = o.i("--repeat-factor"); p.repeat.p.max_cov = o.i("--repeat-max-cov"); p.repeat.p.min_run = o.i("--repeat-min-run"); p.repeat.p.min_unique = o.i("--repeat-min-unique");
  p.trim.on = o.b("--trim"); p.trim.fasta = o.s("--trim-fasta"); p.trim.table = o.s("--trim-table"); p.trim.penalty = o.i("--trim-penalty");
  mhap_trim_default_params(&p.trim.p);
  p.trim.p.min_cov = o.i("--trim-min-cov"); p.trim.p.end_clip = o.i("--trim-end-clip"); p.trim.p.min_span = o.i("--trim-min-span");
  p.graph.on = o.isset("--gfa"); p.graph.gfa = o.s("--gfa"); p.graph.unitigs = o.s("--gfa-unitigs");
  mhap_graph_default_params(&p.graph.p);
  p.graph.p.max_hang = o.i("--gfa-max-hang"); p.graph.p.min_ovlp = o.i("--gfa-min-overlap"); p.graph.p.fuzz = o.i("--gfa-fuzz");
  p.graph.clean = o.b("--gfa-clean"); p.graph.cp.tip_reads = o.i("--gfa-tip-reads"); p.graph.cp.bubble_bases = o.i("--gfa-bubble-bases"); p.graph.cp.max_rounds = o.i("--gfa-clean-rounds");
  p.graph.consensus = o.b("--gfa-consensus"); p.graph.consensus_fasta = o.s("--gfa-consensus-fasta"); mhap_consensus_default_params(&p.graph.kp); p.graph.kp.min_cov = o.i("--gfa-consensus-min-cov");
  p.begin();
}

// --hpc: the files of -s read whole into the table of reads (ids as the index assigns them), compressed on the GPU, and the compressed
// reads sketched and indexed under those ids; the reads the index took, as add_file_to_index counts them
int64_t add_compressed_to_index(const Engine& E, const Options& o, HpcStage& hpc, int64_t* strands) {
  Reads& R = *hpc.reads;
  for (const std::string& sf : list_files(o.s("-s")))
    R.read_file(sf, o.b("--weigh-qualities"), [](const mhap_fasta& fa) { if (g_headers.full) collect_headers(fa); });
  hpc.compress(0, hpc.index);
  const HpcSide& s = hpc.index;
  if (s.n > 0) chk(E.h, mhap_index_add_reads(E.h, (const char*)s.bases.data(), s.offsets.data(), s.lengths.data(), hpc.ids(s), s.n));
  const mhap_stats st = E.stats();
  *strands = st.strands_indexed;
  return st.strands_indexed / 2;
}

// Usage 1: the index against itself, then every -q file against it (MhapMain.java:453-570)
void search(const Engine& E, const Options& o, const mhap_params& P, Sink& sink, int64_t seq_processed) {
  char err[512] = {0};
  const double t_score = now();
  double t = now();
  if (o.s("-q").empty() || !o.b("--no-self")) {
    E.find_self(sink_cb, &sink);
    sink_flush(sink);
    fprintf(stderr, "Time (s) to score and output to self: %g\n", now() - t);
  }
  for (const std::string& cf : o.s("-q").empty() ? std::vector<std::string>() : list_files(o.s("-q"))) {
    t = now();
    fprintf(stderr, "Opened fasta file %s.\n", cf.c_str());
    int64_t nq = 0;
    if (ends_with(cf, ".dat")) {   // precomputed query sketches: forward entries only (SequenceSketchStreamer.java:291-303)
      if (E.g) die("--gpus N takes FASTA input (precomputed .dat sketches are searched on one GPU)");
      DatEntries d;
      read_dat(cf, seq_processed, P.num_hashes, P.ordered_sketch_size, true, d);
      if (g_headers.full) for (size_t i = 0; i < d.ids.size(); i++) g_headers.byid[d.ids[i]] = d.hdr[i];
      if (!d.ids.empty())
        chk(E.h, mhap_find_matches_sketches(E.h, d.ids.data(), d.seqlen.data(), d.mh.data(), d.ord.data(), d.osz.data(), d.olen.data(),
                                          (int64_t)d.ids.size(), sink_cb, &sink));
      nq = (int64_t)d.ids.size();
    } else {
      mhap_fasta fa;
      if (mhap_fasta_read(cf.c_str(), seq_processed, &fa, err, sizeof err) != MHAP_OK) die(err);   // id offset = reads so far (MhapMain.java:527)
      if (g_headers.full) collect_headers(fa);
      const int64_t first = sink.hpc ? sink.hpc->reads->n() : 0;
      if (sink.pipeline) sink.pipeline->reads.add(fa);
      else if (sink.hpc) sink.hpc->own.add(fa);
      const mhap_stats s0 = E.stats();
      if (sink.hpc) {   // the file's reads compressed, searched as they are then, and every record expanded from this file's maps to the index's
        HpcStage& H = *sink.hpc;
        H.compress(first, H.query);
        H.querying = true;
        const HpcSide& q = H.query;
        if (q.n > 0) chk(E.h, mhap_find_matches_reads(E.h, (const char*)q.bases.data(), q.offsets.data(), q.lengths.data(), H.ids(q), q.n, sink_cb, &sink));
        H.querying = false;
      } else
        E.find_reads(fa, sink_cb, &sink);
      nq = E.stats().queries_searched - s0.queries_searched;   // forward sketches produced = getNumberProcessed() (MhapMain.java:537)
      mhap_fasta_free(&fa);
    }
    sink_flush(sink);
    seq_processed += nq;
    fprintf(stderr, "Processed %lld to sequences.\n", (long long)nq);
    fprintf(stderr, "Time (s) to score, hash to-file, and output: %g\n", now() - t);
  }
  sink_flush(sink);
  fprintf(stderr, "Total scoring time (s): %g\n", now() - t_score);
}

// outputFinalStat (MhapMain.java:572-590); the inverted-index counters have no brute-force analogue
void final_statistics(const Engine& E) {
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
}

}  // namespace

int main(int argc, char** argv) {
  Options o;
  declare_options(o);
  if (!o.parse(argc, argv)) return 0;
  std::vector<int32_t> devs = check_options(o);
  mhap_params P; mhap_default_params(&P);
  P.kmer_size = o.i("-k"); P.num_hashes = o.i("--num-hashes"); P.ordered_kmer_size = o.i("--ordered-kmer-size");
  P.ordered_sketch_size = o.i("--ordered-sketch-size"); P.num_min_matches = o.i("--num-min-matches");
  P.min_store_length = o.i("--min-store-length"); P.min_olap_length = o.i("--min-olap-length"); P.device = o.i("--device");
  P.threshold = o.d("--threshold"); P.max_shift = o.d("--max-shift"); P.repeat_weight = o.d("--repeat-weight");
  const bool precompute = !o.s("-p").empty();
  Engine E = create_engine(o, P, devs, precompute);

  const double t_total = now();
  if (!o.s("-f").empty()) load_filter(E, o);
  if (precompute) {
    precompute_dat(E, o, P);
    fprintf(stderr, "Total time (s): %g\n", now() - t_total);
    E.destroy();
    return 0;
  }

  fprintf(stderr, "Processing files for storage in reverse index...\n");
  const double t_proc = now();
  int64_t strands = 0;
  Sink sink;
  Pipeline pipeline;
  HpcStage hpc;
  if (o.b("--hpc")) {
    hpc.on = true; hpc.h = E.h;
    if (o.b("--realign")) hpc.reads = &pipeline.reads;   // the raw reads are kept once
    sink.hpc = &hpc;
  }
  const int64_t seq_processed = hpc.on ? add_compressed_to_index(E, o, hpc, &strands) : add_file_to_index(E, o.s("-s"), 0, o, &strands);
  fprintf(stderr, "Stored %lld sequences in the index.\n", (long long)strands);
  fprintf(stderr, "Processed %lld unique sequences (fwd and rev).\n", (long long)strands);
  fprintf(stderr, "Time (s) to read and hash from file: %g\n", now() - t_proc);

  if (o.b("--realign")) { begin_pipeline(o, E.h, pipeline); sink.pipeline = &pipeline; }
  search(E, o, P, sink, seq_processed);
  if (hpc.on) hpc.finish();
  if (sink.pipeline) pipeline.finish();
  fprintf(stderr, "Total time (s): %g\n", now() - t_total);
  final_statistics(E);
  // everything is written: leave without tearing down gigabytes of device and host mappings one by one (the kernel does it faster)
  fflush(nullptr);
  _exit(0);
}
