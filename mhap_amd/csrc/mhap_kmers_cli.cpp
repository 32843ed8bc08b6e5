// mhap_kmers_cli.cpp — `mhap-hip-kmers`: counts the k-mers of FASTA files on the GPU and writes the `-f` repeat filter file that
// `mhap-hip -f` (and MHAP's FrequencyCounts, J/sketch/FrequencyCounts.java:63-200) reads.  MHAP has no such tool; its users bring the
// file from a k-mer counter.  Inputs are plain, gz or bz2 FASTA files or directories of them, read by the streamed ingest.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mhap_hip.h"

namespace {

const char* USAGE =
    "Usage: mhap-hip-kmers -o <output file> [-k 16] [--no-rc] [--hpc] [--min-fraction 2.5e-6] [--histogram <file>] [--device 0] <FASTA file or directory> ...\n"
    "       mhap-hip-kmers --assess <FASTA> [--assess-min-count 0] [--assess-table <file>] [--assess-bed <file>] [-o ...] [-k 16] [--no-rc] <FASTA file or directory> ...\n"
    "  -o               the k-mer filter file to write (the -f file of mhap-hip; optional with --assess)\n"
    "  -k               k-mer size, 1 to 16 (default 16)\n"
    "  --no-rc          count k-mers as they are read instead of canonical (the smaller of a k-mer and its reverse complement)\n"
    "  --hpc            count the k-mers of the homopolymer-compressed reads (every run of equal bases collapsed to one, on the GPU):\n"
    "                   the -f file of a `mhap-hip --hpc` search, which sketches the compressed reads, has to be made this way\n"
    "  --min-fraction   write the k-mers whose share of all counted k-mers is at least this (default 2.5e-6)\n"
    "  --histogram      also write the k-mer count histogram, \"<count>\\t<number of k-mers>\" per line in ascending count\n"
    "                   (what `python -m mhap_amd.histogram_stats <file> <percent>` reads to help choose --min-fraction)\n"
    "  --assess         assess the sequences of this FASTA file against the k-mers of the inputs: k-mers of the sequences that the reads\n"
    "                   do not support (a consensus QV) and solid k-mers of the reads that the sequences lack (completeness)\n"
    "  --assess-min-count  a k-mer of the reads is solid when it is counted at least this often (default 0: the valley of the count histogram)\n"
    "  --assess-table   write \"name\\tbases\\twindows\\tmissing\\truns\\tunsupported\\terror\\tqv\" per sequence and a total line\n"
    "  --assess-bed     write \"name\\tbegin\\tend\" per stretch of bases that no supported k-mer covers\n"
    "  --device         HIP device ordinal (default 0)\n";

[[noreturn]] void die(const std::string& m) {
  fprintf(stderr, "mhap-hip-kmers: %s\n%s", m.c_str(), USAGE);
  exit(1);
}

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }

std::vector<std::string> list_files(const std::string& path) {   // non-hidden entries, sorted
  std::vector<std::string> out;
  if (!is_dir(path)) { out.push_back(path); return out; }
  DIR* d = opendir(path.c_str());
  if (!d) return out;
  while (dirent* e = readdir(d)) { std::string n = e->d_name; if (n.empty() || n[0] == '.') continue; out.push_back(path + "/" + n); }
  closedir(d);
  std::sort(out.begin(), out.end());
  return out;
}

bool parse_int(const char* s, long& v) { char* e = nullptr; v = strtol(s, &e, 10); return *s && e && *e == 0; }
bool parse_double(const char* s, double& v) { char* e = nullptr; v = strtod(s, &e); return *s && e && *e == 0 && v == v; }

}  // namespace

int main(int argc, char** argv) {
  std::string out, histogram, assess, assess_table, assess_bed;
  long k = 16, device = 0, assess_min_count = 0;
  bool assess_options = false;
  double min_fraction = 2.5e-6;
  bool rc = true, hpc = false;
  std::vector<std::string> inputs;
  for (int a = 1; a < argc; a++) {
    const std::string s = argv[a];
    auto value = [&]() -> const char* { if (a + 1 >= argc) die("option " + s + " requires a value"); return argv[++a]; };
    if (s == "-h" || s == "--help") { fputs(USAGE, stdout); return 0; }
    else if (s == "-o") out = value();
    else if (s == "-k") { if (!parse_int(value(), k)) die("-k takes an integer"); }
    else if (s == "--no-rc") rc = false;
    else if (s == "--hpc") hpc = true;
    else if (s == "--histogram") histogram = value();
    else if (s == "--min-fraction") { if (!parse_double(value(), min_fraction)) die("--min-fraction takes a number"); }
    else if (s == "--assess") assess = value();
    else if (s == "--assess-min-count") { assess_options = true; if (!parse_int(value(), assess_min_count) || assess_min_count < 0) die("--assess-min-count takes an integer that is not negative"); }
    else if (s == "--assess-table") { assess_options = true; assess_table = value(); }
    else if (s == "--assess-bed") { assess_options = true; assess_bed = value(); }
    else if (s == "--device") { if (!parse_int(value(), device) || device < 0) die("--device takes a device ordinal"); }
    else if (!s.empty() && s[0] == '-') die("unknown option " + s);
    else inputs.push_back(s);
  }
  if (assess_options && assess.empty()) die("--assess-min-count, --assess-table and --assess-bed go with --assess <FASTA>");
  if (hpc && !assess.empty()) die("--hpc makes the -f file of a compressed search: it does not go with --assess");
  if (out.empty() && assess.empty()) die("no output file (-o)");
  if (out.empty() && !histogram.empty()) die("--histogram goes with -o");
  if (inputs.empty()) die("no input file");
  if (k < 1 || k > 16) die("k-mer size must be from 1 to 16 (got " + std::to_string(k) + ")");
  const double t0 = now();
  mhap_params p;
  mhap_default_params(&p);
  p.num_hashes = 1; p.ordered_sketch_size = 1;   // (no sketching here: the smallest per-handle tables)
  p.device = (int32_t)device;
  mhap_handle* h = nullptr;
  char err[512] = {0};
  if (mhap_create(&p, &h, err, sizeof err) != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: %s\n", err); return 1; }
  auto chk = [&](int r) { if (r != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: %s (code %d)\n", mhap_last_error(h), r); mhap_destroy(h); exit(1); } };
  chk(mhap_kmer_count_begin(h, (int32_t)k, rc ? 1 : 0));
  int64_t reads = 0, bases = 0, hpc_counts[MHAP_HPC_COUNTS] = {0, 0, 0, 0, 0, 0};
  double t_scan = 0.0, t_count = 0.0;
  for (const std::string& in : inputs) {
    for (const std::string& f : list_files(in)) {
      const double a = now();
      if (hpc) {   // the file read whole, compressed on the GPU, and the compressed reads counted as they are
        mhap_fasta fa;
        if (mhap_fasta_read(f.c_str(), 0, &fa, err, sizeof err) != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: %s\n", err); mhap_destroy(h); return 1; }
        const double b = now();
        reads += fa.n; bases += fa.total_bases;
        mhap_hpc* c = nullptr;
        int r = mhap_hpc_compress(h, (const uint8_t*)fa.bases, fa.total_bases, fa.ids, fa.offsets, fa.lengths, fa.n, 0, &c);
        mhap_fasta_free(&fa);
        chk(r);
        int64_t cc[MHAP_HPC_COUNTS];
        mhap_hpc_info(c, cc);
        for (int i = 0; i < MHAP_HPC_COUNTS; i++) hpc_counts[i] = i == 4 ? std::max(hpc_counts[i], cc[i]) : hpc_counts[i] + cc[i];
        std::vector<uint8_t> cb((size_t)std::max<int64_t>(cc[2], 1));
        std::vector<int64_t> coff((size_t)cc[0] + 1);
        std::vector<int32_t> clen((size_t)std::max<int64_t>(cc[0], 1));
        r = mhap_hpc_copy(c, cb.data(), coff.data(), clen.data(), nullptr);
        mhap_hpc_free(c);
        chk(r);
        if (cc[0] > 0) chk(mhap_kmer_count_add_reads(h, (const char*)cb.data(), coff.data(), clen.data(), cc[0]));
        t_scan += b - a; t_count += now() - b;
        continue;
      }
      mhap_fasta_scan* s = nullptr;
      if (mhap_fasta_scan_open(f.c_str(), 0, &s, err, sizeof err) != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: %s\n", err); mhap_destroy(h); return 1; }
      const double b = now();
      reads += mhap_fasta_scan_reads(s); bases += mhap_fasta_scan_bases(s);
      const int r = mhap_kmer_count_add_scan(h, s);
      mhap_fasta_scan_free(s);
      chk(r);
      t_scan += b - a; t_count += now() - b;
    }
  }
  int64_t total = 0, distinct = 0, lines = 0;
  int32_t kk = 0;
  double tw = 0.0, tw1 = 0.0;
  if (!out.empty()) {   // with --assess the count stays open: the set is made from the same count of the reads
    mhap_kmer_counts* c = nullptr;
    chk(mhap_kmer_count_finish_flags(h, min_fraction, (histogram.empty() ? 0u : (uint32_t)MHAP_KMER_HISTOGRAM) | (assess.empty() ? 0u : (uint32_t)MHAP_KMER_KEEP_OPEN), &c));
    mhap_kmer_counts_info(c, &total, &distinct, &lines, &kk);
    tw = now();
    const int w = mhap_kmer_counts_write(c, out.c_str());
    const int wh = w != MHAP_OK || histogram.empty() ? MHAP_OK : mhap_kmer_counts_write_histogram(c, histogram.c_str());
    mhap_kmer_counts_free(c);
    tw1 = now();
    if (w != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: cannot write %s\n", out.c_str()); mhap_destroy(h); return 1; }
    if (wh != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: cannot write %s\n", histogram.c_str()); mhap_destroy(h); return 1; }
  }
  char line[1024] = {0};
  if (!assess.empty()) {
    mhap_kmer_set *solid = nullptr, *own = nullptr;
    chk(mhap_kmer_count_finish_set(h, (uint64_t)assess_min_count, &solid));
    if (out.empty()) {
      int64_t members = 0; int32_t canonical = 0; uint64_t mc = 0;
      mhap_kmer_set_info(solid, &total, &distinct, &members, &kk, &canonical, &mc);
    }
    mhap_fasta_scan* s = nullptr;
    if (mhap_fasta_scan_open(assess.c_str(), 0, &s, err, sizeof err) != MHAP_OK) { fprintf(stderr, "mhap-hip-kmers: %s\n", err); mhap_kmer_set_free(solid); mhap_destroy(h); return 1; }
    mhap_kmer_eval* ev = nullptr;
    int64_t both = 0;
    int r = mhap_kmer_eval_scan(h, solid, s, &ev);
    // completeness: the set of the sequences' own k-mers (every one of them: count >= 1) against the solid set
    if (r == MHAP_OK) r = mhap_kmer_count_begin(h, (int32_t)k, rc ? 1 : 0);
    if (r == MHAP_OK) r = mhap_kmer_count_add_scan(h, s);
    if (r == MHAP_OK) r = mhap_kmer_count_finish_set(h, 1, &own);
    if (r == MHAP_OK) r = mhap_kmer_set_compare(h, solid, own, nullptr, nullptr, &both);
    const char* names = nullptr;
    if (r == MHAP_OK) r = mhap_fasta_scan_info(s, nullptr, nullptr, &names, nullptr);
    std::string failed;
    if (r == MHAP_OK && !assess_table.empty() && mhap_kmer_eval_write_table(ev, names, assess_table.c_str()) != MHAP_OK) failed = assess_table;
    if (r == MHAP_OK && failed.empty() && !assess_bed.empty() && mhap_kmer_eval_write_bed(ev, names, assess_bed.c_str()) != MHAP_OK) failed = assess_bed;
    if (r == MHAP_OK) (void)mhap_kmer_eval_summary(ev, solid, own, both, line, sizeof line);
    if (r != MHAP_OK) fprintf(stderr, "mhap-hip-kmers: %s (code %d)\n", mhap_last_error(h), r);
    if (!failed.empty()) fprintf(stderr, "mhap-hip-kmers: cannot write %s\n", failed.c_str());
    mhap_kmer_eval_free(ev);
    mhap_fasta_scan_free(s);
    mhap_kmer_set_free(own);
    mhap_kmer_set_free(solid);
    if (r != MHAP_OK || !failed.empty()) { mhap_destroy(h); return 1; }
  }
  mhap_destroy(h);
  if (!out.empty())
    fprintf(stderr, "Counted %lld %d-mers (%lld distinct) in %lld reads, %.1f Mbase; wrote %lld lines to %s; total %.3f s (scan %.3f s, count %.3f s, write %.3f s)\n",
            (long long)total, (int)kk, (long long)distinct, (long long)reads, bases / 1e6, (long long)lines, out.c_str(), now() - t0, t_scan, t_count, tw1 - tw);
  else
    fprintf(stderr, "Counted %lld %d-mers (%lld distinct) in %lld reads, %.1f Mbase; total %.3f s (scan %.3f s, count %.3f s)\n", (long long)total, (int)kk,
            (long long)distinct, (long long)reads, bases / 1e6, now() - t0, t_scan, t_count);
  if (hpc)
    fprintf(stderr, "Homopolymer compression: %lld reads (%lld empty), %lld bases compressed to %lld; %lld runs longer than 1, the longest of %lld\n", (long long)hpc_counts[0],
            (long long)hpc_counts[5], (long long)hpc_counts[1], (long long)hpc_counts[2], (long long)hpc_counts[3], (long long)hpc_counts[4]);
  if (!assess.empty()) fprintf(stderr, "%s\n", line);
  return 0;
}
