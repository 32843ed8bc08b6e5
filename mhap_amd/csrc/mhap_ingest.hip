// mhap_ingest.hip — streamed FASTA ingest: file text -> 2-bit packed reads in pinned staging -> HBM, overlapped with the kernels.
//
// The reference reads and sketches through a queue (FastaData.dequeue / enqueueNextSequenceInFile, J/impl/FastaData.java:101-204;
// SequenceSketchStreamer.enqueueFullFile with T threads, J/impl/SequenceSketchStreamer.java:179-222).  Round 2's driver did the
// same steps one after the other — parse the whole file into one byte per base, pack it, upload it, sketch it — and 83 % of
// its wall time was host time.  Here the file is mapped and scanned once on all host threads (record boundaries, lengths, is-it-ACGT;
// nothing is copied), and the index is fed in groups: while the GPU sketches and indexes group g, host threads pack group g+1 from
// the mapped text straight into the other of two pinned staging buffers.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fastq_host.hpp"
#include "kernels.hpp"
#include "mhap_internal.hpp"

using namespace mhap;

namespace mhap {
struct FastaScanImpl {
  const char* D = nullptr; size_t N = 0;      // the text
  void* map_base = nullptr; size_t map_len = 0;
  std::string owned;                          // inflated gz / bz2 input, pipes
  // per non-empty record
  std::vector<uint64_t> hdr, body, end;       // offsets of '>', of the first byte after the header line, of the record's end
  bool fastq = false;                         // the text is FASTQ: hdr is the '@', end the '+' line, and the qualities lie in [qual, qual_end)
  std::vector<uint64_t> qual, qual_end;
  std::vector<int32_t> len;                   // bases
  std::vector<uint8_t> raw;                   // 1: has a char other than ACGT/acgt (kept as upper-cased bytes on the device)
  std::vector<uint8_t> oneline;               // 1: the sequence is one line (packed straight from the text)
  std::vector<int64_t> ids;
  int64_t total_bases = 0;
  std::string names; bool names_done = false;
  ~FastaScanImpl() { if (map_base) munmap(map_base, map_len); }
};
}  // namespace mhap
struct mhap_fasta_scan { FastaScanImpl impl; };

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool prof() { static int p = -1; if (p < 0) p = getenv("MHAP_HOST_PROF") ? 1 : 0; return p == 1; }

int host_threads() { return usable_host_threads(64); }

void parallel_chunks(int64_t n, int nthreads, const std::function<void(int64_t, int64_t, int)>& fn) {
  if (n <= 0) return;
  nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, n));
  if (nthreads == 1) { fn(0, n, 0); return; }
  std::vector<std::thread> th;
  const int64_t chunk = (n + nthreads - 1) / nthreads;
  for (int t = 0; t < nthreads; t++) {
    const int64_t lo = t * chunk, hi = std::min(n, lo + chunk);
    if (lo >= hi) break;
    th.emplace_back([=, &fn]() { fn(lo, hi, t); });
  }
  for (auto& t : th) t.join();
}

// 2-bit code of a base in either case: (c >> 1) & 3 maps A,C,G,T (a,c,g,t) to 0,1,3,2; x ^ (x >> 1) turns that into 0,1,2,3
inline uint32_t base_code(uint8_t c) { const uint32_t x = (c >> 1) & 3u; return x ^ (x >> 1); }
inline bool is_base(uint8_t c) { return ((0x54474341u >> (8 * base_code(c))) & 0xFFu) == (uint32_t)(c & 0xDFu); }
inline uint8_t upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 'a' + 'A') : c; }   // toUpperCase(Locale.ENGLISH), FastaData.java:194
inline int64_t align4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// pack L bases at s (ACGT in either case) into dst, 4 per byte, zero-padded to a multiple of 4 bytes
void pack_bases(const uint8_t* s, int L, uint8_t* dst) {
  const int full = L >> 2;
  for (int q = 0; q < full; q++)
    dst[q] = (uint8_t)(base_code(s[4 * q]) | (base_code(s[4 * q + 1]) << 2) | (base_code(s[4 * q + 2]) << 4) | (base_code(s[4 * q + 3]) << 6));
  const int nb = (int)align4((L + 3) / 4);
  for (int q = full; q < nb; q++) {
    uint32_t v = 0;
    for (int j = 4 * q; j < L && j < 4 * q + 4; j++) v |= base_code(s[j]) << (2 * (j & 3));
    dst[q] = (uint8_t)v;
  }
}

bool inflate_file(const std::string& name, std::string& data, std::string& err) {
  char buf[1 << 16];
  auto ends = [&](const char* suf) { const size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
  if (ends("bz2")) {
    void* lib = dlopen("libbz2.so.1.0", RTLD_NOW);
    if (!lib) lib = dlopen("libbz2.so.1", RTLD_NOW);
    typedef void* (*open_t)(const char*, const char*); typedef int (*read_t)(void*, void*, int); typedef void (*close_t)(void*);
    open_t bzopen = lib ? (open_t)dlsym(lib, "BZ2_bzopen") : nullptr;
    read_t bzread = lib ? (read_t)dlsym(lib, "BZ2_bzread") : nullptr;
    close_t bzclose = lib ? (close_t)dlsym(lib, "BZ2_bzclose") : nullptr;
    if (!bzopen || !bzread || !bzclose) { err = "bzip2 input needs libbz2.so.1.0"; return false; }
    void* bf = bzopen(name.c_str(), "rb");
    if (!bf) { err = "cannot open " + name; return false; }
    int got;
    while ((got = bzread(bf, buf, (int)sizeof buf)) > 0) data.append(buf, (size_t)got);
    bzclose(bf);
    return true;
  }
  gzFile gf = gzopen(name.c_str(), "rb");
  if (!gf) { err = "cannot open " + name; return false; }
  int got;
  while ((got = gzread(gf, buf, (unsigned)sizeof buf)) > 0) data.append(buf, (size_t)got);
  gzclose(gf);
  return true;
}

// One group of reads on its way to the GPU.
struct Slot {
  uint8_t* pin = nullptr; size_t cap = 0;     // pinned staging
  std::vector<ReadDesc> descs; std::vector<int64_t> ids;
  size_t bytes = 0;
  bool ready = false, last = false;
};

// the records idx[lo, hi) of the scan packed into slot (descs, ids, bytes); false on allocation failure
bool pack_group(const FastaScanImpl& sc, const std::vector<int64_t>& idx, int64_t lo, int64_t hi, int min_olap, bool fwd_only, Slot& slot, int nthreads) {
  const int64_t n = hi - lo;
  slot.descs.assign((size_t)n, ReadDesc{});
  slot.ids.resize((size_t)n);
  int64_t store = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t r = idx[(size_t)(lo + i)];
    ReadDesc& d = slot.descs[(size_t)i];
    d.length = sc.len[(size_t)r];
    d.flags = 0;
    if (d.length < min_olap) d.flags |= MHAP_RD_SKIP;                 // SequenceSketchStreamer.java:129-133
    if (sc.raw[(size_t)r]) d.flags |= MHAP_RD_RAW;
    if (fwd_only) d.flags |= MHAP_RD_FWDONLY;
    d.base_off = store;
    if (!(d.flags & MHAP_RD_SKIP)) store += (d.flags & MHAP_RD_RAW) ? align4(d.length) : align4((d.length + 3) / 4);
    slot.ids[(size_t)i] = sc.ids[(size_t)r];
  }
  const size_t need = (size_t)std::max<int64_t>(store, 4);
  if (slot.cap < need) {
    if (slot.pin) (void)hipHostFree(slot.pin);
    slot.pin = nullptr; slot.cap = 0;
    if (hipHostMalloc((void**)&slot.pin, need + need / 8, hipHostMallocPortable) != hipSuccess) return false;
    slot.cap = need + need / 8;
  }
  slot.bytes = need;
  uint8_t* hs = slot.pin;
  parallel_chunks(n, nthreads, [&](int64_t a, int64_t b, int) {
    std::vector<uint8_t> tmp;
    for (int64_t i = a; i < b; i++) {
      const ReadDesc& d = slot.descs[(size_t)i];
      if (d.flags & MHAP_RD_SKIP) continue;
      const int64_t r = idx[(size_t)(lo + i)];
      const uint8_t* s = (const uint8_t*)sc.D + sc.body[(size_t)r];
      const int L = d.length;
      if (!sc.oneline[(size_t)r]) {   // several sequence lines: joined in a thread-local buffer (stays in cache), then packed like a single line
        tmp.resize((size_t)L);
        const uint8_t* e = (const uint8_t*)sc.D + sc.end[(size_t)r];
        int w = 0;
        for (const uint8_t* p = s; p < e; p++) { const uint8_t c = *p; if (c != '\n' && c != '\r') tmp[(size_t)w++] = c; }
        s = tmp.data();
      } else {
        while (*s == '\n' || *s == '\r') s++;   // (the line break that ends the header line)
      }
      uint8_t* dst = hs + d.base_off;
      if (d.flags & MHAP_RD_RAW) {
        for (int j = 0; j < L; j++) dst[j] = upper(s[j]);
        for (int j = L; j < (int)align4(L); j++) dst[j] = 0;
      } else pack_bases(s, L, dst);
    }
  });
  return true;
}

}  // namespace

namespace mhap {

// groups of <= group_bases bases (and <= 2^21 reads) over the subset start, start + stride, ...; for each group `consume(slot)` runs on
// the calling thread while a producer thread packs the next group into the other slot
// on_plan(groups): called once before anything is consumed, also for an empty subset (a collective caller agrees with its peers there)
int ingest_pipeline(const FastaScanImpl& sc, int64_t start, int64_t stride, int min_olap, bool fwd_only,
                    const std::function<int(Slot&)>& consume, std::string& err, const std::function<int(size_t)>& on_plan = nullptr) {
  std::vector<int64_t> idx;
  const int64_t nrec = (int64_t)sc.len.size();
  for (int64_t r = start; r < nrec; r += stride) idx.push_back(r);
  if (idx.empty()) return on_plan ? on_plan(0) : MHAP_OK;
  int64_t group_bases = 256LL << 20;
  if (const char* e = getenv("MHAP_INGEST_GROUP_BASES")) { const long long v = atoll(e); if (v > 0) group_bases = v; }
  // a quarter-size first group lets the GPU start early; after it the packing (15 GB/s on 16 threads) stays ahead of the kernels
  // (9 Gbase/s) and every launch is large enough to fill the GPU.  Measured at C2 (1 Gbase): ramped groups of 16..128 Mbase 159 ms
  // for 108 ms of kernels — small launches pay their fixed costs —, this scheme see profiles/r03_e2e_probe.txt
  std::vector<std::pair<int64_t, int64_t>> groups;
  for (int64_t lo = 0; lo < (int64_t)idx.size();) {
    const int64_t cap = groups.empty() ? std::max<int64_t>(group_bases >> 2, 1 << 20) : group_bases;
    int64_t hi = lo, tot = 0;
    while (hi < (int64_t)idx.size() && (hi == lo || tot + sc.len[(size_t)idx[(size_t)hi]] <= cap) && hi - lo < (1 << 21)) { tot += sc.len[(size_t)idx[(size_t)hi]]; hi++; }
    groups.emplace_back(lo, hi);
    lo = hi;
  }
  if (on_plan) { const int rp = on_plan(groups.size()); if (rp != MHAP_OK) return rp; }
  Slot slots[2];
  std::mutex mu; std::condition_variable cv;
  bool failed = false;
  const int nthreads = host_threads();
  std::thread producer([&]() {
    for (size_t g = 0; g < groups.size(); g++) {
      Slot& s = slots[g & 1];
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return !s.ready || failed; }); if (failed) return; }
      const double t0 = now_s();
      const bool ok = pack_group(sc, idx, groups[g].first, groups[g].second, min_olap, fwd_only, s, nthreads);
      if (prof()) fprintf(stderr, "[ingest] group %zu packed: %lld reads, %.1f MB, %.3f s (at %.3f)\n", g, (long long)(groups[g].second - groups[g].first), s.bytes / 1e6, now_s() - t0, now_s());
      { std::lock_guard<std::mutex> lk(mu); if (!ok) failed = true; s.ready = true; s.last = g + 1 == groups.size(); }
      cv.notify_all();
      if (!ok) return;
    }
  });
  int rc = MHAP_OK;
  for (size_t g = 0; g < groups.size(); g++) {
    Slot& s = slots[g & 1];
    { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&]() { return s.ready || failed; }); }
    if (failed) { rc = MHAP_E_NOMEM; err = "cannot allocate pinned staging memory"; break; }
    const double t0 = now_s();
    rc = consume(s);
    if (prof()) fprintf(stderr, "[ingest] group %zu consumed in %.3f s (at %.3f)\n", g, now_s() - t0, now_s());
    { std::lock_guard<std::mutex> lk(mu); s.ready = false; if (rc != MHAP_OK) failed = true; }
    cv.notify_all();
    if (rc != MHAP_OK) break;
  }
  { std::lock_guard<std::mutex> lk(mu); if (rc != MHAP_OK) failed = true; }
  cv.notify_all();
  producer.join();
  for (Slot& s : slots) if (s.pin) (void)hipHostFree(s.pin);
  return rc;
}

const FastaScanImpl* scan_impl(const mhap_fasta_scan* s) { return &s->impl; }

int ingest_add_subset(mhap_handle* h, const FastaScanImpl* scan, int64_t start, int64_t stride) {
  HandleView v = handle_view(h);
  (void)hipSetDevice(v.device);
  std::string err;
  // Under the eager exchange every add is a rendezvous of the ranks, and a rank's share may split into a different number of ingest groups
  // than another's: the ranks agree on the plan FIRST — one rendezvous per call of this function whatever the group counts —
  // and keep the eager exchange only when every rank adds exactly one group; otherwise it is suspended on all of them for this ingest
  // (the exchange then happens at search time) and no add makes a rendezvous.
  const int rc = ingest_pipeline(*scan, start, stride, v.min_olap_length, false, [&](Slot& s) {
    int r = internal_stage_packed(h, s.descs.data(), s.ids.data(), (int64_t)s.descs.size(), s.pin, s.bytes);
    if (r == MHAP_OK) r = mhap_index_add_staged(h);
    return r;
  }, err, [&](size_t ngroups) { const int r = dist_ingest_scope(h, (int64_t)ngroups); return r < 0 ? r : MHAP_OK; });
  dist_ingest_scope_end(h);
  if (rc != MHAP_OK && !err.empty()) *v.err = err;
  return rc;
}

}  // namespace mhap

extern "C" {

int mhap_fasta_scan_open(const char* path, int64_t id_offset, mhap_fasta_scan** out, char* errbuf, size_t errcap) {
  auto seterr = [&](const std::string& m) { if (errbuf && errcap) snprintf(errbuf, errcap, "%s", m.c_str()); };
  if (!path || !out) { seterr("null argument"); return MHAP_E_INVALID; }
  const double t0 = now_s();
  mhap_fasta_scan* S = new mhap_fasta_scan();
  FastaScanImpl& sc = S->impl;
  // Utils.getFile (J/utils/Utils.java:228-266): *bz2 -> bzip2, *gz -> gzip, otherwise the name must carry a FASTA suffix
  const std::string name(path);
  auto ends = [&](const char* suf) { const size_t n = strlen(suf); return name.size() >= n && name.compare(name.size() - n, n, suf) == 0; };
  if (ends("bz2") || ends("gz")) {
    std::string e;
    if (!inflate_file(name, sc.owned, e)) { seterr(e); delete S; return MHAP_E_INVALID; }
    sc.D = sc.owned.data(); sc.N = sc.owned.size();
  } else {
    static const char* suffixes[] = {"fna", "contigs", "contig", "final", "fasta", "fa", "fastq", "fq"};   // FastaData.java:50, and FASTQ's
    bool ok = false;
    for (const char* suf : suffixes) ok = ok || ends(suf);
    if (!ok) { seterr(std::string("Unknown file format of file ") + path + "."); delete S; return MHAP_E_INVALID; }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { seterr(std::string("cannot open ") + path); delete S; return MHAP_E_INVALID; }
    struct stat sb;
    if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
      void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);   // (no MAP_POPULATE: the scan threads fault their own parts in)
      if (m != MAP_FAILED) { sc.map_base = m; sc.map_len = (size_t)sb.st_size; (void)madvise(m, sc.map_len, MADV_WILLNEED); }
    }
    if (!sc.map_base) {   // pipes, empty files, mmap refused: read it
      char buf[1 << 16]; ssize_t got;
      while ((got = read(fd, buf, sizeof buf)) > 0) sc.owned.append(buf, (size_t)got);
      sc.D = sc.owned.data(); sc.N = sc.owned.size();
    } else { sc.D = (const char*)sc.map_base; sc.N = sc.map_len; }
    close(fd);
  }
  const char* D = sc.D; const size_t N = sc.N;
  // a first byte '@': FASTQ.  Its records come from fastq_host.hpp's sequential pass over the lines (the same on any number of host
  // threads); pass 2 below then reads a record's sequence lines, which end at its '+' line, as it reads a FASTA record's
  sc.fastq = N > 0 && D[0] == '@';
  std::vector<FastqRec> fq;
  if (sc.fastq) {
    std::string e;
    if (!fastq_records(D, N, fq, e)) { seterr(e); delete S; return MHAP_E_INVALID; }
  }
  if (N > 0 && D[0] != '>' && !sc.fastq) { seterr("Next sequence does not start with >. Invalid format."); delete S; return MHAP_E_INVALID; }   // FastaData.java:150-151
  // pass 1 (parallel over the text): the '>' that open records (BufferedReader.readLine: a line ends at \n, \r or \r\n)
  const int nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), (int64_t)(N >> 22) + 1));   // >= 4 MB of text per thread
  std::vector<std::vector<uint64_t>> found((size_t)nthreads);
  parallel_chunks(sc.fastq ? 0 : (int64_t)N, nthreads, [&](int64_t lo, int64_t hi, int t) {
    std::vector<uint64_t>& v = found[(size_t)t];
    for (const char* q = D + lo; q < D + hi;) {
      const char* g = (const char*)memchr(q, '>', (size_t)(D + hi - q));
      if (!g) break;
      if (g == D || g[-1] == '\n' || g[-1] == '\r') v.push_back((uint64_t)(g - D));
      q = g + 1;
    }
  });
  std::vector<uint64_t> hdr;
  for (auto& v : found) hdr.insert(hdr.end(), v.begin(), v.end());
  for (const FastqRec& r : fq) hdr.push_back(r.hdr);
  const int64_t nrec = (int64_t)hdr.size();
  // pass 2 (parallel over records): header line, bases, is-it-ACGT, is-it-one-line
  std::vector<uint64_t> body((size_t)nrec), rend((size_t)nrec);
  std::vector<int64_t> rlen((size_t)nrec);
  std::vector<uint8_t> rraw((size_t)nrec), rone((size_t)nrec);
  parallel_chunks(nrec, host_threads(), [&](int64_t lo, int64_t hi, int) {
    for (int64_t r = lo; r < hi; r++) {
      const size_t e = sc.fastq ? (size_t)fq[(size_t)r].seq_end : (r + 1 < nrec) ? (size_t)hdr[(size_t)r + 1] : N;
      size_t p = (size_t)hdr[(size_t)r];
      const char* nl = (const char*)memchr(D + p, '\n', e - p);
      const char* cr = (const char*)memchr(D + p, '\r', nl ? (size_t)(nl - (D + p)) : e - p);
      p = cr ? (size_t)(cr - D) : (nl ? (size_t)(nl - D) : e);
      body[(size_t)r] = p; rend[(size_t)r] = e;
      int64_t breaks = 0; uint32_t bad = 0;
      const uint8_t* s = (const uint8_t*)D;
      for (size_t i = p; i < e; i++) {
        const uint8_t c = s[i];
        const uint32_t isnl = (c == '\n' || c == '\r') ? 1u : 0u;
        breaks += isnl;
        bad |= (isnl | (is_base(c) ? 1u : 0u)) ^ 1u;
      }
      rlen[(size_t)r] = (int64_t)(e - p) - breaks;
      rraw[(size_t)r] = (uint8_t)bad;
      // one line: every line break sits at the two ends of the body
      size_t a = p, b = e;
      while (a < b && (s[a] == '\n' || s[a] == '\r')) a++;
      while (b > a && (s[b - 1] == '\n' || s[b - 1] == '\r')) b--;
      rone[(size_t)r] = (int64_t)(b - a) == rlen[(size_t)r] ? 1 : 0;
    }
  });
  int64_t count = 0;
  for (int64_t r = 0; r < nrec; r++) {
    if (rlen[(size_t)r] <= 0) continue;          // ids count non-empty records only, 1-based (FastaData.java:180-181)
    if (rlen[(size_t)r] > INT32_MAX) { seterr("sequence longer than 2^31-1"); delete S; return MHAP_E_INVALID; }
    count++;
    sc.hdr.push_back(hdr[(size_t)r]); sc.body.push_back(body[(size_t)r]); sc.end.push_back(rend[(size_t)r]);
    sc.len.push_back((int32_t)rlen[(size_t)r]); sc.raw.push_back(rraw[(size_t)r]); sc.oneline.push_back(rone[(size_t)r]);
    sc.ids.push_back(count + id_offset);
    sc.total_bases += rlen[(size_t)r];
    if (sc.fastq) { sc.qual.push_back(fq[(size_t)r].qual); sc.qual_end.push_back(fq[(size_t)r].qual_end); }
  }
  if (prof()) fprintf(stderr, "[ingest] scan of %s: %lld reads, %.1f Mbase, %.3f s on %d threads\n", path, (long long)count, sc.total_bases / 1e6, now_s() - t0, host_threads());
  *out = S;
  return MHAP_OK;
}

void mhap_fasta_scan_free(mhap_fasta_scan* s) { delete s; }
int64_t mhap_fasta_scan_reads(const mhap_fasta_scan* s) { return s ? (int64_t)s->impl.len.size() : 0; }
int64_t mhap_fasta_scan_bases(const mhap_fasta_scan* s) { return s ? s->impl.total_bases : 0; }

int mhap_fasta_scan_has_qualities(const mhap_fasta_scan* s) { return s && s->impl.fastq ? 1 : 0; }

int mhap_fasta_scan_qualities(const mhap_fasta_scan* s, uint8_t* qualities) {
  if (!s || !s->impl.fastq || (!qualities && s->impl.total_bases > 0)) return MHAP_E_INVALID;
  const FastaScanImpl& sc = s->impl;
  std::vector<int64_t> at(sc.len.size() + 1, 0);
  for (size_t r = 0; r < sc.len.size(); r++) at[r + 1] = at[r] + sc.len[r];
  parallel_chunks((int64_t)sc.len.size(), host_threads(), [&](int64_t lo, int64_t hi, int) {
    for (int64_t r = lo; r < hi; r++) {
      FastqRec rec{};
      rec.qual = sc.qual[(size_t)r]; rec.qual_end = sc.qual_end[(size_t)r]; rec.len = sc.len[(size_t)r];
      fastq_copy_qualities(sc.D, rec, qualities + at[(size_t)r]);
    }
  });
  return MHAP_OK;
}

int mhap_fasta_scan_info(mhap_fasta_scan* s, int64_t* ids, int32_t* lengths, const char** headers, int64_t* headers_bytes) {
  if (!s) return MHAP_E_INVALID;
  FastaScanImpl& sc = s->impl;
  const size_t n = sc.len.size();
  if (ids && n) memcpy(ids, sc.ids.data(), n * 8);
  if (lengths && n) memcpy(lengths, sc.len.data(), n * 4);
  if (headers || headers_bytes) {
    if (!sc.names_done) {   // substring(1).split("[\\s,]+", 2)[0] (FastaData.java:155-156)
      for (size_t r = 0; r < n; r++) {
        size_t a = (size_t)sc.hdr[r] + 1, e = a;
        while (e < (size_t)sc.body[r] && !(isspace((unsigned char)sc.D[e]) || sc.D[e] == ',')) e++;
        sc.names.append(sc.D + a, e - a);
        sc.names.push_back('\0');
      }
      sc.names_done = true;
    }
    if (headers) *headers = sc.names.data();
    if (headers_bytes) *headers_bytes = (int64_t)sc.names.size();
  }
  return MHAP_OK;
}

int mhap_index_add_scan(mhap_handle* h, const mhap_fasta_scan* s) {
  if (!h || !s) return MHAP_E_INVALID;
  int64_t entries = 0;
  (void)mhap_index_size(h, &entries);
  if (entries == 0) { const int rc = mhap_index_reserve(h, (int64_t)s->impl.len.size()); if (rc != MHAP_OK) return rc; }
  return ingest_add_subset(h, &s->impl, 0, 1);
}

int mhap_find_matches_scan(mhap_handle* h, const mhap_fasta_scan* s, mhap_record_sink sink, void* user) {
  if (!h || !s) return MHAP_E_INVALID;
  // -q mode: groups of query reads; the library's entry point takes one byte per base, so a group's text is joined here (queries are
  // a small share of a run)
  const FastaScanImpl& sc = s->impl;
  const int64_t n = (int64_t)sc.len.size();
  const int64_t group_bases = 256LL << 20;
  for (int64_t lo = 0; lo < n;) {
    int64_t hi = lo, tot = 0;
    while (hi < n && (hi == lo || tot + sc.len[(size_t)hi] <= group_bases)) { tot += sc.len[(size_t)hi]; hi++; }
    std::vector<char> bases((size_t)std::max<int64_t>(tot, 1));
    std::vector<int64_t> offs((size_t)(hi - lo));
    int64_t at = 0;
    for (int64_t r = lo; r < hi; r++) { offs[(size_t)(r - lo)] = at; at += sc.len[(size_t)r]; }
    parallel_chunks(hi - lo, host_threads(), [&](int64_t a, int64_t b, int) {
      for (int64_t i = a; i < b; i++) {
        const int64_t r = lo + i;
        char* w = bases.data() + offs[(size_t)i];
        for (size_t p = (size_t)sc.body[(size_t)r]; p < (size_t)sc.end[(size_t)r]; p++) { const char c = sc.D[p]; if (c != '\n' && c != '\r') *w++ = (char)upper((uint8_t)c); }
      }
    });
    const int rc = mhap_find_matches_reads(h, bases.data(), offs.data(), sc.len.data() + lo, sc.ids.data() + lo, hi - lo, sink, user);
    if (rc != MHAP_OK) return rc;
    lo = hi;
  }
  return MHAP_OK;
}

}  // extern "C"

// ---- exact k-mer counting: the C ABI (kernels and their driver: kmer_kernels.hip) ---------------------------------------------
struct mhap_kmer_set { KmerSet set; };
struct mhap_kmer_eval { KmerEval eval; };
struct mhap_kmer_counts {
  int32_t k = 0;
  int64_t total = 0, distinct = 0;
  std::vector<uint32_t> values, counts;   // the lines, in file order
  bool has_histogram = false;
  KmerHistogram histogram;                // (when asked for at finish)
};

namespace {

// the open count of h, or null with the reason in h's error (a count that an index call interrupted is closed here)
KmerCountState* kc_state(const HandleView& v, const char* what, int& rc) {
  KmerCountState* S = (KmerCountState*)*v.kmer;
  rc = MHAP_OK;
  if (!S) { *v.err = std::string(what) + ": no k-mer count is open on this handle (mhap_kmer_count_begin starts one)"; rc = MHAP_E_STATE; return nullptr; }
  if (kmer_count_index_gen(*S) != v.index_gen) {
    *v.err = std::string(what) + ": the index changed while a k-mer count was open; the count is closed (begin it again)";
    kmer_count_release(S); *v.kmer = nullptr; rc = MHAP_E_STATE; return nullptr;
  }
  return S;
}
// a failed add or finish closes the count: its state is partial
int kc_close_on_error(const HandleView& v, int rc) {
  if (rc != MHAP_OK && *v.kmer) { kmer_count_release((KmerCountState*)*v.kmer); *v.kmer = nullptr; }
  return rc;
}
inline bool is_upper_base(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// reads given as bytes, in groups of <= 256 Mbase (and <= 2^21 reads), packed like the ingest packs them: 2 bits per base when every
// byte is A/C/G/T, else the bytes as they are; each group goes to consume(descs, reads, packed, bytes), whose first error ends the walk
int pack_read_groups(const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n,
                     const std::function<int(const ReadDesc*, int64_t, const void*, size_t)>& consume) {
  const int nthreads = host_threads();
  std::vector<ReadDesc> descs;
  std::vector<uint8_t> packed;
  for (int64_t lo = 0; lo < n;) {
    int64_t hi = lo, tot = 0;
    while (hi < n && (hi == lo || tot + lengths[hi] <= (256LL << 20)) && hi - lo < (1 << 21)) { tot += lengths[hi]; hi++; }
    descs.assign((size_t)(hi - lo), ReadDesc{});
    std::vector<uint8_t> raw((size_t)(hi - lo));
    parallel_chunks(hi - lo, nthreads, [&](int64_t a, int64_t b, int) {
      for (int64_t i = a; i < b; i++) {
        const uint8_t* s = (const uint8_t*)bases + offsets[lo + i];
        bool pure = true;
        for (int j = 0; j < lengths[lo + i] && pure; j++) pure = is_upper_base(s[j]);
        raw[(size_t)i] = pure ? 0 : 1;
      }
    });
    int64_t store = 0;
    for (int64_t i = 0; i < hi - lo; i++) {
      ReadDesc& d = descs[(size_t)i];
      d.length = lengths[lo + i];
      d.flags = raw[(size_t)i] ? MHAP_RD_RAW : 0;
      d.base_off = store;
      store += raw[(size_t)i] ? align4(d.length) : align4((d.length + 3) / 4);
    }
    packed.assign((size_t)std::max<int64_t>(store, 4), 0);
    parallel_chunks(hi - lo, nthreads, [&](int64_t a, int64_t b, int) {
      for (int64_t i = a; i < b; i++) {
        const ReadDesc& d = descs[(size_t)i];
        const uint8_t* s = (const uint8_t*)bases + offsets[lo + i];
        if (d.flags & MHAP_RD_RAW) memcpy(packed.data() + d.base_off, s, (size_t)d.length);
        else pack_bases(s, d.length, packed.data() + d.base_off);
      }
    });
    const int rc = consume(descs.data(), hi - lo, packed.data(), (size_t)store);
    if (rc != MHAP_OK) return rc;
    lo = hi;
  }
  return MHAP_OK;
}

}  // namespace

extern "C" {

int mhap_kmer_count_begin(mhap_handle* h, int32_t k, int32_t canonical) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (k < 1 || k > 16) { *v.err = "k-mer counting supports k from 1 to 16 (got " + std::to_string(k) + ")"; return MHAP_E_INVALID; }
  if (*v.kmer) { *v.err = "mhap_kmer_count_begin: a k-mer count is already open on this handle (mhap_kmer_count_finish ends it)"; return MHAP_E_STATE; }
  KmerCountState* S = nullptr;
  const int rc = kmer_count_begin(S, v, k, canonical);
  if (rc == MHAP_OK) *v.kmer = S;
  return rc;
}

int mhap_kmer_count_add_reads(mhap_handle* h, const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  int rc;
  KmerCountState* S = kc_state(v, "mhap_kmer_count_add_reads", rc);
  if (!S) return rc;
  if (n < 0 || (n > 0 && (!bases || !offsets || !lengths))) { *v.err = "mhap_kmer_count_add_reads: null argument"; return MHAP_E_INVALID; }
  for (int64_t i = 0; i < n; i++) if (lengths[i] < 0 || offsets[i] < 0) { *v.err = "mhap_kmer_count_add_reads: negative read length or offset"; return MHAP_E_INVALID; }
  rc = pack_read_groups(bases, offsets, lengths, n, [&](const ReadDesc* descs, int64_t count, const void* packed, size_t bytes) {
    return kmer_count_add_group(*S, v, descs, count, packed, bytes);
  });
  return kc_close_on_error(v, rc);
}

int mhap_kmer_count_add_scan(mhap_handle* h, const mhap_fasta_scan* s) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  int rc;
  KmerCountState* S = kc_state(v, "mhap_kmer_count_add_scan", rc);
  if (!S) return rc;
  if (!s) { *v.err = "mhap_kmer_count_add_scan: null scan"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  const FastaScanImpl& sc = s->impl;
  uint64_t windows = 0;
  for (int32_t L : sc.len) windows += (uint64_t)std::max(0, L - kmer_count_k(*S) + 1);
  rc = kmer_count_reserve(*S, v, std::min(windows, kmer_count_budget(*S)));   // the staging arena at its size for this file (up to the flush budget) at once
  if (rc != MHAP_OK) return kc_close_on_error(v, rc);
  std::string err;
  // min_olap 0: reads below --min-olap-length are counted too (the counter never skips a read)
  rc = ingest_pipeline(sc, 0, 1, 0, false, [&](Slot& sl) {
    return kmer_count_add_group(*S, v, sl.descs.data(), (int64_t)sl.descs.size(), sl.pin, sl.bytes);
  }, err);
  if (rc != MHAP_OK && !err.empty()) *v.err = err;
  return kc_close_on_error(v, rc);
}

int mhap_kmer_count_finish(mhap_handle* h, double min_fraction, mhap_kmer_counts** out) {
  return mhap_kmer_count_finish_flags(h, min_fraction, 0, out);
}

int mhap_kmer_count_finish_flags(mhap_handle* h, double min_fraction, uint32_t flags, mhap_kmer_counts** out) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  int rc;
  KmerCountState* S = kc_state(v, "mhap_kmer_count_finish", rc);
  if (!S) return rc;
  if (!out) { *v.err = "mhap_kmer_count_finish: null output"; return MHAP_E_INVALID; }
  if (!(min_fraction == min_fraction)) { *v.err = "mhap_kmer_count_finish: min_fraction is NaN"; return MHAP_E_INVALID; }
  if (flags & ~(uint32_t)(MHAP_KMER_HISTOGRAM | MHAP_KMER_KEEP_OPEN)) { *v.err = "mhap_kmer_count_finish_flags: unknown flags " + std::to_string(flags); return MHAP_E_INVALID; }
  mhap_kmer_counts* c = new mhap_kmer_counts();
  c->has_histogram = (flags & MHAP_KMER_HISTOGRAM) != 0;
  rc = kmer_count_finish(*S, v, min_fraction, c->values, c->counts, c->distinct, c->has_histogram ? &c->histogram : nullptr);
  c->k = kmer_count_k(*S);
  c->total = kmer_count_total(*S);
  if (rc != MHAP_OK || !(flags & MHAP_KMER_KEEP_OPEN)) { kmer_count_release(S); *v.kmer = nullptr; }
  if (rc != MHAP_OK) { delete c; return rc; }
  *out = c;
  return MHAP_OK;
}

int mhap_kmer_counts_info(const mhap_kmer_counts* c, int64_t* total, int64_t* distinct, int64_t* lines, int32_t* k) {
  if (!c) return MHAP_E_INVALID;
  if (total) *total = c->total;
  if (distinct) *distinct = c->distinct;
  if (lines) *lines = (int64_t)c->values.size();
  if (k) *k = c->k;
  return MHAP_OK;
}

int mhap_kmer_counts_lines(const mhap_kmer_counts* c, uint64_t* kmers, uint64_t* counts) {
  if (!c) return MHAP_E_INVALID;
  for (size_t i = 0; i < c->values.size(); i++) {
    if (kmers) kmers[i] = c->values[i];
    if (counts) counts[i] = c->counts[i];
  }
  return MHAP_OK;
}

int mhap_kmer_counts_write(const mhap_kmer_counts* c, const char* path) {
  if (!c || !path) return MHAP_E_INVALID;
  FILE* f = fopen(path, "w");
  if (!f) return MHAP_E_IO;
  std::vector<char> buf(1 << 20);
  setvbuf(f, buf.data(), _IOFBF, buf.size());
  bool ok = fprintf(f, "%lld %lld\n", (long long)c->distinct, (long long)c->values.size()) > 0;
  char km[17];
  const double T = (double)c->total;
  for (size_t i = 0; i < c->values.size() && ok; i++) {
    for (int j = 0; j < c->k; j++) km[j] = "ACGT"[(c->values[i] >> (2 * (c->k - 1 - j))) & 3u];
    km[c->k] = 0;
    ok = fprintf(f, "%s\t%.10e\n", km, (double)c->counts[i] / T) > 0;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? MHAP_OK : MHAP_E_IO;
}

int mhap_kmer_counts_histogram_size(const mhap_kmer_counts* c, int64_t* n) {
  if (!c || !n) return MHAP_E_INVALID;
  *n = c->has_histogram ? (int64_t)c->histogram.counts.size() : 0;
  return c->has_histogram ? MHAP_OK : MHAP_E_STATE;
}

int mhap_kmer_counts_histogram(const mhap_kmer_counts* c, uint32_t* counts, uint64_t* numbers) {
  if (!c) return MHAP_E_INVALID;
  if (!c->has_histogram) return MHAP_E_STATE;
  for (size_t i = 0; i < c->histogram.counts.size(); i++) {
    if (counts) counts[i] = c->histogram.counts[i];
    if (numbers) numbers[i] = c->histogram.numbers[i];
  }
  return MHAP_OK;
}

int mhap_kmer_counts_write_histogram(const mhap_kmer_counts* c, const char* path) {
  if (!c || !path) return MHAP_E_INVALID;
  if (!c->has_histogram) return MHAP_E_STATE;
  FILE* f = fopen(path, "w");
  if (!f) return MHAP_E_IO;
  std::vector<char> buf(1 << 20);
  setvbuf(f, buf.data(), _IOFBF, buf.size());
  bool ok = true;
  for (size_t i = 0; i < c->histogram.counts.size() && ok; i++)
    ok = fprintf(f, "%u\t%llu\n", (unsigned)c->histogram.counts[i], (unsigned long long)c->histogram.numbers[i]) > 0;
  ok = (fclose(f) == 0) && ok;
  return ok ? MHAP_OK : MHAP_E_IO;
}

void mhap_kmer_counts_free(mhap_kmer_counts* c) { delete c; }

// ---- sequence assessment: the set of the solid k-mers, sequences against it, set against set ----------------------------------------
int mhap_kmer_histogram_valley(const uint32_t* counts, const uint64_t* numbers, int64_t n, uint64_t* valley) {
  if (!valley || n < 0 || (n > 0 && (!counts || !numbers))) return MHAP_E_INVALID;
  for (int64_t i = 0; i < n; i++) if (counts[i] < 1 || (i > 0 && counts[i] <= counts[i - 1])) return MHAP_E_INVALID;
  // the smallest c >= 1 with n[c + 1] >= n[c]: a count that is absent (n[c] = 0) ends the walk, so it only steps over entries in a row
  uint64_t c = 1;
  for (int64_t i = 0; i < n && counts[i] == c && numbers[i] > 0; i++, c++) {
    const uint64_t next = i + 1 < n && counts[i + 1] == c + 1 ? numbers[i + 1] : 0;
    if (next >= numbers[i]) break;
  }
  *valley = c;
  return MHAP_OK;
}

int mhap_kmer_qv(int64_t windows, int64_t missing, int32_t k, double* error, double* qv) {
  if (windows < 0 || missing < 0 || missing > windows || k < 1) return MHAP_E_INVALID;
  double e, q;
  if (windows == 0) e = q = std::numeric_limits<double>::quiet_NaN();
  else if (missing == 0) { e = 0.0; q = std::numeric_limits<double>::infinity(); }
  else {
    e = 1.0 - std::pow(1.0 - (double)missing / (double)windows, 1.0 / (double)k);
    q = 0.0 - 10.0 * std::log10(e);   // (0.0 -: an error of 1 gives +0)
  }
  if (error) *error = e;
  if (qv) *qv = q;
  return MHAP_OK;
}

int mhap_kmer_count_finish_set(mhap_handle* h, uint64_t min_count, mhap_kmer_set** out) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  int rc;
  KmerCountState* S = kc_state(v, "mhap_kmer_count_finish_set", rc);
  if (!S) return rc;
  if (!out) { *v.err = "mhap_kmer_count_finish_set: null output"; return MHAP_E_INVALID; }
  if (min_count == 0) {   // the valley of the count histogram: the histogram finish reads the open state and leaves it as it is
    std::vector<uint32_t> values, counts;
    int64_t distinct = 0;
    KmerHistogram hist;
    rc = kmer_count_finish(*S, v, 2.0, values, counts, distinct, &hist);   // (a fraction above 1: no lines)
    if (rc == MHAP_OK) rc = mhap_kmer_histogram_valley(hist.counts.data(), hist.numbers.data(), (int64_t)hist.counts.size(), &min_count);
  }
  mhap_kmer_set* s = new mhap_kmer_set();
  if (rc == MHAP_OK) rc = kmer_count_finish_set(*S, v, min_count, s->set);
  kmer_count_release(S); *v.kmer = nullptr;
  if (rc != MHAP_OK) { kmer_set_release(s->set); delete s; return rc; }
  *out = s;
  return MHAP_OK;
}

void mhap_kmer_set_free(mhap_kmer_set* s) {
  if (!s) return;
  kmer_set_release(s->set);
  delete s;
}

int mhap_kmer_set_info(const mhap_kmer_set* s, int64_t* total, int64_t* distinct, int64_t* members, int32_t* k, int32_t* canonical, uint64_t* min_count) {
  if (!s) return MHAP_E_INVALID;
  if (total) *total = s->set.total;
  if (distinct) *distinct = s->set.distinct;
  if (members) *members = s->set.members;
  if (k) *k = s->set.k;
  if (canonical) *canonical = s->set.canonical;
  if (min_count) *min_count = s->set.min_count;
  return MHAP_OK;
}

}  // extern "C"

namespace {
// the set as an entry point may use it: made on the handle's device
bool ks_usable(const HandleView& v, const mhap_kmer_set* s, const char* who) {
  if (!s || !s->set.bits) { *v.err = std::string(who) + ": null set"; return false; }
  if (s->set.device != v.device) { *v.err = std::string(who) + ": the set was made on device " + std::to_string(s->set.device) + ", the handle is on " + std::to_string(v.device); return false; }
  return true;
}
}  // namespace

extern "C" {

int mhap_kmer_set_contains(mhap_handle* h, const mhap_kmer_set* s, const uint64_t* values, int64_t n, uint8_t* out) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!ks_usable(v, s, "mhap_kmer_set_contains")) return MHAP_E_INVALID;
  if (n < 0 || (n > 0 && (!values || !out))) { *v.err = "mhap_kmer_set_contains: null argument"; return MHAP_E_INVALID; }
  return kmer_set_contains(v, s->set, values, n, out);
}

int mhap_kmer_set_compare(mhap_handle* h, const mhap_kmer_set* a, const mhap_kmer_set* b, int64_t* a_members, int64_t* b_members, int64_t* both) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!ks_usable(v, a, "mhap_kmer_set_compare") || !ks_usable(v, b, "mhap_kmer_set_compare")) return MHAP_E_INVALID;
  if (a->set.k != b->set.k || a->set.canonical != b->set.canonical) {
    *v.err = "mhap_kmer_set_compare: the sets differ in k or in canonical (" + std::to_string(a->set.k) + "/" + std::to_string(a->set.canonical) + " against " +
             std::to_string(b->set.k) + "/" + std::to_string(b->set.canonical) + ")";
    return MHAP_E_INVALID;
  }
  int64_t c[3] = {0, 0, 0};
  const int rc = kmer_set_compare(v, a->set, b->set, c);
  if (rc != MHAP_OK) return rc;
  if (a_members) *a_members = c[0];
  if (b_members) *b_members = c[1];
  if (both) *both = c[2];
  return MHAP_OK;
}

int mhap_kmer_eval_reads(mhap_handle* h, const mhap_kmer_set* s, const char* bases, const int64_t* offsets, const int32_t* lengths, int64_t n, mhap_kmer_eval** out) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!ks_usable(v, s, "mhap_kmer_eval_reads")) return MHAP_E_INVALID;
  if (!out || n < 0 || (n > 0 && (!bases || !offsets || !lengths))) { *v.err = "mhap_kmer_eval_reads: null argument"; return MHAP_E_INVALID; }
  for (int64_t i = 0; i < n; i++) if (lengths[i] < 0 || offsets[i] < 0) { *v.err = "mhap_kmer_eval_reads: negative sequence length or offset"; return MHAP_E_INVALID; }
  mhap_kmer_eval* e = new mhap_kmer_eval();
  e->eval.k = s->set.k;
  const int rc = pack_read_groups(bases, offsets, lengths, n, [&](const ReadDesc* descs, int64_t count, const void* packed, size_t bytes) {
    return kmer_eval_group(v, s->set, descs, count, packed, bytes, e->eval);
  });
  kmer_eval_done(v, e->eval);
  if (rc != MHAP_OK) { delete e; return rc; }
  *out = e;
  return MHAP_OK;
}

int mhap_kmer_eval_scan(mhap_handle* h, const mhap_kmer_set* s, const mhap_fasta_scan* scan, mhap_kmer_eval** out) {
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!ks_usable(v, s, "mhap_kmer_eval_scan")) return MHAP_E_INVALID;
  if (!out || !scan) { *v.err = "mhap_kmer_eval_scan: null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  mhap_kmer_eval* e = new mhap_kmer_eval();
  e->eval.k = s->set.k;
  std::string err;
  const int rc = ingest_pipeline(scan->impl, 0, 1, 0, false, [&](Slot& sl) {
    return kmer_eval_group(v, s->set, sl.descs.data(), (int64_t)sl.descs.size(), sl.pin, sl.bytes, e->eval);
  }, err);
  kmer_eval_done(v, e->eval);
  if (rc != MHAP_OK) { if (!err.empty()) *v.err = err; delete e; return rc; }
  *out = e;
  return MHAP_OK;
}

void mhap_kmer_eval_free(mhap_kmer_eval* e) { delete e; }

int mhap_kmer_eval_info(const mhap_kmer_eval* e, int64_t* sequences, int64_t* intervals, int32_t* k, int64_t* totals) {
  if (!e) return MHAP_E_INVALID;
  const KmerEval& E = e->eval;
  if (sequences) *sequences = (int64_t)(E.rows.size() / 5);
  if (intervals) *intervals = (int64_t)(E.intervals.size() / 3);
  if (k) *k = E.k;
  if (totals) {
    for (int f = 0; f < 5; f++) totals[f] = 0;
    for (size_t i = 0; i < E.rows.size(); i++) totals[i % 5] += E.rows[i];
  }
  return MHAP_OK;
}

int mhap_kmer_eval_rows(const mhap_kmer_eval* e, int64_t* rows) {
  if (!e) return MHAP_E_INVALID;
  if (rows && !e->eval.rows.empty()) memcpy(rows, e->eval.rows.data(), e->eval.rows.size() * 8);
  return MHAP_OK;
}

int mhap_kmer_eval_intervals(const mhap_kmer_eval* e, int64_t* intervals) {
  if (!e) return MHAP_E_INVALID;
  if (intervals && !e->eval.intervals.empty()) memcpy(intervals, e->eval.intervals.data(), e->eval.intervals.size() * 8);
  return MHAP_OK;
}

}  // extern "C"

namespace {
// name i of `names` (NUL-terminated, back to back), or seq<i + 1> without names; `at` walks the names
std::string ke_name(const char*& at, int64_t i) {
  if (!at) return "seq" + std::to_string(i + 1);
  std::string s(at);
  at += s.size() + 1;
  return s;
}
bool ke_table_line(FILE* f, const std::string& name, const int64_t* r, int k) {
  double err = 0.0, qv = 0.0;
  (void)mhap_kmer_qv(r[1], r[2], k, &err, &qv);
  return fprintf(f, "%s\t%lld\t%lld\t%lld\t%lld\t%lld\t%.6e\t%.2f\n", name.c_str(), (long long)r[0], (long long)r[1], (long long)r[2], (long long)r[3],
                 (long long)r[4], err, qv) > 0;
}
}  // namespace

extern "C" {

int mhap_kmer_eval_write_table(const mhap_kmer_eval* e, const char* names, const char* path) {
  if (!e || !path) return MHAP_E_INVALID;
  FILE* f = fopen(path, "w");
  if (!f) return MHAP_E_IO;
  std::vector<char> buf(1 << 20);
  setvbuf(f, buf.data(), _IOFBF, buf.size());
  const KmerEval& E = e->eval;
  int64_t tot[5] = {0, 0, 0, 0, 0};
  bool ok = true;
  const char* at = names;
  for (size_t i = 0; i * 5 < E.rows.size() && ok; i++) {
    const int64_t* r = E.rows.data() + i * 5;
    for (int j = 0; j < 5; j++) tot[j] += r[j];
    ok = ke_table_line(f, ke_name(at, (int64_t)i), r, E.k);
  }
  ok = ok && ke_table_line(f, "total", tot, E.k);
  ok = (fclose(f) == 0) && ok;
  return ok ? MHAP_OK : MHAP_E_IO;
}

int mhap_kmer_eval_write_bed(const mhap_kmer_eval* e, const char* names, const char* path) {
  if (!e || !path) return MHAP_E_INVALID;
  FILE* f = fopen(path, "w");
  if (!f) return MHAP_E_IO;
  std::vector<char> buf(1 << 20);
  setvbuf(f, buf.data(), _IOFBF, buf.size());
  const KmerEval& E = e->eval;
  bool ok = true;
  const char* at = names;
  int64_t named = -1;   // the sequence `name` belongs to (intervals are in sequence order)
  std::string name;
  for (size_t i = 0; i * 3 < E.intervals.size() && ok; i++) {
    const int64_t* iv = E.intervals.data() + i * 3;
    while (named < iv[0]) name = ke_name(at, ++named);
    ok = fprintf(f, "%s\t%lld\t%lld\n", name.c_str(), (long long)iv[1], (long long)iv[2]) > 0;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? MHAP_OK : MHAP_E_IO;
}

int mhap_kmer_eval_summary(const mhap_kmer_eval* e, const mhap_kmer_set* reads, const mhap_kmer_set* own, int64_t both, char* line, size_t cap) {
  if (!e || !reads || !line || cap == 0) return MHAP_E_INVALID;
  int64_t n = 0, t[5];
  (void)mhap_kmer_eval_info(e, &n, nullptr, nullptr, t);
  double err = 0.0, qv = 0.0;
  (void)mhap_kmer_qv(t[1], t[2], e->eval.k, &err, &qv);
  std::string s(512, 0);
  int w = snprintf(&s[0], s.size(), "Assessed %lld sequences, %lld bases against %lld solid %d-mers (count >= %llu): %lld windows, %lld missing in %lld runs, "
                   "%lld unsupported bases, QV %.2f", (long long)n, (long long)t[0], (long long)reads->set.members, (int)reads->set.k,
                   (unsigned long long)reads->set.min_count, (long long)t[1], (long long)t[2], (long long)t[3], (long long)t[4], qv);
  s.resize((size_t)std::max(w, 0));
  if (own) {
    char c[160];
    const double comp = reads->set.members > 0 ? (double)both / (double)reads->set.members : std::numeric_limits<double>::quiet_NaN();
    snprintf(c, sizeof c, "; completeness %.6f (%lld of the solid %d-mers are among the sequences' %lld)", comp, (long long)both, (int)reads->set.k,
             (long long)own->set.members);
    s += c;
  }
  snprintf(line, cap, "%s", s.c_str());
  return MHAP_OK;
}

}  // extern "C"
