// fastq_host.cpp — the FASTQ record pass of both readers (fastq_host.hpp); the grammar is the "FASTQ input" paragraph of include/mhap_hip.h.
#include "fastq_host.hpp"

#include <string.h>

namespace mhap {
namespace {

inline bool is_eol(char c) { return c == '\n' || c == '\r'; }

// the end of the line that p lies on: the first \n or \r at or after p, or N.  Two memchr per window of 4 096 bytes, so that a text
// whose lines end with \r alone is not searched to its end for a \n from every line
inline size_t line_end(const char* D, size_t N, size_t p) {
  for (size_t a = p; a < N; a += 4096) {
    const size_t b = N - a < 4096 ? N : a + 4096;
    const char* nl = (const char*)memchr(D + a, '\n', b - a);
    const char* cr = (const char*)memchr(D + a, '\r', (nl ? (size_t)(nl - D) : b) - a);
    if (cr) return (size_t)(cr - D);
    if (nl) return (size_t)(nl - D);
  }
  return N;
}

}  // namespace

bool fastq_records(const char* D, size_t N, std::vector<FastqRec>& recs, std::string& err) {
  recs.clear();
  size_t p = 0;
  int64_t number = 0;   // of the record being read, counted from 1, empty records included
  auto fail = [&](const char* what) {
    err = "FASTQ record " + std::to_string(number) + " " + what;
    return false;
  };
  while (true) {
    while (p < N && is_eol(D[p])) p++;   // line ends between records
    if (p >= N) break;
    number++;
    if (D[p] != '@') return fail("does not start with @. Invalid format.");
    FastqRec r{};
    r.hdr = p;
    p = line_end(D, N, p);
    r.body = p;
    // sequence lines, up to the line that begins with '+'
    bool plus = false;
    while (p < N) {
      while (p < N && is_eol(D[p])) p++;
      if (p >= N) break;
      if (D[p] == '+') { plus = true; break; }
      if (D[p] == '@') break;   // the next record's header: this one has no qualities
      const size_t e = line_end(D, N, p);
      r.len += (int64_t)(e - p);
      p = e;
    }
    if (!plus) return fail("has no + line after its sequence.");
    r.seq_end = p;
    p = line_end(D, N, p);   // the rest of the + line is ignored
    if (p < N) p += (D[p] == '\r' && p + 1 < N && D[p + 1] == '\n') ? 2 : 1;
    r.qual = p;
    // quality lines, until as many bytes as the sequence has; any byte may open one of them
    int64_t got = 0;
    while (got < r.len) {
      while (p < N && is_eol(D[p])) p++;
      if (p >= N) return fail("is cut short: the file ends before its qualities are complete.");
      const size_t e = line_end(D, N, p);
      if ((int64_t)(e - p) > r.len - got) return fail("has a quality line that runs past its sequence.");
      unsigned bad = 0;   // (no branch in the loop: one pass over the line at the width the compiler finds)
      for (size_t i = p; i < e; i++) bad |= (unsigned)((unsigned char)D[i] - 33u > 93u);
      if (bad) return fail("has a quality byte outside 33 .. 126.");
      got += (int64_t)(e - p);
      p = e;
    }
    r.qual_end = p;
    recs.push_back(r);
  }
  return true;
}

void fastq_copy_qualities(const char* D, const FastqRec& r, uint8_t* out) {
  int64_t w = 0;
  for (uint64_t p = r.qual; p < r.qual_end && w < r.len; p++)
    if (!is_eol(D[p])) out[w++] = (uint8_t)((unsigned char)D[p] - 33);
}

}  // namespace mhap
