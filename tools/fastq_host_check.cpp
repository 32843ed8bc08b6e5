// fastq_host_check.cpp — the FASTQ record pass of both readers under the sanitizers, as a program of its own (no GPU, no HIP, nothing
// loaded into Python): fastq_records and fastq_copy_qualities (mhap_amd/csrc/fastq_host.cpp) over the files named on the command line
// and over every truncation of each, every text in a heap block of exactly its size so that a read past its end is caught.  From the
// repository's root:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/fastq_host_check.cpp mhap_amd/csrc/fastq_host.cpp -o fastq_host_check
//   ./fastq_host_check reads.fastq ...     (per file one line, "<path>: <records> records, <bases> bases, quality sum <sum>" or
//                                           "<path>: refused: <the parser's line>", then "fastq_host_check: ok"; exits 0)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../mhap_amd/csrc/fastq_host.hpp"

using namespace mhap;

namespace {

// parse text[0, n) from a block of exactly n bytes; the qualities go to blocks of exactly len bytes
bool parse_exact(const std::string& text, size_t n, int64_t* records, int64_t* bases, int64_t* qsum, std::string& err) {
  std::unique_ptr<char[]> block(new char[n ? n : 1]);
  memcpy(block.get(), text.data(), n);
  std::vector<FastqRec> recs;
  if (!fastq_records(block.get(), n, recs, err)) return false;
  *records = (int64_t)recs.size(); *bases = 0; *qsum = 0;
  for (const FastqRec& r : recs) {
    if (r.hdr > r.body || r.body > r.seq_end || r.seq_end > r.qual || r.qual > r.qual_end || r.qual_end > n || r.len < 0) {
      fprintf(stderr, "fastq_host_check: a record's offsets are out of order\n");
      exit(1);
    }
    std::unique_ptr<uint8_t[]> q(new uint8_t[r.len ? r.len : 1]);
    fastq_copy_qualities(block.get(), r, q.get());
    for (int64_t i = 0; i < r.len; i++) {
      if (q[i] > 93) { fprintf(stderr, "fastq_host_check: a Phred value above 93\n"); exit(1); }
      *qsum += q[i];
    }
    *bases += r.len;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    FILE* fh = fopen(argv[a], "rb");
    if (!fh) { fprintf(stderr, "fastq_host_check: cannot open %s\n", argv[a]); return 1; }
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fh)) > 0) text.append(buf, got);
    fclose(fh);
    int64_t records = 0, bases = 0, qsum = 0;
    std::string err;
    for (size_t n = 0; n < text.size(); n++) {   // every truncation: accepted or refused, never read past
      std::string e;
      if (!parse_exact(text, n, &records, &bases, &qsum, e) && e.find("FASTQ record ") != 0) {
        fprintf(stderr, "fastq_host_check: %s cut at %zu: a refusal that names no record: %s\n", argv[a], n, e.c_str());
        return 1;
      }
    }
    if (parse_exact(text, text.size(), &records, &bases, &qsum, err))
      printf("%s: %lld records, %lld bases, quality sum %lld\n", argv[a], (long long)records, (long long)bases, (long long)qsum);
    else
      printf("%s: refused: %s\n", argv[a], err.c_str());
  }
  printf("fastq_host_check: ok\n");
  return 0;
}
