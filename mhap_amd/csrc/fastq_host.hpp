// fastq_host.hpp — the record grammar of FASTQ input ("FASTQ input" in include/mhap_hip.h), shared by mhap_fasta_read (host_util.cpp)
// and mhap_fasta_scan_open (mhap_ingest.hip).  No GPU and no HIP: tools/fastq_host_check.cpp runs fastq_host.cpp under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace mhap {

// One record of the text, empty ones included.  [body, seq_end) holds the sequence lines with their line ends, as the stretch between
// a FASTA header line and the next '>' does; the record's `len` quality bytes are the bytes of [qual, qual_end) that are no line end.
struct FastqRec {
  uint64_t hdr;        // the '@' that opens the record
  uint64_t body;       // the line end of the header line
  uint64_t seq_end;    // the '+' that opens the separator line
  uint64_t qual;       // the first byte after the separator line's line end
  uint64_t qual_end;   // one past the last quality byte
  int64_t len;         // bases = quality bytes
};

// The records of text[0, n), one sequential pass over its lines ('@' is no record marker inside qualities, so a parallel search for
// it would have to be checked by this pass anyway).  false with one line in err that names the record, counted from 1.
bool fastq_records(const char* text, size_t n, std::vector<FastqRec>& recs, std::string& err);

// the Phred values (byte - 33) of one record: r.len bytes to out
void fastq_copy_qualities(const char* text, const FastqRec& r, uint8_t* out);

}  // namespace mhap
