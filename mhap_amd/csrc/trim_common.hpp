// trim_common.hpp — the rules of "read trimming" (include/mhap_hip.h) that host and device share, written once: which records count,
// the interval a record contributes to a read, and a record rewritten onto the trimmed reads.  add_kernel and apply_kernel
// (trim_kernels.hip) and mhap_trim_clip_record (host, no GPU) all go through these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mhap {

enum { TRIM_DELETED = 1, TRIM_CUT5 = 2, TRIM_CUT3 = 4, TRIM_GAPPED = 8 };

struct TParams { int32_t min_cov, end_clip, min_span; double min_identity; };

// a record rewritten: the six fields that change
struct TClip { int32_t a1, a2, alen, b1, b2, blen; };

// A, B: anything that is equal exactly when the two reads are the same read (ids on the host, table positions on the device)
__host__ __device__ inline bool trim_eligible(int64_t A, int64_t B, double score, const TParams& P) {
  return A != B && score != 0.0 && !(score < P.min_identity);
}

// the interval [s, e) that the aligned ends x1 .. x2 of one side contribute to their read, or false
__host__ __device__ inline bool trim_interval(int32_t x1, int32_t x2, const TParams& P, int64_t& s, int64_t& e) {
  s = (int64_t)x1 + P.end_clip;
  e = (int64_t)x2 + 1 - P.end_clip;
  return (int64_t)x2 + 1 - x1 >= P.min_span && e > s;
}

__host__ __device__ inline int64_t trim_max0(int64_t a, int64_t b) { return a > b ? a : b; }

// The record (a1, a2, b1, b2, to_rc = o) of an eligible pair onto the clear ranges [ca, ea) of A and [bb, be) of B (B's own forward
// coordinates; blen: B's untrimmed length).  False: the record is void (a deleted read, an empty interval, or nothing left).
__host__ __device__ inline bool trim_clip(int32_t a1, int32_t a2, int32_t b1, int32_t b2, int o, int32_t blen, int32_t ca, int32_t ea,
                                          int32_t bb, int32_t be, TClip& out) {
  if (ea <= ca || be <= bb) return false;
  const int64_t qs = a1, qe = (int64_t)a2 + 1;
  const int64_t ts = o ? (int64_t)blen - b2 - 1 : (int64_t)b1, te = o ? (int64_t)blen - b1 : (int64_t)b2 + 1;
  const int64_t cb = o ? (int64_t)blen - be : (int64_t)bb, eb = o ? (int64_t)blen - bb : (int64_t)be;
  const int64_t SQ = qe - qs, ST = te - ts;
  if (SQ <= 0 || ST <= 0) return false;
  const int64_t d5q = trim_max0(0, ca - qs), d5t = trim_max0(0, cb - ts), d3q = trim_max0(0, qe - ea), d3t = trim_max0(0, te - eb);
  const int64_t s5q = trim_max0(d5q, d5t * SQ / ST), s5t = trim_max0(d5t, d5q * ST / SQ);
  const int64_t s3q = trim_max0(d3q, d3t * SQ / ST), s3t = trim_max0(d3t, d3q * ST / SQ);
  const int64_t qs2 = qs + s5q, qe2 = qe - s3q, ts2 = ts + s5t, te2 = te - s3t;
  if (qe2 <= qs2 || te2 <= ts2) return false;
  const int64_t u = ts2 - cb, v = te2 - cb, nb = eb - cb;
  out.a1 = (int32_t)(qs2 - ca); out.a2 = (int32_t)(qe2 - 1 - ca); out.alen = ea - ca;
  out.b1 = (int32_t)(o ? nb - v : u); out.b2 = (int32_t)(o ? nb - u - 1 : v - 1); out.blen = (int32_t)nb;
  return true;
}

// The best sub-path of a record's alignment path under the stricter score of "read trimming" (+1 per '=' column, -penalty per X, I
// or D column): the runs are walked in order with a running sum that starts again from 0 at an '=' run when it is <= 0, and the best
// is the first strictly greatest sum seen at the end of an '=' run.  (qs, ts): where the path begins on A and on B in the aligner's
// frame.  Out: the sub-path's [qs2, qe2) and [ts2, te2) and its columns and errors; false when the path has no '=' column.
struct TRefined { int64_t qs, qe, ts, te, columns, errors; };
__host__ __device__ inline bool trim_refine(const uint32_t* ops, int64_t n_ops, int64_t qs, int64_t ts, int32_t penalty, TRefined& out) {
  int64_t i = qs, j = ts, cols = 0, errs = 0, sum = 0, best = 0;
  int64_t si = qs, sj = ts, sc = 0, se = 0;   // where the running stretch began
  for (int64_t k = 0; k < n_ops; k++) {
    const int64_t n = ops[k] >> 4;
    const uint32_t code = ops[k] & 15u;
    if (code == 7u) {   // '='
      if (sum <= 0) { sum = 0; si = i; sj = j; sc = cols; se = errs; }
      sum += n; i += n; j += n; cols += n;
      if (sum > best) { best = sum; out = TRefined{si, i, sj, j, cols - sc, errs - se}; }
    } else {
      sum -= (int64_t)penalty * n; cols += n; errs += n;
      if (code == 8u) { i += n; j += n; }   // X
      else if (code == 1u) i += n;          // I: consumes A
      else j += n;                          // D: consumes B
    }
  }
  return best > 0;
}

}  // namespace mhap
