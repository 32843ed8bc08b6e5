// select_common.hpp — the rule of "overlap selection" (include/mhap_hip.h) that host and device share, written once: the key of one
// view of an eligible record.  entry_kernel and apply_kernel (select_kernels.hip) and mhap_select_judge_record (host, no GPU) all go
// through select_key.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "trim_common.hpp"

namespace mhap {

struct SParams { int32_t best_n, min_span; double min_identity; };

// the trimming's rule and one clause more: a NaN score is not eligible
__host__ __device__ inline bool select_eligible(int64_t A, int64_t B, double score, double min_identity) {
  return trim_eligible(A, B, score, TParams{1, 0, 0, min_identity}) && score == score;
}

// The key of the view that spans x1 .. x2 of its read, 0 when the span is below min_span: 1 + floor(span * min(score, 1)), the
// counted matches on that read.  One compare, one min, one multiply of a double by an exact integer and one floor: nothing here
// can be contracted into a fused operation, so host and device give the same bits.  span < 2^31 and 0 < min(score, 1) <= 1 (a
// negative score gives a negative product, which the conversion below would not define: it counts as no match at all).
__host__ __device__ inline uint32_t select_key(int32_t x1, int32_t x2, double score, int32_t min_span) {
  const int64_t span = (int64_t)x2 + 1 - x1;
  if (span < min_span) return 0u;
  const double m = floor((double)span * (score < 1.0 ? score : 1.0));
  return 1u + (m > 0.0 ? (uint32_t)m : 0u);
}

}  // namespace mhap
