// weighted_vote.hpp — what is about weights in the "quality-weighted votes" contract of include/mhap_hip.h: an evidence byte votes
// with the weight of its own Phred value, Del and span with the neutral 2, and every comparison of the call is the unweighted one in
// doubled units.  The thresholds, the weight of a Phred value, the cap on views and the two weight policies are here; the walk, the
// decision, the qualities and the kernels are vote_common.hpp's and the callers', written once over a policy.
#pragma once
#include "vote_common.hpp"

namespace mhap {

constexpr int W_NEUTRAL = 2;
constexpr uint32_t WK_CAP = CK_CAP / 3;   // accepted views per target: a view adds at most 3 to a counter

struct Weights { int q_lo, q_hi; };

inline bool weight_params_ok(int q_lo, int q_hi, const char* who, std::string& err) {
  if (q_lo >= 0 && q_lo <= q_hi && q_hi < QUAL_BINS) return true;
  err = std::string(who) + ": the weights need 0 <= q_lo <= q_hi <= 93 (" + std::to_string(q_lo) + ", " + std::to_string(q_hi) + ")";
  return false;
}

__device__ inline int weight_of(uint32_t q, Weights W) { return 1 + ((int)q >= W.q_lo ? 1 : 0) + ((int)q >= W.q_hi ? 1 : 0); }

// the byte stored at `at` weighs what its Phred value says; quals: one byte per base, parallel to the bases
struct QualityWeight {
  static constexpr int neutral = W_NEUTRAL;
  const uint8_t* quals;
  Weights W;
  __device__ int operator()(int64_t at) const { return weight_of(quals[at], W); }
};

// a byte without a quality of its own in a weighted table (a draft byte of the consensus): the neutral weight
struct NeutralWeight {
  static constexpr int neutral = W_NEUTRAL;
  __device__ int operator()(int64_t) const { return W_NEUTRAL; }
};

}  // namespace mhap
