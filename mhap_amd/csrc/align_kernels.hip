// align_kernels.hip — batched local alignment on the GPU: the Smith-Waterman check of EstimateROC's computeDP
// (J/main/EstimateROC.java:746-800, Aligner.align(s1, s2, MATCH_MATRIX, 2, 1, true) with the +2 / -2 matrix of :302-308).
//
// The scoring, tie and path rules are the contract of mhap_align_pairs in include/mhap_hip.h; tests/align_ref.py restates them on the CPU.
// There is no traceback matrix: every cell carries, along the predecessor its rules choose, the begin cell of its path, the path's column
// count and its error count.  The maximum cell's carried values are then what a traceback from it would count.
//
// One workgroup per pair (a persistent grid takes pairs in the order the host sorted them, longest first).  Lane t of the workgroup owns a
// strip of R consecutive rows of s1 (R cells per step, in registers) and processes column j of s2 at step j + t, so the lanes form a
// systolic chain along s1: lane t takes the bottom row of lane t - 1's strip (H, F and their carried values) through __shfl_up inside a
// wave and through a double-buffered LDS slot between waves (one barrier per step).  When s1 has more rows than the workgroup's lanes
// hold, the rows are taken in passes; the bottom row of a pass goes to HBM (10 words per column) and is the top boundary of the next.  The
// first pass is the short one, padded at its top with rows whose H is always 0, which is what the boundary above row 0 is.
//
// The cell rule, the chain between lanes, the work claim, the HBM row, the best-end reduction and the launch path are align_common.hpp's.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "align_common.hpp"
#include "device_common.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

template <int NW>
__global__ __launch_bounds__(NW * 64) void align_pairs_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ pairs,
                                                              const int32_t* __restrict__ order, int n_order, int* __restrict__ next,
                                                              int32_t* __restrict__ scratch, int64_t scratch_stride,
                                                              int32_t* __restrict__ results) {
  constexpr int T = NW * 64;
  __shared__ Edge hand[2][NW > 1 ? NW - 1 : 1];
  const int t = threadIdx.x;
  int32_t* edge = scratch ? scratch + (int64_t)blockIdx.x * scratch_stride : nullptr;
  for (;;) {
    const int k = claim_next(next);
    if (k >= n_order) return;
    const int pi = order[k];
    const int64_t a_off = pairs[5 * (int64_t)pi + 0], b_off = pairs[5 * (int64_t)pi + 2];
    const int m = (int)pairs[5 * (int64_t)pi + 1], n = (int)pairs[5 * (int64_t)pi + 3];
    const bool b_rc = pairs[5 * (int64_t)pi + 4] != 0;
    // lanes and passes: as few passes as T lanes allow, then as few lanes as that many passes need; the padding goes on top of pass 0
    int passes = 1, L = 1;
    if (m > 0) {
      passes = (m + T * AL_R - 1) / (T * AL_R);
      L = (m + passes * AL_R - 1) / (passes * AL_R);
      if (passes * L * AL_R - m >= L * AL_R) { L = T; passes = (m + T * AL_R - 1) / (T * AL_R); }
    }
    const int P = L * AL_R, pad = passes * P - m;
    BestEnd lane_best{0, 0, 0, {0, 0, 0, 0}};   // this lane's best end cell over all passes
    for (int p = 0; p < passes && n > 0 && m > 0; p++) {
      Strip S;
      S.reset();
      const int row0 = p * P + t * AL_R - pad;   // s1 row of register 0 (negative: padding)
#pragma unroll
      for (int r = 0; r < AL_R; r++) {
        const int i = row0 + r;
        S.c1[r] = (t < L && i >= 0 && i < m) ? (uint32_t)bases[a_off + i] : AL_PAD;
      }
      const int steps = n + L - 1;
      for (int s = 0; s < steps; s++) {
        const int j = s - t;
        const bool active = j >= 0 && j < n;
        Edge in = edge_from_above<NW>(S.out, hand, s);
        if (t == 0) in = (p == 0 || !active) ? edge_boundary() : edge_load(edge + j, n);
        if (t < L && active) {
          const uint32_t c2 = b_rc ? rc_char(bases[b_off + (n - 1 - j)]) : (uint32_t)bases[b_off + j];
          S.column(in, c2, row0, j, [](uint32_t, int) { return true; });
          if (t == L - 1 && p + 1 < passes) edge_store(edge + j, n, S.out);
        }
        edge_to_below<NW>(S.out, hand, s);
      }
      if (better_end(S.best, lane_best)) lane_best = S.best;
      __syncthreads();   // the pass's bottom row (HBM) before the next pass reads it
    }
    write_best_end<T>(lane_best, results + 7 * (int64_t)pi);
  }
}

}  // namespace
}  // namespace mhap

using namespace mhap;

extern "C" int mhap_align_pairs(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t* results) {
  const char* who = "mhap_align_pairs";
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (n < 0 || n_bases < 0 || (n > 0 && (!pairs || !results)) || (n_bases > 0 && !bases)) { *v.err = "mhap_align_pairs: null or negative argument"; return MHAP_E_INVALID; }
  if (n > INT32_MAX) { *v.err = "mhap_align_pairs: more than 2^31 - 1 pairs in one call"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  for (int64_t q = 0; q < n; q++) {
    const int64_t* p = pairs + 5 * q;
    for (int f = 0; f < 2; f++) {
      const int64_t off = p[2 * f], len = p[2 * f + 1];
      if (off < 0 || len < 0 || len > INT32_MAX / 2 || off > n_bases - len) {
        *v.err = "mhap_align_pairs: pair " + std::to_string(q) + " has a segment outside the " + std::to_string(n_bases) + " bases";
        return MHAP_E_INVALID;
      }
    }
  }
  // longest first (m * n), and by class: pairs whose s1 fits one wave's lanes take the one-wave kernel
  size_t n_big;
  const std::vector<int32_t> order = longest_first(
      n, [&](int64_t q) { return (pairs[5 * q + 1] + AL_R - 1) / AL_R > 64; },
      [&](int64_t q) { return (double)pairs[5 * q + 1] * (double)pairs[5 * q + 3]; }, n_big);
  // HBM rows between passes: 10 words per column of s2, one set per workgroup of the big kernel
  int64_t n_max_multi = 0;
  for (size_t u = 0; u < n_big; u++) {
    const int64_t* p = pairs + 5 * (int64_t)order[u];
    if (p[1] > (int64_t)AL_NWB * 64 * AL_R) n_max_multi = std::max(n_max_multi, p[3]);
  }
  // at most 2 GiB of pass boundaries: fewer big workgroups in flight beyond that
  const FormShape big{grid_size(n_big, 2, v, 10 * n_max_multi, (int64_t)2 << 30), 10 * n_max_multi};
  const FormShape small{grid_size((size_t)n - n_big, 8, v), 0};
  AlignBufs B;
  hipError_t e;
  int rc = upload_bases(v, B, bases, n_bases, who);
  if (rc != MHAP_OK) return rc;
  if ((e = B.results.ensure(28 * n)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  rc = launch_forms(v, who, B, align_pairs_kernel<AL_NWB>, align_pairs_kernel<1>, pairs, 40, order, n_big, big, small, B.results.as<int32_t>());
  return rc != MHAP_OK ? rc : download_results(v, who, B, results, n);
}
