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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

constexpr int AL_R = 8;                // rows of s1 per lane
constexpr int AL_NEG = -(1 << 28);     // minus infinity for E and F (no overflow over any read length)
constexpr uint32_t AL_PAD = 0x100u;    // s1 "byte" of a padding row: equal to no byte, so its H stays 0

struct Meta { int bi, bj, cols, errs; };   // begin cell (0-based row, column), columns, errors of the path into a cell

__device__ inline Meta meta_sel(bool c, const Meta& a, const Meta& b) {
  return Meta{c ? a.bi : b.bi, c ? a.bj : b.bj, c ? a.cols : b.cols, c ? a.errs : b.errs};
}
__device__ inline Meta meta_shfl_up(const Meta& m) {
  return Meta{__shfl_up(m.bi, 1), __shfl_up(m.bj, 1), __shfl_up(m.cols, 1), __shfl_up(m.errs, 1)};
}
// (score, end column, end row) order of the end cell: higher score, then smaller j, then smaller i
__device__ inline bool better_end(int s, int j, int i, int bs, int bj, int bi) {
  return s > bs || (s == bs && s > 0 && (j < bj || (j == bj && i < bi)));
}

struct Edge { int H, F; Meta mH, mF; };   // the bottom row of a strip at one column: what the strip below reads

template <int NW>
__global__ __launch_bounds__(NW * 64) void align_pairs_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ pairs,
                                                              const int32_t* __restrict__ order, int n_order, int* __restrict__ next,
                                                              int32_t* __restrict__ scratch, int64_t scratch_stride,
                                                              int32_t* __restrict__ results) {
  constexpr int T = NW * 64;
  __shared__ Edge hand[2][NW > 1 ? NW - 1 : 1];     // lane 63 of wave w -> lane 0 of wave w + 1, by step parity
  __shared__ int best_s[T], best_j[T], best_i[T];
  __shared__ Meta best_m[T];
  __shared__ int cur;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  int32_t* edge = scratch ? scratch + (int64_t)blockIdx.x * scratch_stride : nullptr;
  for (;;) {
    if (t == 0) cur = atomicAdd(next, 1);
    __syncthreads();
    const int k = cur;
    __syncthreads();
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
    int ls = 0, lj = 0, li = 0;               // this lane's best end cell over all passes
    Meta lm{0, 0, 0, 0};
    for (int p = 0; p < passes && n > 0 && m > 0; p++) {
      uint32_t c1[AL_R];
      int Hp[AL_R], Ep[AL_R];
      Meta Hm[AL_R], Em[AL_R];
      const int row0 = p * P + t * AL_R - pad;   // s1 row of register 0 (negative: padding)
#pragma unroll
      for (int r = 0; r < AL_R; r++) {
        const int i = row0 + r;
        c1[r] = (t < L && i >= 0 && i < m) ? (uint32_t)bases[a_off + i] : AL_PAD;
        Hp[r] = 0; Ep[r] = AL_NEG; Hm[r] = Meta{0, 0, 0, 0}; Em[r] = Meta{0, 0, 0, 0};
      }
      int dH = 0;                                // H(top - 1, j - 1) and its carried values
      Meta dm{0, 0, 0, 0};
      Edge out{0, AL_NEG, {0, 0, 0, 0}, {0, 0, 0, 0}};
      int ps = 0, pj = 0, pin = 0;               // this pass's best: strict > is the tie rule within a lane (j, then i, increase)
      Meta pm{0, 0, 0, 0};
      const int steps = n + L - 1;
      for (int s = 0; s < steps; s++) {
        const int j = s - t;
        Edge in;
        in.H = __shfl_up(out.H, 1); in.F = __shfl_up(out.F, 1); in.mH = meta_shfl_up(out.mH); in.mF = meta_shfl_up(out.mF);
        if (t == 0) {
          if (p == 0 || j < 0 || j >= n) { in.H = 0; in.F = AL_NEG; in.mH = Meta{0, 0, 0, 0}; in.mF = in.mH; }
          else {
            const int32_t* e = edge + j;
            in.H = e[0]; in.F = e[n]; in.mH = Meta{e[2 * n], e[3 * n], e[4 * n], e[5 * n]}; in.mF = Meta{e[6 * n], e[7 * n], e[8 * n], e[9 * n]};
          }
        } else if (NW > 1 && lane == 0) {
          in = hand[(s + 1) & 1][wave - 1];
        }
        if (t < L && j >= 0 && j < n) {
          const uint32_t c2 = b_rc ? rc_char(bases[b_off + (n - 1 - j)]) : (uint32_t)bases[b_off + j];
          int upH = in.H, upF = in.F;
          Meta upmH = in.mH, upmF = in.mF;
          int diagH = dH;
          Meta diagm = dm;
#pragma unroll
          for (int r = 0; r < AL_R; r++) {
            const int i = row0 + r;
            const bool mis = c1[r] != c2;
            const int D = diagH + (mis ? -2 : 2);
            // E(i,j) = max(H(i,j-1) - 2, E(i,j-1) - 1): a deletion (consumes s2); extension wins a tie
            const int eext = Ep[r] - 1, eopn = Hp[r] - 2;
            const bool ext = eext >= eopn;
            const int E = ext ? eext : eopn;
            Meta me = meta_sel(ext, Em[r], Hm[r]);
            me.cols += 1; me.errs += 1;
            // F(i,j) = max(H(i-1,j) - 2, F(i-1,j) - 1): an insertion (consumes s1); extension wins a tie
            const int fext = upF - 1, fopn = upH - 2;
            const bool fx = fext >= fopn;
            const int F = fx ? fext : fopn;
            Meta mf = meta_sel(fx, upmF, upmH);
            mf.cols += 1; mf.errs += 1;
            // H = max(0, diagonal, E, F), preferring diagonal, then E, then F; a diagonal step out of an H = 0 cell begins a path
            Meta md = diagm;
            md.cols += 1; md.errs += mis ? 1 : 0;
            if (diagH == 0) md = Meta{i, j, 1, mis ? 1 : 0};
            const bool take_d = D > 0 && D >= E && D >= F;
            const bool take_e = !take_d && E > 0 && E >= F;
            const bool take_f = !take_d && !take_e && F > 0;
            const int H = take_d ? D : take_e ? E : take_f ? F : 0;
            Meta mh = meta_sel(take_d, md, meta_sel(take_e, me, mf));
            diagH = Hp[r]; diagm = Hm[r];
            Hp[r] = H; Hm[r] = mh; Ep[r] = E; Em[r] = me;
            upH = H; upF = F; upmH = mh; upmF = mf;
            if (H > ps) { ps = H; pj = j; pin = i; pm = mh; }
          }
          dH = in.H; dm = in.mH;
          out = Edge{upH, upF, upmH, upmF};
          if (t == L - 1 && p + 1 < passes) {
            int32_t* e = edge + j;
            e[0] = out.H; e[n] = out.F;
            e[2 * n] = out.mH.bi; e[3 * n] = out.mH.bj; e[4 * n] = out.mH.cols; e[5 * n] = out.mH.errs;
            e[6 * n] = out.mF.bi; e[7 * n] = out.mF.bj; e[8 * n] = out.mF.cols; e[9 * n] = out.mF.errs;
          }
        }
        if constexpr (NW > 1) {
          if (lane == 63 && wave + 1 < NW) hand[s & 1][wave] = out;
          __syncthreads();
        }
      }
      if (better_end(ps, pj, pin, ls, lj, li)) { ls = ps; lj = pj; li = pin; lm = pm; }
      __syncthreads();   // the pass's bottom row (HBM) before the next pass reads it
    }
    best_s[t] = ls; best_j[t] = lj; best_i[t] = li; best_m[t] = lm;
    __syncthreads();
    if (t == 0) {
      int b = 0;
      for (int u = 1; u < T; u++)
        if (better_end(best_s[u], best_j[u], best_i[u], best_s[b], best_j[b], best_i[b])) b = u;
      int32_t* o = results + 7 * (int64_t)pi;
      if (best_s[b] > 0) {
        o[0] = best_s[b]; o[1] = best_m[b].bi; o[2] = best_i[b]; o[3] = best_m[b].bj; o[4] = best_j[b];
        o[5] = best_m[b].cols; o[6] = best_m[b].errs;
      } else {
        o[0] = 0; o[1] = o[2] = o[3] = o[4] = -1; o[5] = o[6] = 0;
      }
    }
    __syncthreads();
  }
}

struct AlignBufs {
  DevBuf bases, pairs, order, next, scratch, results;
  void release() { bases.release(); pairs.release(); order.release(); next.release(); scratch.release(); results.release(); }
};

}  // namespace
}  // namespace mhap

using namespace mhap;

extern "C" int mhap_align_pairs(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t* results) {
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
  constexpr int NWB = 4;
  std::vector<int32_t> big, small;
  for (int64_t q = 0; q < n; q++) ((pairs[5 * q + 1] + AL_R - 1) / AL_R > 64 ? big : small).push_back((int32_t)q);
  auto cells = [&](int32_t q) { return (double)pairs[5 * (int64_t)q + 1] * (double)pairs[5 * (int64_t)q + 3]; };
  auto by_cells = [&](int32_t a, int32_t b) { const double ca = cells(a), cb = cells(b); return ca != cb ? ca > cb : a < b; };
  std::stable_sort(big.begin(), big.end(), by_cells);
  std::stable_sort(small.begin(), small.end(), by_cells);
  std::vector<int32_t> order(big);
  order.insert(order.end(), small.begin(), small.end());
  // HBM rows between passes: 10 words per column of s2, one set per workgroup of the big kernel
  int64_t n_max_multi = 0;
  for (int32_t q : big) if (pairs[5 * (int64_t)q + 1] > (int64_t)NWB * 64 * AL_R) n_max_multi = std::max(n_max_multi, pairs[5 * (int64_t)q + 3]);
  int grid_big = (int)std::min<int64_t>((int64_t)big.size(), 2LL * v.num_cus);   // (the handle's compute units: MHAP_NUM_CUS caps them)
  const int grid_small = (int)std::min<int64_t>((int64_t)small.size(), 8LL * v.num_cus);
  const int64_t stride = 10 * n_max_multi;
  if (stride > 0) {
    const int64_t budget = (int64_t)2 << 30;   // at most 2 GiB of pass boundaries: fewer big workgroups in flight beyond that
    grid_big = (int)std::max<int64_t>(1, std::min<int64_t>(grid_big, budget / (stride * 4)));
  }
  AlignBufs B;
  auto fail = [&](hipError_t e, const char* what) {
    *v.err = std::string("mhap_align_pairs: ") + what + ": " + hipGetErrorString(e);
    B.release();
    return MHAP_E_HIP;
  };
  hipError_t e;
  (void)hipSetDevice(v.device);
  if ((e = B.bases.ensure(std::max<int64_t>(n_bases, 1))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.pairs.ensure(40 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.order.ensure(4 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.next.ensure(8)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.results.ensure(28 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if (stride > 0 && (e = B.scratch.ensure((size_t)stride * 4 * grid_big)) != hipSuccess) return fail(e, "hipMalloc (pass boundaries)");
  if (n_bases > 0 && (e = hipMemcpyAsync(B.bases.p, bases, n_bases, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemcpyAsync(B.pairs.p, pairs, 40 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemcpyAsync(B.order.p, order.data(), 4 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemsetAsync(B.next.p, 0, 8, v.stream)) != hipSuccess) return fail(e, "memset");
  int* nx = B.next.as<int>();
  if (!big.empty())
    hipLaunchKernelGGL(align_pairs_kernel<NWB>, dim3(grid_big), dim3(NWB * 64), 0, v.stream, B.bases.as<uint8_t>(), B.pairs.as<int64_t>(),
                       B.order.as<int32_t>(), (int)big.size(), nx, stride > 0 ? B.scratch.as<int32_t>() : nullptr, stride, B.results.as<int32_t>());
  if (!small.empty())
    hipLaunchKernelGGL(align_pairs_kernel<1>, dim3(grid_small), dim3(64), 0, v.stream, B.bases.as<uint8_t>(), B.pairs.as<int64_t>(),
                       B.order.as<int32_t>() + big.size(), (int)small.size(), nx + 1, nullptr, (int64_t)0, B.results.as<int32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  if ((e = hipMemcpyAsync(results, B.results.p, 28 * n, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail(e, "kernel");
  B.release();
  return MHAP_OK;
}
