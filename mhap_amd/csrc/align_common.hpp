// align_common.hpp — what the alignment kernels (align_kernels.hip: full matrix; realign_kernels.hip: banded, and the trace of a path)
// share: the cell rule of the contract in include/mhap_hip.h, the systolic chain between lanes, the persistent grid's work claim, the
// bottom row of a pass in HBM, the reduction of the best end cell, and the host code that orders, sizes and launches a batch.  Each is
// written here once; the kernels differ in which columns a lane walks, and that is all they state themselves.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "mhap_internal.hpp"

namespace mhap {

constexpr int AL_R = 8;                // rows of s1 per lane
constexpr int AL_NEG = -(1 << 28);     // minus infinity for E and F (no overflow over any read length)
constexpr uint32_t AL_PAD = 0x100u;    // s1 "byte" of a row that does not exist: equal to no byte, so its H stays 0
constexpr int AL_NWB = 4;              // waves of the wide form of a kernel; the other form has one

struct Meta { int bi, bj, cols, errs; };   // begin cell (0-based row, column), columns, errors of the path into a cell

__device__ inline Meta meta_sel(bool c, const Meta& a, const Meta& b) {
  return Meta{c ? a.bi : b.bi, c ? a.bj : b.bj, c ? a.cols : b.cols, c ? a.errs : b.errs};
}
__device__ inline Meta meta_shfl_up(const Meta& m) {
  return Meta{__shfl_up(m.bi, 1), __shfl_up(m.bj, 1), __shfl_up(m.cols, 1), __shfl_up(m.errs, 1)};
}

struct BestEnd { int s, j, i; Meta m; };   // an end cell: score, column, row and what the cell carries
// (score, end column, end row) order of the end cell: higher score, then smaller j, then smaller i
__device__ inline bool better_end(const BestEnd& a, const BestEnd& b) {
  return a.s > b.s || (a.s == b.s && a.s > 0 && (a.j < b.j || (a.j == b.j && a.i < b.i)));
}

// The bottom row of a strip at one column, what the strip below reads: all of it for the aligners, H and F for the trace.
struct Edge { int H, F; Meta mH, mF; };
struct EdgeHF { int H, F; };
__device__ inline Edge edge_boundary() { return Edge{0, AL_NEG, {0, 0, 0, 0}, {0, 0, 0, 0}}; }   // above row 0, outside a band
__device__ inline Edge edge_shfl_up(const Edge& e) { return Edge{__shfl_up(e.H, 1), __shfl_up(e.F, 1), meta_shfl_up(e.mH), meta_shfl_up(e.mF)}; }
__device__ inline EdgeHF edge_shfl_up(const EdgeHF& e) { return EdgeHF{__shfl_up(e.H, 1), __shfl_up(e.F, 1)}; }

// an edge to or from LDS, word by word (as one struct copy the compiler wants its registers in aligned runs, which cost the trace
// kernel's wide form 8 VGPRs and a wave per SIMD)
template <class E>
__device__ __forceinline__ void edge_copy(E& dst, const E& src) {
  static_assert(sizeof(E) % sizeof(int) == 0, "an edge is a row of ints");
#pragma unroll
  for (unsigned i = 0; i < sizeof(E) / sizeof(int); i++) ((int*)&dst)[i] = ((const int*)&src)[i];
}

// The systolic chain: what the lane above put out one step ago.  __shfl_up inside a wave; lane 63 of wave w reaches lane 0 of wave
// w + 1 through hand[step parity][w] (LDS), published by edge_to_below at the end of every step, which is the step's one barrier.
template <int NW, class E>
__device__ __forceinline__ E edge_from_above(const E& out, const E (&hand)[2][NW > 1 ? NW - 1 : 1], int s) {
  E in = edge_shfl_up(out);
  if (NW > 1 && (threadIdx.x & 63) == 0 && threadIdx.x > 0) edge_copy(in, hand[(s + 1) & 1][(threadIdx.x >> 6) - 1]);
  return in;
}
template <int NW, class E>
__device__ __forceinline__ void edge_to_below(const E& out, E (&hand)[2][NW > 1 ? NW - 1 : 1], int s) {
  if constexpr (NW > 1) {
    if ((threadIdx.x & 63) == 63 && (threadIdx.x >> 6) + 1 < NW) edge_copy(hand[s & 1][threadIdx.x >> 6], out);
    __syncthreads();
  }
}

// The bottom row of a pass in HBM, the top boundary of the next: 10 words per column, word w of the column at e[w * stride].  The
// stride is the number of columns kept: n in the full matrix, the band's W diagonals in the banded kernel.
__device__ __forceinline__ Edge edge_load(const int32_t* e, int stride) {
  return Edge{e[0], e[stride], Meta{e[2 * stride], e[3 * stride], e[4 * stride], e[5 * stride]},
              Meta{e[6 * stride], e[7 * stride], e[8 * stride], e[9 * stride]}};
}
__device__ __forceinline__ void edge_store(int32_t* e, int stride, const Edge& o) {
  e[0] = o.H; e[stride] = o.F;
  e[2 * stride] = o.mH.bi; e[3 * stride] = o.mH.bj; e[4 * stride] = o.mH.cols; e[5 * stride] = o.mH.errs;
  e[6 * stride] = o.mF.bi; e[7 * stride] = o.mF.bj; e[8 * stride] = o.mF.cols; e[9 * stride] = o.mF.errs;
}

// The cell rule.  From H(i-1,j-1), H(i,j-1), E(i,j-1), H(i-1,j), F(i-1,j) and whether the two bytes differ: the cell's H, E, F and
// the choices that made them.  Whatever follows a path — the carried fields of the aligners, the nibble of the trace — reads the
// choices from here and repeats no comparison.
struct Cell { int H, E, F; bool ext, fx, take_d, take_e; };
__device__ __forceinline__ Cell cell_rule(int diagH, int Hp, int Ep, int upH, int upF, bool mis) {
  Cell c;
  const int D = diagH + (mis ? -2 : 2);
  // E(i,j) = max(H(i,j-1) - 2, E(i,j-1) - 1): a deletion (consumes s2); extension wins a tie
  const int eext = Ep - 1, eopn = Hp - 2;
  c.ext = eext >= eopn;
  c.E = c.ext ? eext : eopn;
  // F(i,j) = max(H(i-1,j) - 2, F(i-1,j) - 1): an insertion (consumes s1); extension wins a tie
  const int fext = upF - 1, fopn = upH - 2;
  c.fx = fext >= fopn;
  c.F = c.fx ? fext : fopn;
  // H = max(0, diagonal, E, F), preferring diagonal, then E, then F
  c.take_d = D > 0 && D >= c.E && D >= c.F;
  c.take_e = !c.take_d && c.E > 0 && c.E >= c.F;
  const bool take_f = !c.take_d && !c.take_e && c.F > 0;
  c.H = c.take_d ? D : c.take_e ? c.E : take_f ? c.F : 0;
  return c;
}

// A lane's strip of an aligner: AL_R rows of one column in registers, with what every cell carries along the predecessor the rule
// chose (there is no traceback matrix: the maximum cell's carried values are what a traceback from it would count).
struct Strip {
  uint32_t c1[AL_R];             // the rows' bytes of s1, AL_PAD where there is no row: the kernel fills them
  int Hp[AL_R], Ep[AL_R];        // H and E of the previous column
  Meta Hm[AL_R], Em[AL_R];
  int dH;                        // H(row0 - 1, j - 1) and its carried values
  Meta dm;
  Edge out;                      // the bottom row at the column just done
  BestEnd best;                  // this pass's best: strict > is the tie rule within a lane (j, then i, increase)

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int r = 0; r < AL_R; r++) { Hp[r] = 0; Ep[r] = AL_NEG; Hm[r] = Meta{0, 0, 0, 0}; Em[r] = Meta{0, 0, 0, 0}; }
    dH = 0; dm = Meta{0, 0, 0, 0};
    out = edge_boundary();
    best = BestEnd{0, 0, 0, {0, 0, 0, 0}};
  }

  // Column j (byte c2 of s2) of the rows row0 ..., below the row `in`.  A cell for which inband(c1[r], r) is false is the boundary (H 0,
  // E = F = -inf); what it carries is never read: only a positive value's carried fields reach a result, and nothing positive
  // descends from the boundary.
  template <class InBand>
  __device__ __forceinline__ void column(const Edge& in, uint32_t c2, int row0, int j, InBand inband) {
    int upH = in.H, upF = in.F, diagH = dH;
    Meta upmH = in.mH, upmF = in.mF, diagm = dm;
#pragma unroll
    for (int r = 0; r < AL_R; r++) {
      const bool mis = c1[r] != c2;
      Cell c = cell_rule(diagH, Hp[r], Ep[r], upH, upF, mis);
      Meta me = meta_sel(c.ext, Em[r], Hm[r]);
      me.cols += 1; me.errs += 1;
      Meta mf = meta_sel(c.fx, upmF, upmH);
      mf.cols += 1; mf.errs += 1;
      Meta md = diagm;
      md.cols += 1; md.errs += mis ? 1 : 0;
      if (diagH == 0) md = Meta{row0 + r, j, 1, mis ? 1 : 0};   // a diagonal step out of an H = 0 cell begins a path
      const Meta mh = meta_sel(c.take_d, md, meta_sel(c.take_e, me, mf));
      if (!inband(c1[r], r)) { c.H = 0; c.E = AL_NEG; c.F = AL_NEG; }
      diagH = Hp[r]; diagm = Hm[r];
      Hp[r] = c.H; Hm[r] = mh; Ep[r] = c.E; Em[r] = me;
      upH = c.H; upF = c.F; upmH = mh; upmF = mf;
      if (c.H > best.s) best = BestEnd{c.H, j, row0 + r, mh};
    }
    dH = in.H; dm = in.mH;
    out = Edge{upH, upF, upmH, upmF};
  }
};

// The next item of a persistent grid: every lane of the workgroup calls it and gets the same index into the launch's order.
__device__ __forceinline__ int claim_next(int* next) {
  __shared__ int cur;
  if (threadIdx.x == 0) cur = atomicAdd(next, 1);
  __syncthreads();
  const int k = cur;
  __syncthreads();
  return k;
}

// The best end cell of a workgroup of T lanes from every lane's own, and the seven result fields of the pair (o), or those of "no
// alignment".  Every lane calls it; it ends in a barrier, so the next item may follow at once.
template <int T>
__device__ __forceinline__ void write_best_end(const BestEnd& mine, int32_t* o) {
  __shared__ BestEnd best[T];
  best[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
    for (int u = 1; u < T; u++)
      if (better_end(best[u], best[b])) b = u;
    if (best[b].s > 0) {
      o[0] = best[b].s; o[1] = best[b].m.bi; o[2] = best[b].i; o[3] = best[b].m.bj; o[4] = best[b].j;
      o[5] = best[b].m.cols; o[6] = best[b].m.errs;
    } else {
      o[0] = 0; o[1] = o[2] = o[3] = o[4] = -1; o[5] = o[6] = 0;
    }
  }
  __syncthreads();
}

// ---- host side: one batch through the wide and the one-wave form of a kernel -------------------------------------------------------------

// The device buffers of a launch path; whatever a path does not use stays empty.  Freed when the call that owns them returns.
struct AlignBufs {
  DevBuf bases, items, order, next, scratch, results, trace, ops, n_ops;
  AlignBufs() = default;
  AlignBufs(const AlignBufs&) = delete;
  AlignBufs& operator=(const AlignBufs&) = delete;
  ~AlignBufs() { for (DevBuf* b : {&bases, &items, &order, &next, &scratch, &results, &trace, &ops, &n_ops}) b->release(); }
};

inline int upload_bases(const HandleView& v, AlignBufs& B, const uint8_t* bases, int64_t n_bases, const char* who) {
  hipError_t e;
  (void)hipSetDevice(v.device);
  if ((e = B.bases.ensure((size_t)std::max<int64_t>(n_bases, 1))) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  if (n_bases > 0 && (e = hipMemcpyAsync(B.bases.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  return MHAP_OK;
}

// The order a persistent launch takes n items in: those for which big(q) holds (the wide form's) before the others, each class
// longest first by cells(q), the index breaking ties.  n_big: how many the wide form takes.
template <class Big, class Cells>
std::vector<int32_t> longest_first(int64_t n, Big big, Cells cells, size_t& n_big) {
  std::vector<int32_t> order, small;
  for (int64_t q = 0; q < n; q++) (big(q) ? order : small).push_back((int32_t)q);
  n_big = order.size();
  order.insert(order.end(), small.begin(), small.end());
  auto by_cells = [&](int32_t a, int32_t b) { const double ca = cells(a), cb = cells(b); return ca != cb ? ca > cb : a < b; };
  std::stable_sort(order.begin(), order.begin() + n_big, by_cells);
  std::stable_sort(order.begin() + n_big, order.end(), by_cells);
  return order;
}

// Workgroups of one form: per_cu for each of the handle's compute units (MHAP_NUM_CUS caps them) and no more than its items; when a
// workgroup keeps stride_words of pass boundaries in HBM and there is a budget, no more than fit it (but one).
inline int grid_size(size_t n_items, int per_cu, const HandleView& v, int64_t stride_words = 0, int64_t budget_bytes = 0) {
  int64_t g = std::min<int64_t>((int64_t)n_items, (int64_t)per_cu * v.num_cus);
  if (stride_words > 0 && budget_bytes > 0) g = std::max<int64_t>(1, std::min<int64_t>(g, budget_bytes / (stride_words * 4)));
  return (int)g;
}

// One form of a launch: its workgroups and the words of pass boundaries each of them keeps (0: its items need no second pass).
struct FormShape { int grid; int64_t stride; };

// Grow, upload, zero, launch, check: the order's items (host, item_bytes each) into B.items, their order into B.order, the two claim counters zeroed, B.scratch
// grown to both forms' pass boundaries, then the wide form over order[0, n_big) and the one-wave form over the rest, both on
// v.stream against B.bases.  The caller has sized whatever `out` points to.
template <class Item, class Out>
int launch_forms(const HandleView& v, const char* who, AlignBufs& B,
                 void (*wide)(const uint8_t*, const Item*, const int32_t*, int, int*, int32_t*, int64_t, Out*),
                 void (*narrow)(const uint8_t*, const Item*, const int32_t*, int, int*, int32_t*, int64_t, Out*),
                 const Item* items, size_t item_bytes, const std::vector<int32_t>& order, size_t n_big, FormShape big, FormShape small, Out* out) {
  const size_t n = order.size();
  const int64_t scratch_big = big.stride * big.grid, scratch_words = scratch_big + small.stride * small.grid;
  hipError_t e;
  if ((e = B.items.ensure(item_bytes * n)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  if ((e = B.order.ensure(4 * n)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  if ((e = B.next.ensure(8)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  if (scratch_words > 0 && (e = B.scratch.ensure((size_t)scratch_words * 4)) != hipSuccess) return hip_fail(v, who, "hipMalloc (pass boundaries)", e);
  if ((e = hipMemcpyAsync(B.items.p, items, item_bytes * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  if ((e = hipMemcpyAsync(B.order.p, order.data(), 4 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  if ((e = hipMemsetAsync(B.next.p, 0, 8, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  int* nx = B.next.as<int>();
  if (n_big > 0)
    hipLaunchKernelGGL(wide, dim3(big.grid), dim3(AL_NWB * 64), 0, v.stream, B.bases.as<uint8_t>(), B.items.as<Item>(), B.order.as<int32_t>(),
                       (int)n_big, nx, big.stride > 0 ? B.scratch.as<int32_t>() : nullptr, big.stride, out);
  if (n > n_big)
    hipLaunchKernelGGL(narrow, dim3(small.grid), dim3(64), 0, v.stream, B.bases.as<uint8_t>(), B.items.as<Item>(), B.order.as<int32_t>() + n_big,
                       (int)(n - n_big), nx + 1, small.stride > 0 ? B.scratch.as<int32_t>() + scratch_big : nullptr, small.stride, out);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  return MHAP_OK;
}

// The seven fields of every pair from B.results to the host, and the end of the stream's work.
inline int download_results(const HandleView& v, const char* who, const AlignBufs& B, int32_t* results, int64_t n) {
  hipError_t e;
  if ((e = hipMemcpyAsync(results, B.results.p, 28 * n, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  return MHAP_OK;
}

}  // namespace mhap
