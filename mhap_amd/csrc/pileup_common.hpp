// pileup_common.hpp — what "read trimming" (trim_kernels.hip) and "repeat marking" (repeat_kernels.hip) share, written once: the
// per-base difference array of a table of reads, the kernel that piles records up on it, the tile step that turns differences into
// coverage, and the host side of a pile up to the add.  The table of reads, the packed records and the queued uploads underneath
// are read_table.hpp's ReadTable, which needs no pile.
//
// Layout: read r owns lengths[r] + 1 int32 slots at an offset rounded up to four slots, so that a read's slots begin on a 16-byte
// word; the array is zeroed once.  A tile is PILE_TILE positions: four 16-byte loads per lane of a workgroup of 256, each contiguous
// across the wave, so a lane holds four groups of four positions and the order of a tile is (load j, lane, k).
#pragma once
#include <hip/hip_runtime.h>

#include <numeric>
#include <vector>

#include "read_table.hpp"
#include "trim_common.hpp"

namespace mhap {
namespace {

enum { PILE_T = 256, PILE_WAVES = PILE_T / 64, PILE_LOADS = 4, PILE_TILE = PILE_T * PILE_LOADS * 4 };

// one lane per record: +1 at an interval's begin, -1 at its end, up to four atomicAdd(int32); the eligible records are counted once
// per wave.  The intervals are trim_interval's: P.end_clip = P.min_span = 0 gives the aligned intervals as they are.
__global__ __launch_bounds__(256) void add_kernel(const int4* __restrict__ items, int64_t n, const int32_t* __restrict__ lengths,
                                                  const int64_t* __restrict__ off, TParams P, int32_t* __restrict__ diff,
                                                  u64* __restrict__ eligible) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool el = false;
  if (q < n) {
    const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
    const int32_t A = w0.x, B = w0.y >> 1;
    el = trim_eligible(A, B, __hiloint2double(w1.w, w1.z), P);
    if (el) {
      int64_t s, e;   // (the host has refused ends outside the read; the bounds are looked at again where the store is)
      if (trim_interval(w0.z, w0.w, P, s, e) && s >= 0 && e <= lengths[A]) { atomicAdd(diff + off[A] + s, 1); atomicAdd(diff + off[A] + e, -1); }
      if (trim_interval(w1.x, w1.y, P, s, e) && s >= 0 && e <= lengths[B]) { atomicAdd(diff + off[B] + s, 1); atomicAdd(diff + off[B] + e, -1); }
    }
  }
  const u64 m = __ballot(el);   // one add per wave
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(eligible, (u64)__popcll(m));
}

__device__ inline int32_t quad(const int4& d, int k) { return k == 0 ? d.x : k == 1 ? d.y : k == 2 ? d.z : d.w; }

// The tile of 16-byte words g0 .. of a read's `groups` words at `base`: d[j] = the lane's four differences of load j (zeros behind
// the read) and c0[j] = the coverage in front of them, by a wave scan of the lanes' sums and the 16 (j, wave) totals in ws.  carry:
// the coverage at the tile's end, taken from and handed to the next tile.  One __syncthreads, between the write of ws and its reads:
// the caller has another one between this call and the next.
__device__ inline void pile_coverage_tile(const int4* __restrict__ base, int64_t groups, int64_t g0, int tid, int lane, int wave,
                                          int32_t (*ws)[PILE_WAVES], int32_t& carry, int4 (&d)[PILE_LOADS], int32_t (&c0)[PILE_LOADS]) {
  int32_t tot[PILE_LOADS], inc[PILE_LOADS], pre[PILE_LOADS];
#pragma unroll
  for (int j = 0; j < PILE_LOADS; j++) {
    const int64_t g = g0 + j * PILE_T + tid;
    d[j] = g < groups ? base[g] : make_int4(0, 0, 0, 0);
    inc[j] = tot[j] = d[j].x + d[j].y + d[j].z + d[j].w;
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const int32_t u = __shfl_up(inc[j], s);
      if (lane >= s) inc[j] += u;
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) ws[j][wave] = inc[j];
  }
  __syncthreads();
  int32_t acc = carry;
#pragma unroll
  for (int j = 0; j < PILE_LOADS; j++) {
#pragma unroll
    for (int w = 0; w < PILE_WAVES; w++) {
      if (w == wave) pre[j] = acc;
      acc += ws[j][w];
    }
  }
  carry = acc;
#pragma unroll
  for (int j = 0; j < PILE_LOADS; j++) c0[j] = pre[j] + inc[j] - tot[j];
}

// The same shape for any associative op: v[j] = the lane's own value of load j (in), ex[j] = op over `carry` and everything in
// front of the lane in the tile's order (out); carry becomes op over the whole tile.  One __syncthreads, as above.
template <class T, class Op>
__device__ inline void pile_scan_tile(const T (&v)[PILE_LOADS], int lane, int wave, T (*wl)[PILE_WAVES], T& carry, T (&ex)[PILE_LOADS], Op op) {
  T inc[PILE_LOADS];
#pragma unroll
  for (int j = 0; j < PILE_LOADS; j++) inc[j] = v[j];
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const T u = __shfl_up(inc[j], s);
      if (lane >= s) inc[j] = op(u, inc[j]);
    }
  }
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) wl[j][wave] = inc[j];
  }
  __syncthreads();
  T acc = carry;
#pragma unroll
  for (int j = 0; j < PILE_LOADS; j++) {
    const T left = __shfl_up(inc[j], 1);
#pragma unroll
    for (int w = 0; w < PILE_WAVES; w++) {
      if (w == wave) ex[j] = lane > 0 ? op(acc, left) : acc;
      acc = op(acc, wl[j][w]);
    }
  }
  carry = acc;
}

// The table with the per-base difference array of the trimming and the repeat marking on top.
struct Pile : ReadTable {
  int64_t bases_in = 0, n_slots = 0;
  std::vector<int64_t> slot_off;                          // slot_off[r]: read r's first slot of the difference array
  std::vector<int32_t> order;                             // the reads longest first (the upload reads it until the begin has waited)
  DevBuf d_off, d_order, diff;

  void release_pile() {
    release_table();
    for (DevBuf* b : {&d_off, &d_order, &diff}) b->release();
  }

  // the table on the host and on the device, the difference array zeroed; queued on the handle's stream, not waited for
  hipError_t begin_pile(const HandleView& v, mhap_handle* handle, const int64_t* read_ids, const int32_t* lens, int64_t n) {
    hipError_t e = begin_table(v, handle, read_ids, lens, n);
    slot_off.resize((size_t)n + 1);
    for (int64_t i = 0; i < n; i++) {
      slot_off[(size_t)i] = n_slots;
      n_slots += ((int64_t)lens[i] + 4) & ~(int64_t)3;
      bases_in += lens[i];
    }
    slot_off[(size_t)n] = n_slots;
    order.resize((size_t)n);   // the long workgroups start early
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return lens[a] > lens[b]; });
    const size_t nr = (size_t)std::max<int64_t>(n, 1), db = 4 * (size_t)std::max<int64_t>(n_slots, 4);
    if (e == hipSuccess) e = d_order.ensure(4 * nr);
    if (e == hipSuccess) e = d_off.ensure(8 * (nr + 1));
    if (e == hipSuccess) e = diff.ensure(db);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_order.p, order.data(), 4 * (size_t)n, hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, slot_off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, v.stream);
    if (e == hipSuccess) e = hipMemsetAsync(diff.p, 0, db, v.stream);
    return e;
  }

  // an add: the records are checked (a refused call queues nothing), uploaded and piled up under P; nothing waits
  int add_records(const char* who, const mhap_record* recs, int64_t n, const TParams& P, u64* d_eligible) {
    HandleView v = handle_view(h);
    Pending p;
    const int rc = queue_add(v, who, recs, n, p);
    if (rc != MHAP_OK || !p.ev) return rc;
    hipLaunchKernelGGL(add_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, items.as<int4>(), n, d_lengths.as<int32_t>(),
                       d_off.as<int64_t>(), P, diff.as<int32_t>(), d_eligible);
    return commit_add(v, who, p, n);
  }
};

}  // namespace
}  // namespace mhap
