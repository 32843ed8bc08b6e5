// repeat_kernels.hip — repeats marked from the overlap pile-up and repeat-only overlaps set aside (mhap_repeat_begin / _add / _finish /
// _copy / _histogram / _apply / _judge_record / _free).  The contract — eligible records, coverage, the typical depth D, the threshold
// T, the repeat intervals, the per-read row and a record's judgement — is the prose of include/mhap_hip.h ("repeat marking");
// tests/repeat_ref.py restates it.  The difference array, the add and the tile's coverage scan are pileup_common.hpp's, shared with
// the trimming.
//
// add:    pileup_common.hpp's add_kernel with end_clip = min_span = 0: the aligned intervals as they are.  Nothing waits.
// finish: hist_kernel, one workgroup of 256 lanes per read, longest first, over tiles of PILE_TILE positions: the coverage of every
//         position goes into 4096 bins in LDS (a lane adds a stretch of equal depths at once) and the bins up to the read's greatest
//         are flushed with 64-bit atomics.  depth_kernel, one workgroup, reads the bins and leaves {D, T} on the device.
//         mark_kernel<false> walks every read again and counts its intervals, their bases, its greatest depth and its first begin
//         (the row, the flag byte, the counts); scan_kernel turns the counts into the offsets; mark_kernel<true> walks the reads
//         that have intervals a third time and writes each interval at offsets[r] + (the intervals closed before it) together with
//         the bases of the read's intervals in front of it.  A run's begin comes from a running maximum of the begins, carried across
//         tiles, and its rank from a scan of (bases << 32 | count) in the tile's order: every interval has one writer and no atomic
//         decides a place.  The host waits once, for the bins, {D, T} and the counts.
// apply:  one lane per packed record; per read two binary searches in its intervals give the positions of the aligned interval that
//         lie inside them.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_common.hpp"
#include "graph_class.hpp"
#include "mhap_internal.hpp"
#include "pileup_common.hpp"
#include "trim_common.hpp"

namespace mhap {
namespace {

// counts: reads, reads with an interval, whole-repeat reads, intervals, repeat bases, bases, eligible records, D, T
enum { RC_READS = 0, RC_SOME, RC_WHOLE, RC_INTERVALS, RC_REPEAT_BASES, RC_BASES, RC_ELIGIBLE, RC_D, RC_T };
static_assert(RC_T + 1 == MHAP_REPEAT_COUNTS, "the counts of the header");
static_assert(MHAP_REPEAT_BINS == PILE_TILE, "the bins are zeroed and flushed like a tile is walked");

struct RParams { int32_t factor_pct, max_cov, min_run, min_unique; };

// the positions of [0, x) that lie inside the n ascending, disjoint intervals iv; cum[i] = the bases of the intervals in front of i
__host__ __device__ inline int64_t repeat_below(const int2* iv, const int32_t* cum, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;   // the intervals that begin in front of x
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (iv[mid].x < x) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;
  const int2 last = iv[lo - 1];
  return (int64_t)cum[lo - 1] + ((x < last.y ? x : (int64_t)last.y) - last.x);
}

// the aligned positions x1 .. x2 of one side that lie outside the read's intervals
__host__ __device__ inline int32_t repeat_unique(const int2* iv, const int32_t* cum, int64_t n, int32_t x1, int32_t x2) {
  const int64_t s = x1, e = (int64_t)x2 + 1;
  return (int32_t)((e - s) - (repeat_below(iv, cum, n, e) - repeat_below(iv, cum, n, s)));
}

__global__ __launch_bounds__(PILE_T) void hist_kernel(const int32_t* __restrict__ diff, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ lengths, const int32_t* __restrict__ order,
                                                      u64* __restrict__ hist) {
  __shared__ uint32_t bins[MHAP_REPEAT_BINS];
  __shared__ int32_t ws[PILE_LOADS][PILE_WAVES], wx[PILE_WAVES];
  const int32_t r = order[blockIdx.x], len = lengths[r];
  if (len == 0) return;
  const int64_t groups = ((int64_t)len + 4) >> 2;
  const int4* __restrict__ base = (const int4*)(diff + off[r]);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < MHAP_REPEAT_BINS; c += PILE_T) bins[c] = 0;
  __syncthreads();
  int32_t carry = 0, top = 0;
  for (int64_t g0 = 0; g0 < groups; g0 += PILE_T * PILE_LOADS) {
    int4 d[PILE_LOADS];
    int32_t c0[PILE_LOADS];
    pile_coverage_tile(base, groups, g0, tid, lane, wave, ws, carry, d, c0);
    int32_t bin = 0;   // a stretch of equal depths goes into its bin at once
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const int64_t p0 = (g0 + j * PILE_T + tid) << 2;
      int32_t c = c0[j];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        c += quad(d[j], k);
        if (p0 + k >= len) continue;
        const int32_t b = c < 0 ? 0 : c > MHAP_REPEAT_BINS - 1 ? MHAP_REPEAT_BINS - 1 : c;
        if (b != bin) {
          if (n) atomicAdd(&bins[bin], n);
          bin = b; n = 0;
        }
        n++;
        if (b > top) top = b;
      }
    }
    if (n) atomicAdd(&bins[bin], n);
    __syncthreads();   // (ws has been read by everyone who comes here)
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const int32_t t = __shfl_down(top, s);
    if (t > top) top = t;
  }
  if (lane == 0) wx[wave] = top;
  __syncthreads();   // (and every add to the bins has been made)
  top = wx[0];
  for (int w = 1; w < PILE_WAVES; w++) if (wx[w] > top) top = wx[w];
  for (int c = tid; c <= top; c += PILE_T)
    if (bins[c]) atomicAdd(hist + c, (u64)bins[c]);
}

// dt = {D, T}: D the smallest c >= 1 with 2 (hist[1] + .. + hist[c]) >= N1, 0 when N1 == 0; T = max_cov or D factor_pct div 100 (at
// most 2^31 - 1, which no depth exceeds)
__global__ __launch_bounds__(256) void depth_kernel(const u64* __restrict__ hist, RParams P, int32_t* __restrict__ dt) {
  __shared__ u64 part[256];
  const int tid = threadIdx.x;
  const int per = MHAP_REPEAT_BINS / 256;
  u64 s = 0;
  for (int k = 0; k < per; k++) {
    const int c = tid * per + k;
    if (c >= 1) s += hist[c];
  }
  part[tid] = s;
  __syncthreads();
  if (tid != 0) return;
  u64 n1 = 0;
  for (int i = 0; i < 256; i++) n1 += part[i];
  int32_t D = 0;
  if (n1 > 0) {
    u64 acc = 0;
    int i = 0;
    while (i < 255 && 2 * (acc + part[i]) < n1) acc += part[i++];   // the 16 bins that hold D
    for (int c = i * per > 1 ? i * per : 1; c < MHAP_REPEAT_BINS; c++) {
      acc += hist[c];
      if (2 * acc >= n1) { D = c; break; }
    }
  }
  const int64_t T = P.max_cov > 0 ? (int64_t)P.max_cov : (int64_t)D * P.factor_pct / 100;
  dt[0] = D;
  dt[1] = T > INT32_MAX ? INT32_MAX : (int32_t)T;
}

struct MaxOp { __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; } };
struct SumOp { __device__ u64 operator()(u64 a, u64 b) const { return a + b; } };

// FILL false: cnt[r], the row, the flag byte and the counts.  FILL true: the intervals of the reads that have some and, next to each,
// the bases of the read's intervals in front of it.
template <bool FILL>
__global__ __launch_bounds__(PILE_T) void mark_kernel(const int32_t* __restrict__ diff, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ lengths, const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ dt, int32_t min_run, int32_t* __restrict__ cnt,
                                                      int32_t* __restrict__ rows, uint8_t* __restrict__ flags, u64* __restrict__ counts,
                                                      const int64_t* __restrict__ offsets, int64_t cap, int2* __restrict__ iv,
                                                      int32_t* __restrict__ cum) {
  __shared__ int32_t ws[PILE_LOADS][PILE_WAVES], wm[PILE_LOADS][PILE_WAVES], wx[PILE_WAVES], wf[PILE_WAVES];
  __shared__ u64 wk[PILE_LOADS][PILE_WAVES], wt[PILE_WAVES];
  const int32_t r = order[blockIdx.x], len = lengths[r];
  int64_t first_slot = 0;
  if (FILL) {
    first_slot = offsets[r];
    if (offsets[r + 1] == first_slot) return;
  }
  const int32_t T = dt[1];
  const int64_t groups = ((int64_t)len + 4) >> 2;
  const int4* __restrict__ base = (const int4*)(diff + off[r]);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t carry = 0, open_begin = -1, top = 0, first = INT32_MAX;
  u64 closed = 0, mine = 0;   // (bases << 32) | intervals: closed in the tiles before, and by this lane
  for (int64_t g0 = 0; g0 < groups; g0 += PILE_T * PILE_LOADS) {
    int4 d[PILE_LOADS];
    int32_t c0[PILE_LOADS], m[PILE_LOADS], cur0[PILE_LOADS];
    pile_coverage_tile(base, groups, g0, tid, lane, wave, ws, carry, d, c0);
    // pass 1: the latest first position of a run in each of the lane's groups
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const int32_t p0 = (int32_t)((g0 + j * PILE_T + tid) << 2);
      int32_t c = c0[j];
      m[j] = -1;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int32_t before = c;
        c += quad(d[j], k);
        if (c > T && !(before > T)) m[j] = p0 + k;
        if (!FILL && c > top) top = c;   // (behind the read the differences are zero and the depth is 0)
      }
    }
    pile_scan_tile(m, lane, wave, wm, open_begin, cur0, MaxOp());   // (its barrier: ws has been read by everyone who comes here)
    // pass 2: every position behind a run's last closes the run that began latest; at most two of a group's four positions do
    int32_t cb[PILE_LOADS][2], ce[PILE_LOADS][2];
    u64 key[PILE_LOADS], ex[PILE_LOADS];
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const int32_t p0 = (int32_t)((g0 + j * PILE_T + tid) << 2);
      int32_t cur = cur0[j], c = c0[j];
      key[j] = 0;
      cb[j][0] = cb[j][1] = ce[j][0] = ce[j][1] = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int32_t before = c;
        c += quad(d[j], k);
        const bool in = c > T, was = before > T;
        if (in && !was) cur = p0 + k;
        if (!in && was && cur >= 0 && p0 + k - cur >= min_run) {
          const int slot = (int)(key[j] & 1);   // (k = 0 or 1 closes the first, k = 2 or 3 the second or the first)
          if (slot == 0) { cb[j][0] = cur; ce[j][0] = p0 + k; } else { cb[j][1] = cur; ce[j][1] = p0 + k; }
          key[j] += ((u64)(uint32_t)(p0 + k - cur) << 32) | 1u;
          if (cur < first) first = cur;
        }
      }
      mine += key[j];
    }
    if (FILL) {
      pile_scan_tile(key, lane, wave, wk, closed, ex, SumOp());   // (its barrier: wm has been read by everyone who comes here)
#pragma unroll
      for (int j = 0; j < PILE_LOADS; j++) {
        const int n = (int)(uint32_t)key[j];
        const int64_t at = first_slot + (int64_t)(uint32_t)ex[j];
        const int32_t before = (int32_t)(ex[j] >> 32);
        if (n > 0 && at < cap) { iv[at] = make_int2(cb[j][0], ce[j][0]); cum[at] = before; }
        if (n > 1 && at + 1 < cap) { iv[at + 1] = make_int2(cb[j][1], ce[j][1]); cum[at + 1] = before + (ce[j][0] - cb[j][0]); }
      }
    }
  }
  if (FILL) return;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    mine += __shfl_down(mine, s);
    const int32_t t = __shfl_down(top, s), f = __shfl_down(first, s);
    if (t > top) top = t;
    if (f < first) first = f;
  }
  if (lane == 0) { wt[wave] = mine; wx[wave] = top; wf[wave] = first; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < PILE_WAVES; w++) {
    mine += wt[w];
    if (wx[w] > top) top = wx[w];
    if (wf[w] < first) first = wf[w];
  }
  const int32_t n = (int32_t)(uint32_t)mine, bases = (int32_t)(mine >> 32);
  const bool whole = n == 1 && first == 0 && bases == len;
  cnt[r] = n;
  ((int4*)rows)[r] = make_int4(n, bases, top, n ? first : -1);
  flags[r] = (uint8_t)((n ? MHAP_REPEAT_SOME : 0) | (whole ? MHAP_REPEAT_WHOLE : 0));
  if (n) {
    atomicAdd(counts + RC_SOME, (u64)1);
    atomicAdd(counts + RC_INTERVALS, (u64)n);
    atomicAdd(counts + RC_REPEAT_BASES, (u64)bases);
  }
  if (whole) atomicAdd(counts + RC_WHOLE, (u64)1);
}

// out: one 16-byte word per record, {keep, uA, uB, 0}
__global__ __launch_bounds__(256) void judge_kernel(const int4* __restrict__ items, int64_t n, const int64_t* __restrict__ offsets,
                                                    const int2* __restrict__ iv, const int32_t* __restrict__ cum, TParams E, int32_t min_unique,
                                                    int4* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
  const int32_t A = w0.x, B = w0.y >> 1;
  if (!trim_eligible(A, B, __hiloint2double(w1.w, w1.z), E)) { out[q] = make_int4(1, -1, -1, 0); return; }
  const int64_t oa = offsets[A], ob = offsets[B];
  const int32_t ua = repeat_unique(iv + oa, cum + oa, offsets[A + 1] - oa, w0.z, w0.w);
  const int32_t ub = repeat_unique(iv + ob, cum + ob, offsets[B + 1] - ob, w1.x, w1.y);
  out[q] = make_int4(ua >= min_unique && ub >= min_unique ? 1 : 0, ua, ub, 0);
}

bool params_ok(const mhap_repeat_params& p) { return p.factor_pct >= 100 && p.max_cov >= 0 && p.min_run >= 1 && p.min_unique >= 0; }

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_repeat_session : Pile {
  static constexpr const char* finish_name = "mhap_repeat_finish";
  static constexpr int unfinished_rc = MHAP_E_INVALID;
  RParams P{};
  TParams E{};   // the add's parameters: eligibility, and the aligned intervals as they are
  bool finished = false;
  int64_t cap = 0, n_intervals = 0;   // the interval slots allocated (the most the reads can have), and those of the last finish
  uint64_t hist[MHAP_REPEAT_BINS] = {0};
  DevBuf d_hist, dt, cnt, offsets, iv, cum, rows, flags, counts, judged;   // counts: MHAP_REPEAT_COUNTS x uint64
  void release() {
    release_pile();
    for (DevBuf* b : {&d_hist, &dt, &cnt, &offsets, &iv, &cum, &rows, &flags, &counts, &judged}) b->release();
  }
};

extern "C" void mhap_repeat_default_params(mhap_repeat_params* p) {
  if (!p) return;
  p->factor_pct = 200; p->max_cov = 0; p->min_run = 500; p->min_unique = 500; p->min_identity = 0.0;
}

extern "C" int mhap_repeat_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_repeat_params* params,
                                 mhap_repeat_session** session) {
  return session_begin("mhap_repeat_begin", h, read_ids, lengths, n_reads, params, mhap_repeat_default_params, params_ok,
                       "factor_pct must be >= 100, max_cov >= 0, min_run >= 1 and min_unique >= 0", session,
                       [&](mhap_repeat_session& s, const mhap_repeat_params& p, const HandleView& v) {
    s.P = RParams{p.factor_pct, p.max_cov, p.min_run, p.min_unique};
    s.E = TParams{1, 0, 0, p.min_identity};
    for (int64_t i = 0; i < n_reads; i++) s.cap += ((int64_t)lengths[i] + 1) / ((int64_t)p.min_run + 1);   // a run and the position behind it
    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1), ni = (size_t)std::max<int64_t>(s.cap, 1);
    Steps q{s.begin_pile(v, h, read_ids, lengths, n_reads), v.stream};
    q.ensure(s.d_hist, 8 * MHAP_REPEAT_BINS);
    q.ensure(s.dt, 8);
    q.ensure(s.cnt, 4 * nr);
    q.ensure(s.offsets, 8 * (nr + 1));
    q.ensure(s.iv, 8 * ni);
    q.ensure(s.cum, 4 * ni);
    q.ensure(s.rows, 16 * nr);
    q.ensure(s.flags, nr);
    q.ensure(s.counts, 8 * MHAP_REPEAT_COUNTS);
    q.zero(s.counts, 8 * MHAP_REPEAT_COUNTS);
    q.zero(s.offsets, 8 * (nr + 1));
    return q.e;
  });
}

extern "C" int mhap_repeat_add(mhap_repeat_session* s, const mhap_record* recs, int64_t n) {
  const char* who = "mhap_repeat_add";
  if (!s) return MHAP_E_INVALID;
  return s->add_records(who, recs, n, s->E, s->counts.as<u64>() + RC_ELIGIBLE);
}

extern "C" int mhap_repeat_finish(mhap_repeat_session* s, int64_t* counts) {
  const char* who = "mhap_repeat_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  s->finished = false;
  hipError_t e;
  u64* d_counts = s->counts.as<u64>();
  // the counts and bins of this finish; the eligible records are summed over the adds and stay
  if ((e = hipMemsetAsync(d_counts, 0, 8 * RC_ELIGIBLE, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if ((e = hipMemsetAsync(s->d_hist.p, 0, 8 * MHAP_REPEAT_BINS, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  const dim3 grid((unsigned)std::max<int64_t>(s->n_reads, 1)), wg(PILE_T);
  const int32_t *diff = s->diff.as<int32_t>(), *lens = s->d_lengths.as<int32_t>(), *order = s->d_order.as<int32_t>(), *dt = s->dt.as<int32_t>();
  const int64_t* off = s->d_off.as<int64_t>();
  if (s->n_reads > 0) hipLaunchKernelGGL(hist_kernel, grid, wg, 0, v.stream, diff, off, lens, order, s->d_hist.as<u64>());
  hipLaunchKernelGGL(depth_kernel, dim3(1), dim3(256), 0, v.stream, s->d_hist.as<u64>(), s->P, s->dt.as<int32_t>());
  if (s->n_reads > 0) {
    hipLaunchKernelGGL(mark_kernel<false>, grid, wg, 0, v.stream, diff, off, lens, order, dt, s->P.min_run, s->cnt.as<int32_t>(),
                       s->rows.as<int32_t>(), s->flags.as<uint8_t>(), d_counts, (const int64_t*)nullptr, (int64_t)0, (int2*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->cnt.as<int32_t>(), s->n_reads, s->offsets.as<int64_t>());
    hipLaunchKernelGGL(mark_kernel<true>, grid, wg, 0, v.stream, diff, off, lens, order, dt, s->P.min_run, (int32_t*)nullptr, (int32_t*)nullptr,
                       (uint8_t*)nullptr, (u64*)nullptr, s->offsets.as<int64_t>(), s->cap, s->iv.as<int2>(), s->cum.as<int32_t>());
  }
  if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
  u64 hc[MHAP_REPEAT_COUNTS];
  int32_t hdt[2] = {0, 0};
  e = hipMemcpyAsync(s->hist, s->d_hist.p, 8 * MHAP_REPEAT_BINS, hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hdt, s->dt.p, sizeof hdt, hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hc, d_counts, sizeof hc, hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);   // the one wait of a finish
  if (e != hipSuccess) return hip_fail(v, who, "download", e);
  if (es != hipSuccess) return hip_fail(v, who, "kernel", es);
  s->reap(true);   // the stream is empty: every upload has been read
  if (s->P.max_cov == 0 && hdt[0] == MHAP_REPEAT_BINS - 1) {
    *v.err = std::string(who) + ": the typical depth reaches the last of the " + std::to_string(MHAP_REPEAT_BINS) +
             " bins, which holds every greater depth too: give max_cov";
    return MHAP_E_INVALID;
  }
  for (int k = 0; k < MHAP_REPEAT_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[RC_READS] = s->n_reads;
  counts[RC_BASES] = s->bases_in;
  counts[RC_D] = hdt[0];
  counts[RC_T] = s->P.max_cov > 0 ? (int64_t)s->P.max_cov : (int64_t)hdt[0] * s->P.factor_pct / 100;
  s->n_intervals = (int64_t)hc[RC_INTERVALS];
  s->finished = true;
  return MHAP_OK;
}

extern "C" int mhap_repeat_copy(mhap_repeat_session* s, int32_t* rows, uint8_t* flags, int64_t* offsets, int32_t* intervals) {
  const char* who = "mhap_repeat_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = check_finished(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!offsets || (s->n_reads > 0 && (!rows || !flags)) || (s->n_intervals > 0 && !intervals)) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  rc = s->download(who, offsets, s->offsets.p, 8 * ((size_t)s->n_reads + 1));
  if (rc == MHAP_OK && s->n_reads > 0) rc = s->download(who, rows, s->rows.p, 16 * (size_t)s->n_reads);
  if (rc == MHAP_OK && s->n_reads > 0) rc = s->download(who, flags, s->flags.p, (size_t)s->n_reads);
  if (rc == MHAP_OK && s->n_intervals > 0) rc = s->download(who, intervals, s->iv.p, 8 * (size_t)s->n_intervals);
  return rc;
}

extern "C" int mhap_repeat_histogram(mhap_repeat_session* s, int64_t* bins) {
  const char* who = "mhap_repeat_histogram";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = check_finished(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!bins) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  for (int c = 0; c < MHAP_REPEAT_BINS; c++) bins[c] = (int64_t)s->hist[c];
  return MHAP_OK;
}

extern "C" int mhap_repeat_apply(mhap_repeat_session* s, const mhap_record* in, int64_t n, uint8_t* keep, int32_t* unique) {
  const char* who = "mhap_repeat_apply";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  std::vector<GItem> items;
  int rc = apply_begin(s, v, who, in, n, keep && unique, items, s->judged, 16 * (size_t)n, "hipMalloc of the records");
  if (rc != MHAP_OK || n == 0) return rc;
  hipLaunchKernelGGL(judge_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, s->items.as<int4>(), n, s->offsets.as<int64_t>(), s->iv.as<int2>(),
                     s->cum.as<int32_t>(), s->E, s->P.min_unique, s->judged.as<int4>());
  std::vector<int32_t> got(4 * (size_t)n);
  if ((rc = apply_end(v, who, got.data(), s->judged, 16 * (size_t)n)) != MHAP_OK) return rc;
  for (int64_t q = 0; q < n; q++) {
    keep[q] = (uint8_t)got[4 * (size_t)q];
    unique[2 * q] = got[4 * (size_t)q + 1];
    unique[2 * q + 1] = got[4 * (size_t)q + 2];
  }
  return MHAP_OK;
}

extern "C" int mhap_repeat_judge_record(const mhap_record* in, const int32_t* intervalsA, int64_t nA, const int32_t* intervalsB, int64_t nB,
                                        const mhap_repeat_params* params, int32_t* unique) {
  if (!in || nA < 0 || nB < 0 || (nA > 0 && !intervalsA) || (nB > 0 && !intervalsB)) return -1;
  mhap_repeat_params p;
  mhap_repeat_default_params(&p);
  if (params) p = *params;
  if (!params_ok(p)) return -1;
  const int32_t* lists[2] = {intervalsA, intervalsB};
  const int64_t ns[2] = {nA, nB};
  const int32_t lens[2] = {in->alen, in->blen}, x1[2] = {in->a1, in->b1}, x2[2] = {in->a2, in->b2};
  int32_t u[2] = {-1, -1};
  const bool el = trim_eligible(in->from_id, in->to_id, in->score, TParams{1, 0, 0, p.min_identity});
  for (int f = 0; f < 2; f++) {
    std::vector<int2> iv((size_t)ns[f]);
    std::vector<int32_t> cum((size_t)ns[f]);
    int64_t prev = 0, sum = 0;
    for (int64_t i = 0; i < ns[f]; i++) {   // ascending, disjoint, not empty, inside the read
      const int32_t b = lists[f][2 * i], e = lists[f][2 * i + 1];
      if (b < prev || e <= b || e > lens[f]) return -1;
      iv[(size_t)i] = make_int2(b, e);
      cum[(size_t)i] = (int32_t)sum;
      sum += e - b; prev = e;
    }
    if (!el) continue;
    if (x1[f] < 0 || x2[f] < x1[f] || x2[f] >= lens[f]) return -1;
    u[f] = repeat_unique(iv.data(), cum.data(), ns[f], x1[f], x2[f]);
  }
  if (unique) { unique[0] = u[0]; unique[1] = u[1]; }
  return !el || (u[0] >= p.min_unique && u[1] >= p.min_unique) ? 1 : 0;
}

extern "C" void mhap_repeat_free(mhap_repeat_session* s) { session_free(s); }
