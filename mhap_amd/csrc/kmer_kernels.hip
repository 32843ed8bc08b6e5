// kmer_kernels.hip — exact k-mer counting (k <= 16) on the GPU: what the `-f` repeat filter file is made from.
//
// MHAP reads the filter and never writes it (J/sketch/FrequencyCounts.java:63-200).  This counts every window of the reads, as the
// ingest delivers them (2-bit codes of pure reads, upper-cased bytes of the others), in three kernels per ingest group and one per flush:
//   1. kmer_hist_kernel     one wave per read; the canonical values rolled forward and reverse-complement together; a histogram of
//                           the value's top 2k - L bits (the bucket) in global memory (at most 2^17 words; one global atomic per window)
//   2. kmer_scan_kernel     exclusive scan of that histogram: where each bucket's segment of this group starts in the staging arena
//   3. kmer_hist_kernel<1>  the same walk again; the low L bits of every window (2 bytes) go to its bucket's segment (a global
//                           atomic on the bucket's cursor per window: these two passes are 96 % of the device time, EXPERIMENTS.md)
//   4. kmer_count_kernel    one workgroup per bucket: the bucket's 2^L counters in LDS (128 KiB at L = 15), the counts kept from earlier
//                           flushes and the bucket's segments of every staged group folded in with LDS atomics; then either the kept
//                           counts are written back (sparse: (low bits, count) of the values seen), or, at finish, the bucket's distinct
//                           values are counted and the (value, count) pairs at or above the line threshold are emitted; the
//                           histogram finish (kmer_count_kernel<2>) also bins every final count: counts 1..4096 in LDS, merged into
//                           a global histogram by nonzero bin, larger counts to a tail list (one entry per value)
// Each bucket is owned by one workgroup, so the counts need no global atomics.  Staging is 2 bytes per window; it is flushed into the
// kept counts when the next group would pass a budget (a quarter of the free HBM), so every allocation is sized by the input.
//
// Sequence assessment sits on the same counts (the second half of this file): kmer_set_kernel ends a count as a bitmap of 4^k bits (step
// 4's fold, then the values counted often enough, a ballot per word), kmer_eval_kernel walks arbitrary sequences against such a bitmap
// (a wave per tile of 4 032 positions: windows valid, present or missing, runs of missing ones, bases no present window covers),
// kmer_eval_intervals_kernel turns the uncovered bases into intervals, kmer_set_compare_kernel counts two bitmaps and their intersection.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"

namespace mhap {

// ---- window arithmetic (host and device) -------------------------------------------------------------------------------------
// 2 bits per base, A=0 C=1 G=2 T=3, first base most significant; canonical = min(value, value of the reverse complement).
struct KmerRoll {
  uint32_t fwd = 0, rc = 0;
  int run = 0;   // valid bases in a row up to the last one pushed
};
// byte -> code; true when the byte is one of A, C, G, T (the ingest upper-cases, so other bytes are N / IUPAC / anything else)
__host__ __device__ inline bool kmer_code(uint32_t c, uint32_t& code) {
  const uint32_t x = (c >> 1) & 3u;
  code = x ^ (x >> 1);
  return ((0x54474341u >> (8 * code)) & 0xFFu) == c;
}
__host__ __device__ inline uint32_t kmer_mask(int k) { return k >= 16 ? 0xFFFFFFFFu : ((1u << (2 * k)) - 1u); }
__host__ __device__ inline void kmer_push(KmerRoll& r, uint32_t code, bool valid, int k, uint32_t mask) {
  r.fwd = ((r.fwd << 2) | code) & mask;
  r.rc = (r.rc >> 2) | ((3u - code) << (2 * (k - 1)));
  r.run = valid ? r.run + 1 : 0;
}
__host__ __device__ inline uint32_t kmer_value(const KmerRoll& r, bool canonical) { return canonical && r.rc < r.fwd ? r.rc : r.fwd; }   // (unsigned: min() may pick an int overload)
// low bits per bucket: 15 at k >= 12 (2^15 LDS counters), fewer below so that there are >= 256 buckets where 4^k allows
__host__ __device__ inline int kmer_low_bits(int k) { return min(15, max(0, 2 * k - 8)); }

constexpr int KC_THREADS = 256;     // hist / scatter workgroups: 4 waves, one read per wave at a time
constexpr int KC_COUNT_THREADS = 1024;
constexpr int KC_SCAN_THREADS = 1024;
constexpr int KC_LDS = 1 << 15;
constexpr int KC_HIST_DENSE = 4096;  // histogram finish: counts 1..4096 binned in LDS (16 KiB beside cnt[]'s 128 KiB: one workgroup per CU either way)

// The windows [s, e) of the lane's share of read rd, each passed to emit(value).
template <class F>
__device__ inline void kmer_walk(const uint8_t* __restrict__ store, const ReadDesc& rd, int k, bool canonical, uint32_t mask, int lane, F&& emit) {
  const int nw = rd.length - k + 1;
  if (nw <= 0 || (rd.flags & MHAP_RD_SKIP)) return;
  const int chunk = (nw + MHAP_WAVE - 1) / MHAP_WAVE;
  const int s = lane * chunk;
  if (s >= nw) return;
  const int e = min(nw, s + chunk) + k - 1;   // bases [s, e)
  const uint32_t* __restrict__ W = (const uint32_t*)(store + rd.base_off);
  KmerRoll r;
  uint32_t w = 0;
  if (rd.flags & MHAP_RD_RAW) {
    for (int p = s; p < e; p++) {
      if (p == s || (p & 3) == 0) w = W[p >> 2];
      uint32_t code;
      const bool ok = kmer_code((w >> (8 * (p & 3))) & 0xFFu, code);
      kmer_push(r, code, ok, k, mask);
      if (r.run >= k) emit(kmer_value(r, canonical));
    }
  } else {
    for (int p = s; p < e; p++) {
      if (p == s || (p & 15) == 0) w = W[p >> 4];
      kmer_push(r, (w >> (2 * (p & 15))) & 3u, true, k, mask);
      if (r.run >= k) emit(kmer_value(r, canonical));
    }
  }
}

// Steps 1 and 3.  SCATTER = 0: hist[bucket]++; SCATTER = 1: stage[base + cursor[bucket]++] = low bits.
template <int SCATTER>
__global__ __launch_bounds__(KC_THREADS) void kmer_hist_kernel(const uint8_t* __restrict__ store, const ReadDesc* __restrict__ descs, int64_t n, int k,
                                                               int canonical, int L, uint32_t* __restrict__ hist, uint16_t* __restrict__ stage, uint64_t base) {
  const int lane = threadIdx.x & (MHAP_WAVE - 1);
  const int64_t wave = ((int64_t)blockIdx.x * KC_THREADS + threadIdx.x) / MHAP_WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * (KC_THREADS / MHAP_WAVE);
  const uint32_t mask = kmer_mask(k), lowm = (1u << L) - 1u;
  for (int64_t r = wave; r < n; r += nwaves) {
    const ReadDesc rd = descs[r];
    kmer_walk(store, rd, k, canonical != 0, mask, lane, [&](uint32_t v) {
      if (SCATTER) {
        const uint32_t at = atomicAdd(hist + (v >> L), 1u);
        stage[base + at] = (uint16_t)(v & lowm);
      } else {
        atomicAdd(hist + (v >> L), 1u);
      }
    });
  }
}

// Exclusive scan of n items by one workgroup: item(i) -> uint64, out(i, exclusive prefix); the last thread writes the sum to *total.
template <class In, class Out>
__device__ inline void kc_block_scan(int64_t n, In item, Out out, unsigned long long* total) {
  __shared__ unsigned long long wsum[KC_SCAN_THREADS / MHAP_WAVE];
  const int t = threadIdx.x, lane = t & (MHAP_WAVE - 1), wv = t / MHAP_WAVE;
  const int64_t chunk = (n + KC_SCAN_THREADS - 1) / KC_SCAN_THREADS;
  const int64_t lo = min(n, (int64_t)t * chunk), hi = min(n, lo + chunk);
  unsigned long long mine = 0;
  for (int64_t i = lo; i < hi; i++) mine += item(i);
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < MHAP_WAVE; off <<= 1) { const unsigned long long v = __shfl_up(incl, off); if (lane >= off) incl += v; }
  if (lane == MHAP_WAVE - 1) wsum[wv] = incl;
  __syncthreads();
  unsigned long long run = incl - mine;
  for (int w = 0; w < wv; w++) run += wsum[w];
  for (int64_t i = lo; i < hi; i++) { const unsigned long long v = item(i); out(i, run); run += v; }
  if (t == KC_SCAN_THREADS - 1) *total = run;
}

// Step 2 for group g: segs[g][b] = base + start of bucket b's segment (segs[g][NB] = its end), hist[b] = that start within the group
// (the scatter's cursors),
// flush_n[b] += windows of bucket b, *total = the group's windows.
__global__ __launch_bounds__(KC_SCAN_THREADS) void kmer_scan_kernel(uint32_t* __restrict__ hist, int NB, uint64_t* __restrict__ seg_row, uint64_t base,
                                                                    unsigned long long* __restrict__ flush_n, unsigned long long* __restrict__ total) {
  kc_block_scan(NB, [&](int64_t i) { return (unsigned long long)hist[i]; },
                [&](int64_t i, unsigned long long ex) {
                  flush_n[i] += hist[i];
                  seg_row[i] = base + ex;
                  hist[i] = (uint32_t)ex;
                }, total);
  __syncthreads();
  if (threadIdx.x == KC_SCAN_THREADS - 1) seg_row[NB] = base + *total;
}

// Before a flush that keeps its counts: room for bucket b's kept entries = min(kept_n[b] + flush_n[b], 2^L), laid out back to back.
__global__ __launch_bounds__(KC_SCAN_THREADS) void kmer_kept_room_kernel(const uint32_t* __restrict__ kept_n, const unsigned long long* __restrict__ flush_n,
                                                                         int NB, int L, uint64_t* __restrict__ off, unsigned long long* __restrict__ total) {
  kc_block_scan(NB, [&](int64_t i) { return min((unsigned long long)kept_n[i] + flush_n[i], 1ULL << L); },
                [&](int64_t i, unsigned long long ex) { off[i] = ex; }, total);
}

struct KcCountArgs {
  const uint16_t* stage; const uint64_t* segs; int ngroups; int NB; int L;
  const uint2* kept; const uint64_t* kept_off; const uint32_t* kept_n;      // counts kept so far: (low bits, count)
  uint2* kept_out; const uint64_t* kept_out_off; uint32_t* kept_out_n;      // FINISH = 0: the counts to keep
  uint32_t* distinct; uint2* sel; unsigned long long* nsel; uint64_t sel_cap; uint32_t thr;   // FINISH = 1: (value, count >= thr)
  int* overflow;
  // FINISH = 2, the histogram: dense[c - 1] += distinct values with count c (c <= KC_HIST_DENSE, merged by nonzero bin); every count
  // above that goes to tail[] (at most total / (KC_HIST_DENSE + 1) entries: each such value holds more than KC_HIST_DENSE windows)
  unsigned long long* dense; uint32_t* tail; unsigned long long* ntail; uint64_t tail_cap;
};

// The fold of step 4 into bucket b's zeroed LDS counters: the counts kept from earlier flushes, then the bucket's segment of every
// staged group.  True in a thread that saw a counter wrap.
__device__ inline bool kc_fold(const KcCountArgs& a, uint32_t* cnt, int b, int t) {
  const uint64_t k0 = a.kept_off[b];
  const uint32_t kn = a.kept_n[b];
  for (uint32_t i = t; i < kn; i += KC_COUNT_THREADS) { const uint2 e = a.kept[k0 + i]; cnt[e.x] = e.y; }   // (distinct low bits: no two threads meet)
  __syncthreads();
  bool over = false;
  for (int g = 0; g < a.ngroups; g++) {
    const uint64_t* row = a.segs + (size_t)g * (a.NB + 1);
    const uint64_t s = row[b], e = row[b + 1];
    for (uint64_t i = s + t; i < e; i += KC_COUNT_THREADS) over |= atomicAdd(&cnt[a.stage[i]], 1u) == 0xFFFFFFFFu;
  }
  return over;
}

// Step 4: one workgroup per bucket.  FINISH = 0: a flush, 1: the finish, 2: the finish with the histogram.
template <int FINISH>
__global__ __launch_bounds__(KC_COUNT_THREADS) void kmer_count_kernel(KcCountArgs a) {
  __shared__ uint32_t cnt[KC_LDS];
  __shared__ uint32_t cursor;
  __shared__ uint32_t bins[FINISH == 2 ? KC_HIST_DENSE : 1];   // (unused below FINISH = 2, so not allocated there)
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (MHAP_WAVE - 1);
  const int nv = 1 << a.L;
  for (int i = t; i < nv; i += KC_COUNT_THREADS) cnt[i] = 0u;
  if constexpr (FINISH == 2) {
    for (int i = t; i < KC_HIST_DENSE; i += KC_COUNT_THREADS) bins[i] = 0u;
  }
  if (t == 0) cursor = 0u;
  __syncthreads();
  if (kc_fold(a, cnt, b, t)) *a.overflow = 1;
  __syncthreads();
  for (int i0 = 0; i0 < nv; i0 += KC_COUNT_THREADS) {
    const int i = i0 + t;
    const uint32_t c = i < nv ? cnt[i] : 0u;
    const bool pick = FINISH ? a.sel_cap > 0 && c >= a.thr && c > 0u : c > 0u;
    const unsigned long long m = __ballot(pick);
    if (FINISH) {
      const unsigned long long nz = __ballot(c > 0u);
      if (lane == 0 && nz) atomicAdd(&cursor, (uint32_t)__popcll(nz));
    }
    if constexpr (FINISH == 2) {
      // count 1, the most common one, once per wave; the other dense counts one LDS atomic per value; the rest to the tail
      const unsigned long long ones = __ballot(c == 1u), big = __ballot(c > (uint32_t)KC_HIST_DENSE);
      if (lane == 0 && ones) atomicAdd(&bins[0], (uint32_t)__popcll(ones));
      if (c > 1u && c <= (uint32_t)KC_HIST_DENSE) atomicAdd(&bins[c - 1u], 1u);
      if (big) {
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(a.ntail, (unsigned long long)__popcll(big));
        at = __shfl(at, 0) + (unsigned long long)__popcll(big & ((1ULL << lane) - 1ULL));
        if (c > (uint32_t)KC_HIST_DENSE && at < a.tail_cap) a.tail[at] = c;
      }
    }
    if (!m) continue;
    const uint32_t before = (uint32_t)__popcll(m & ((1ULL << lane) - 1ULL));
    if (FINISH) {
      unsigned long long at = 0;
      if (lane == 0) at = atomicAdd(a.nsel, (unsigned long long)__popcll(m));
      at = __shfl(at, 0);
      if (pick && at + before < a.sel_cap) a.sel[at + before] = make_uint2(((uint32_t)b << a.L) | (uint32_t)i, c);
    } else {
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(&cursor, (uint32_t)__popcll(m));
      at = __shfl(at, 0);
      if (pick) a.kept_out[a.kept_out_off[b] + at + before] = make_uint2((uint32_t)i, c);
    }
  }
  __syncthreads();
  if constexpr (FINISH == 2) {
    for (int i = t; i < KC_HIST_DENSE; i += KC_COUNT_THREADS) {
      const uint32_t n = bins[i];
      if (n) atomicAdd(a.dense + i, (unsigned long long)n);
    }
  }
  if (t == 0) {
    if (FINISH) a.distinct[b] = cursor;
    else a.kept_out_n[b] = cursor;
  }
}

// ---- the set of the solid k-mers and sequences walked against it (sequence assessment) --------------------------------------------
// The set finish: step 4's fold, then bit v of a bitmap of 4^k bits = (final count of v >= thr).  Value v = (b << L) | i sits in 64-bit
// word v >> 6 at bit v & 63, so a wave's ballot over 64 consecutive i is one whole word with one writer; a bucket narrower than a word
// (L < 6) ORs its bits into the zeroed word it shares with its neighbours.  distinct[b] as at the finish; *members += the bucket's bits.
__global__ __launch_bounds__(KC_COUNT_THREADS) void kmer_set_kernel(KcCountArgs a, uint64_t thr, unsigned long long* __restrict__ bits,
                                                                    unsigned long long* __restrict__ members) {
  __shared__ uint32_t cnt[KC_LDS];
  __shared__ uint32_t ndistinct, nmembers;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (MHAP_WAVE - 1);
  const int nv = 1 << a.L;
  for (int i = t; i < nv; i += KC_COUNT_THREADS) cnt[i] = 0u;
  if (t == 0) { ndistinct = 0u; nmembers = 0u; }
  __syncthreads();
  if (kc_fold(a, cnt, b, t)) *a.overflow = 1;
  __syncthreads();
  for (int i0 = 0; i0 < nv; i0 += KC_COUNT_THREADS) {
    const int i = i0 + t;
    const uint32_t c = i < nv ? cnt[i] : 0u;
    const unsigned long long in = __ballot(c > 0u && (uint64_t)c >= thr), nz = __ballot(c > 0u);
    if (lane == 0 && i < nv) {
      if (nz) atomicAdd(&ndistinct, (uint32_t)__popcll(nz));
      if (in) atomicAdd(&nmembers, (uint32_t)__popcll(in));
      const uint64_t v0 = ((uint64_t)b << a.L) | (uint64_t)i;   // the value of this wave's first counter
      if (nv >= MHAP_WAVE) bits[v0 >> 6] = in;
      else if (in) atomicOr(bits + (v0 >> 6), in << (v0 & 63u));
    }
  }
  __syncthreads();
  if (t == 0) {
    a.distinct[b] = ndistinct;
    if (nmembers) atomicAdd(members, (unsigned long long)nmembers);
  }
}

// out[i] = 1 when the set holds values[i] (a value outside the 4^k values of the set: 0)
__global__ __launch_bounds__(KC_THREADS) void kmer_set_contains_kernel(const uint32_t* __restrict__ bits, int k, const uint64_t* __restrict__ values, int64_t n,
                                                                       uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint64_t v = values[i];
  out[i] = v < (1ULL << (2 * k)) ? (uint8_t)((bits[v >> 5] >> (v & 31u)) & 1u) : (uint8_t)0;
}

// out[0], out[1], out[2] += the bits of a, of b and of a & b over n16 16-byte pieces of the two bitmaps
__global__ __launch_bounds__(KC_THREADS) void kmer_set_compare_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, int64_t n16,
                                                                      unsigned long long* __restrict__ out) {
  unsigned long long ca = 0, cb = 0, cab = 0;
  const int64_t step = (int64_t)gridDim.x * KC_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * KC_THREADS + threadIdx.x; i < n16; i += step) {
    const uint4 x = a[i], y = b[i];
    ca += (unsigned)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w));
    cb += (unsigned)(__popc(y.x) + __popc(y.y) + __popc(y.z) + __popc(y.w));
    cab += (unsigned)(__popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w));
  }
#pragma unroll
  for (int off = MHAP_WAVE / 2; off > 0; off >>= 1) { ca += __shfl_xor(ca, off); cb += __shfl_xor(cb, off); cab += __shfl_xor(cab, off); }
  if ((threadIdx.x & (MHAP_WAVE - 1)) == 0) {
    if (ca) atomicAdd(out, ca);
    if (cb) atomicAdd(out + 1, cb);
    if (cab) atomicAdd(out + 2, cab);
  }
}

// Sequences against a set.  A window is named by its LAST base j (it starts at j - k + 1), so bit b of a lane's masks is both the
// window that ends at base s + b and the position s + b.  One wave takes a tile of KE_TILE positions of one sequence: lane l walks
// the KE_LANE positions from s = tile start + 64 l after a warm-up of KE_WARM bases (>= k - 1, so no lane needs a state of the lane
// before it) and keeps two masks, V (valid windows) and P (valid windows the set holds).  Everything a position needs from elsewhere
// lies AFTER it — the k - 1 windows that also contain it, the window that would continue a missing run — and comes from the next lane
// by one shuffle; lane 63 walks the first 64 positions of the next tile for that purpose alone and counts nothing, so no pass
// stitches tiles.  Bases before the sequence or past its end are invalid, which makes their windows invalid and their positions uncovered.
constexpr int KE_LANE = 64;
constexpr int KE_TILE = 63 * KE_LANE;
constexpr int KE_WARM = 16;
constexpr int KE_BATCH = 32;    // bitmap lookups issued together (dependent random loads: all of a batch are in flight before the first use)
constexpr int KE_THREADS = 256;

// OR over d in [0, k) of (hi:lo >> d), low 64 bits: position p is covered when a window that ends in [p, p + k) is set (k <= 16)
__host__ __device__ inline unsigned long long ke_cover(unsigned long long lo, unsigned long long hi, int k) {
  int w = 1;   // lo and hi hold the OR over d in [0, w)
  while (2 * w <= k) { lo |= (lo >> w) | (hi << (64 - w)); hi |= hi >> w; w *= 2; }
  const int r = k - w;
  if (r > 0) lo |= (lo >> r) | (hi << (64 - r));
  return lo;
}

// V and P of the windows that end at bases [s, s + 64) of a sequence of n bases stored at W (s a multiple of 64)
template <bool RAW>
__host__ __device__ inline void ke_lane_states(const uint32_t* __restrict__ W, int64_t s, int n, int k, bool canonical, const uint32_t* __restrict__ bits,
                                      unsigned long long& V, unsigned long long& P) {
  constexpr int PER = RAW ? 4 : 16, NW = (KE_WARM + KE_LANE) / PER;   // bases per dword; dwords of the bases [s - 16, s + 64)
  const int64_t w0 = (s - KE_WARM) / PER, nwords = ((int64_t)n + PER - 1) / PER;
  uint32_t bw[NW];
#pragma unroll
  for (int i = 0; i < NW; i++) { const int64_t d = w0 + i; bw[i] = d >= 0 && d < nwords ? W[d] : 0u; }
  // base s + rel is in the sequence for rel in [lo, hi) (s = 0: nothing before it; a packed dword's padding decodes as A)
  const int lo = s == 0 ? 0 : -KE_WARM, hi = (int64_t)n - s < KE_LANE ? (int)((int64_t)n - s) : KE_LANE;
  const uint32_t mask = kmer_mask(k);
  KmerRoll r;
  auto push = [&](int q) {   // base s - 16 + q
    uint32_t code;
    bool ok = true;
    if (RAW) ok = kmer_code((bw[q >> 2] >> (8 * (q & 3))) & 0xFFu, code);
    else code = (bw[q >> 4] >> (2 * (q & 15))) & 3u;
    kmer_push(r, code, ok && q - KE_WARM >= lo && q - KE_WARM < hi, k, mask);
  };
#pragma unroll
  for (int q = 0; q < KE_WARM; q++) push(q);
  V = 0; P = 0;
#pragma unroll
  for (int h = 0; h < KE_LANE / KE_BATCH; h++) {
    uint32_t val[KE_BATCH], word[KE_BATCH], vm = 0, pm = 0;
#pragma unroll
    for (int j = 0; j < KE_BATCH; j++) {
      push(KE_WARM + h * KE_BATCH + j);
      const bool ok = r.run >= k;
      val[j] = ok ? kmer_value(r, canonical) : 0u;
      vm |= (ok ? 1u : 0u) << j;
    }
#pragma unroll
    for (int j = 0; j < KE_BATCH; j++) word[j] = bits[val[j] >> 5];
#pragma unroll
    for (int j = 0; j < KE_BATCH; j++) pm |= ((word[j] >> (val[j] & 31u)) & 1u) << j;
    V |= (unsigned long long)vm << (h * KE_BATCH);
    P |= (unsigned long long)(pm & vm) << (h * KE_BATCH);
  }
}

// What a lane counts from its masks and the next lane's: packed as windows | missing << 16 | runs << 32 | unsupported << 48 (a wave's
// sums are at most KE_TILE each), and U, the unsupported ones of its 64 positions.
__host__ __device__ inline unsigned long long ke_lane_counts(unsigned long long V, unsigned long long P, unsigned long long nV, unsigned long long nP, int k,
                                                             unsigned long long& U) {
  const unsigned long long M = V & ~P, nM = nV & ~nP;
  const unsigned long long ends = M & ~((M >> 1) | (nM << 63));   // a missing run ends where the next window is not missing
  U = ke_cover(V, nV, k) & ~ke_cover(P, nP, k);
  return (unsigned long long)__builtin_popcountll(V) | ((unsigned long long)__builtin_popcountll(M) << 16) |
         ((unsigned long long)__builtin_popcountll(ends) << 32) | ((unsigned long long)__builtin_popcountll(U) << 48);
}

struct KeArgs {
  const uint8_t* store; const ReadDesc* descs;
  const int32_t* tile_seq; const int64_t* tile_first; int64_t ntiles;   // tile w belongs to sequence tile_seq[w], whose tiles start at tile_first[]
  const uint32_t* bits; int k; int canonical;
  unsigned long long* rows;    // [sequence][4]: windows, missing, runs, unsupported
  unsigned long long* umask;   // [tile][63]: the unsupported positions, a bit each (the tiles of a sequence are in a row: its positions in order)
};

__global__ __launch_bounds__(KE_THREADS) void kmer_eval_kernel(KeArgs a) {
  const int lane = threadIdx.x & (MHAP_WAVE - 1);
  const int64_t w = ((int64_t)blockIdx.x * KE_THREADS + threadIdx.x) / MHAP_WAVE;
  if (w >= a.ntiles) return;
  const int seq = a.tile_seq[w];
  const ReadDesc rd = a.descs[seq];
  const int64_t s = (w - a.tile_first[seq]) * KE_TILE + (int64_t)lane * KE_LANE;
  const uint32_t* __restrict__ W = (const uint32_t*)(a.store + rd.base_off);
  unsigned long long V, P;
  if (rd.flags & MHAP_RD_RAW) ke_lane_states<true>(W, s, rd.length, a.k, a.canonical != 0, a.bits, V, P);
  else ke_lane_states<false>(W, s, rd.length, a.k, a.canonical != 0, a.bits, V, P);
  const unsigned long long nV = __shfl_down(V, 1), nP = __shfl_down(P, 1);   // (lane 63 gets its own: it counts nothing)
  unsigned long long U;
  unsigned long long sum = ke_lane_counts(V, P, nV, nP, a.k, U);
  if (lane == MHAP_WAVE - 1) sum = 0;
#pragma unroll
  for (int off = MHAP_WAVE / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if (lane < MHAP_WAVE - 1) a.umask[w * (MHAP_WAVE - 1) + lane] = U;
  if (lane == 0) {
    unsigned long long* row = a.rows + (size_t)seq * 4;
#pragma unroll
    for (int f = 0; f < 4; f++) { const unsigned long long c = (sum >> (16 * f)) & 0xFFFFu; if (c) atomicAdd(row + f, c); }
  }
}

// The intervals of unsupported positions from the bit per position: a wave per tile.  FILL = 0 counts the tile's interval begins and
// ends; after a prefix sum of each, FILL = 1 writes them: begins and ends are both in position order, so the i-th begin and the i-th
// end are one interval, whichever tiles they lie in.  iv: (seq0 + sequence, begin, end) per interval, as the host hands them out.
template <int FILL>
__global__ __launch_bounds__(KE_THREADS) void kmer_eval_intervals_kernel(const unsigned long long* __restrict__ umask, const int32_t* __restrict__ tile_seq,
                                                                         const int64_t* __restrict__ tile_first, int64_t ntiles, int32_t* __restrict__ nbegin,
                                                                         int32_t* __restrict__ nend, const int64_t* __restrict__ at_begin,
                                                                         const int64_t* __restrict__ at_end, int64_t seq0, int64_t* __restrict__ iv) {
  constexpr int WORDS = MHAP_WAVE - 1;
  const int lane = threadIdx.x & (MHAP_WAVE - 1);
  const int64_t w = ((int64_t)blockIdx.x * KE_THREADS + threadIdx.x) / MHAP_WAVE;
  if (w >= ntiles) return;
  const int seq = tile_seq[w];
  const int64_t first = tile_first[seq] * WORDS, last = tile_first[seq + 1] * WORDS, g = w * WORDS + lane;   // the sequence's words
  unsigned long long U = 0, before = 0, after = 0;
  if (lane < WORDS) {
    U = umask[g];
    if (g > first) before = umask[g - 1];
    if (g + 1 < last) after = umask[g + 1];
  }
  const unsigned long long B = U & ~((U << 1) | (before >> 63)), E = U & ~((U >> 1) | (after << 63));
  const uint32_t mine = (uint32_t)__popcll(B) | ((uint32_t)__popcll(E) << 16);   // (at most 32 of each per word)
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < MHAP_WAVE; off <<= 1) { const uint32_t u = __shfl_up(incl, off); if (lane >= off) incl += u; }
  if (!FILL) {
    if (lane == MHAP_WAVE - 1) { nbegin[w] = (int32_t)(incl & 0xFFFFu); nend[w] = (int32_t)(incl >> 16); }
    return;
  }
  const uint32_t ex = incl - mine;
  const int32_t p0 = (int32_t)((g - first) * KE_LANE);   // the position of bit 0
  int64_t o = at_begin[w] + (ex & 0xFFFFu);
  for (unsigned long long m = B; m; m &= m - 1) { iv[3 * o] = seq0 + seq; iv[3 * o + 1] = p0 + (__ffsll((long long)m) - 1); o++; }
  o = at_end[w] + (ex >> 16);
  for (unsigned long long m = E; m; m &= m - 1) { iv[3 * o + 2] = p0 + __ffsll((long long)m); o++; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct KmerCountState {
  int k = 16, canonical = 1, L = 15, NB = 1;
  uint64_t index_gen = 0;
  int64_t total = 0;            // windows counted
  int ngroups = 0;              // groups staged since the last flush
  uint64_t arena_used = 0;      // windows staged since the last flush
  uint64_t budget = 0;          // windows staged before a flush
  int flushes = 0;
  DevBuf store, descs, hist, segs, flush_n, arena, kept, kept_off, kept_n, kept2, kept2_off, kept2_n, scalars, distinct, sel, hdense, htail;
  ~KmerCountState() {
    DevBuf* bufs[] = {&store, &descs, &hist, &segs, &flush_n, &arena, &kept, &kept_off, &kept_n, &kept2, &kept2_off, &kept2_n, &scalars, &distinct, &sel,
                      &hdense, &htail};
    for (DevBuf* b : bufs) b->release();
  }
};

namespace {

#define KCHK(v, expr)                                                                                       \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess) {                                                                                 \
      *(v).err = std::string(#expr) + ": " + hipGetErrorString(_e);                                         \
      return _e == hipErrorOutOfMemory ? MHAP_E_NOMEM : MHAP_E_HIP;                                         \
    }                                                                                                       \
  } while (0)

bool kc_prof() { return getenv("MHAP_HOST_PROF") != nullptr; }

// scalars: [0] group total, [1] kept room total, [2] selected pairs, [3] overflow flag (as int), [4] histogram tail entries
int kc_flush(KmerCountState& S, const HandleView& v) {
  if (S.ngroups == 0) return MHAP_OK;
  hipStream_t st = v.stream;
  unsigned long long* sc = S.scalars.as<unsigned long long>();
  kmer_kept_room_kernel<<<1, KC_SCAN_THREADS, 0, st>>>(S.kept_n.as<uint32_t>(), S.flush_n.as<unsigned long long>(), S.NB, S.L, S.kept2_off.as<uint64_t>(), sc + 1);
  KCHK(v, hipGetLastError());
  unsigned long long room = 0;
  KCHK(v, hipMemcpyAsync(&room, sc + 1, 8, hipMemcpyDeviceToHost, st));
  KCHK(v, hipStreamSynchronize(st));
  KCHK(v, S.kept2.ensure(std::max<size_t>(room, 1) * sizeof(uint2)));
  KcCountArgs a{};
  a.stage = S.arena.as<uint16_t>(); a.segs = S.segs.as<uint64_t>(); a.ngroups = S.ngroups; a.NB = S.NB; a.L = S.L;
  a.kept = S.kept.as<uint2>(); a.kept_off = S.kept_off.as<uint64_t>(); a.kept_n = S.kept_n.as<uint32_t>();
  a.kept_out = S.kept2.as<uint2>(); a.kept_out_off = S.kept2_off.as<uint64_t>(); a.kept_out_n = S.kept2_n.as<uint32_t>();
  a.overflow = (int*)(sc + 3);
  kmer_count_kernel<0><<<S.NB, KC_COUNT_THREADS, 0, st>>>(a);
  KCHK(v, hipGetLastError());
  std::swap(S.kept, S.kept2); std::swap(S.kept_off, S.kept2_off); std::swap(S.kept_n, S.kept2_n);
  KCHK(v, hipMemsetAsync(S.flush_n.p, 0, (size_t)S.NB * 8, st));
  int over = 0;
  KCHK(v, hipMemcpyAsync(&over, sc + 3, 4, hipMemcpyDeviceToHost, st));
  KCHK(v, hipStreamSynchronize(st));
  if (over) { *v.err = "a k-mer occurs more than 4294967295 times: its count would overflow the counter"; return MHAP_E_INVALID; }
  if (kc_prof()) fprintf(stderr, "[kmer] flush %d: %d groups, %llu windows, %llu kept entries of room\n", S.flushes, S.ngroups, (unsigned long long)S.arena_used, room);
  S.flushes++;
  S.ngroups = 0; S.arena_used = 0;
  return MHAP_OK;
}

}  // namespace

int kmer_count_begin(KmerCountState*& S, const HandleView& v, int k, int canonical) {
  (void)hipSetDevice(v.device);
  std::unique_ptr<KmerCountState> s(new KmerCountState());
  s->k = k; s->canonical = canonical ? 1 : 0; s->L = kmer_low_bits(k); s->NB = 1 << (2 * k - s->L);
  s->index_gen = v.index_gen;
  size_t free_b = 0, total_b = 0;
  s->budget = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? free_b / 4 / 2 : (1ULL << 30);
  if (const char* e = getenv("MHAP_KMER_STAGE_WINDOWS")) { const long long b = atoll(e); if (b > 0) s->budget = (uint64_t)b; }
  const size_t NB = (size_t)s->NB;
  KCHK(v, s->hist.ensure(NB * 4));
  KCHK(v, s->flush_n.ensure(NB * 8));
  KCHK(v, s->kept_off.ensure(NB * 8)); KCHK(v, s->kept2_off.ensure(NB * 8));
  KCHK(v, s->kept_n.ensure(NB * 4)); KCHK(v, s->kept2_n.ensure(NB * 4));
  KCHK(v, s->kept.ensure(sizeof(uint2))); KCHK(v, s->kept2.ensure(sizeof(uint2)));
  KCHK(v, s->scalars.ensure(64));
  KCHK(v, hipMemsetAsync(s->flush_n.p, 0, NB * 8, v.stream));
  KCHK(v, hipMemsetAsync(s->kept_off.p, 0, NB * 8, v.stream));
  KCHK(v, hipMemsetAsync(s->kept_n.p, 0, NB * 4, v.stream));
  KCHK(v, hipMemsetAsync(s->scalars.p, 0, 64, v.stream));
  KCHK(v, hipStreamSynchronize(v.stream));
  S = s.release();
  return MHAP_OK;
}

void kmer_count_release(KmerCountState* S) { delete S; }
int64_t kmer_count_total(const KmerCountState& S) { return S.total; }
int kmer_count_k(const KmerCountState& S) { return S.k; }
uint64_t kmer_count_index_gen(const KmerCountState& S) { return S.index_gen; }
uint64_t kmer_count_budget(const KmerCountState& S) { return S.budget; }

// Room for `windows` more staged windows in one run (the arena grows to it; a flush first when the budget would be passed).
int kmer_count_reserve(KmerCountState& S, const HandleView& v, uint64_t windows) {
  if (S.arena_used > 0 && S.arena_used + windows > S.budget) { const int rc = kc_flush(S, v); if (rc != MHAP_OK) return rc; }
  const size_t need = (size_t)(S.arena_used + windows) * 2 + 16;
  if (need > S.arena.cap) KCHK(v, S.arena.ensure(std::max(need, std::min<size_t>(S.arena.cap * 2, S.budget * 2 + 16)), true, v.stream));
  return MHAP_OK;
}

int kmer_count_add_group(KmerCountState& S, const HandleView& v, const ReadDesc* descs, int64_t n, const void* packed, size_t bytes) {
  if (n <= 0) return MHAP_OK;
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  uint64_t bound = 0;   // windows <= bases
  for (int64_t i = 0; i < n; i++) bound += (uint64_t)std::max(0, descs[i].length - S.k + 1);
  if (bound == 0) return MHAP_OK;
  if (bound > 0xFFFFFFFFull) { *v.err = "an ingest group of more than 2^32 k-mer windows (lower MHAP_INGEST_GROUP_BASES)"; return MHAP_E_INVALID; }
  int rc = kmer_count_reserve(S, v, bound);
  if (rc != MHAP_OK) return rc;
  KCHK(v, S.store.ensure(std::max<size_t>(bytes, 4)));
  KCHK(v, S.descs.ensure((size_t)n * sizeof(ReadDesc)));
  KCHK(v, S.segs.ensure((size_t)(S.ngroups + 1) * (S.NB + 1) * 8, true, st));
  KCHK(v, hipMemcpyAsync(S.store.p, packed, bytes, hipMemcpyHostToDevice, st));
  KCHK(v, hipMemcpyAsync(S.descs.p, descs, (size_t)n * sizeof(ReadDesc), hipMemcpyHostToDevice, st));
  KCHK(v, hipMemsetAsync(S.hist.p, 0, (size_t)S.NB * 4, st));
  const int grid = (int)std::min<int64_t>((n + KC_THREADS / MHAP_WAVE - 1) / (KC_THREADS / MHAP_WAVE), 8192);
  unsigned long long* sc = S.scalars.as<unsigned long long>();
  kmer_hist_kernel<0><<<grid, KC_THREADS, 0, st>>>(S.store.as<uint8_t>(), S.descs.as<ReadDesc>(), n, S.k, S.canonical, S.L, S.hist.as<uint32_t>(), nullptr, 0);
  KCHK(v, hipGetLastError());
  kmer_scan_kernel<<<1, KC_SCAN_THREADS, 0, st>>>(S.hist.as<uint32_t>(), S.NB, S.segs.as<uint64_t>() + (size_t)S.ngroups * (S.NB + 1), S.arena_used,
                                                  S.flush_n.as<unsigned long long>(), sc);
  KCHK(v, hipGetLastError());
  kmer_hist_kernel<1><<<grid, KC_THREADS, 0, st>>>(S.store.as<uint8_t>(), S.descs.as<ReadDesc>(), n, S.k, S.canonical, S.L, S.hist.as<uint32_t>(),
                                                   S.arena.as<uint16_t>(), S.arena_used);
  KCHK(v, hipGetLastError());
  unsigned long long got = 0;
  KCHK(v, hipMemcpyAsync(&got, sc, 8, hipMemcpyDeviceToHost, st));
  KCHK(v, hipStreamSynchronize(st));   // (the caller reuses its staging buffer)
  if (got > bound) { *v.err = "k-mer counter: more windows than bases (internal error)"; return MHAP_E_HIP; }
  S.arena_used += got; S.total += (int64_t)got; S.ngroups++;
  return MHAP_OK;
}

// The smallest count c >= 1 with (double)c / (double)total >= min_fraction (total + 1: none).
uint64_t kmer_line_threshold(uint64_t total, double mf) {
  if (total == 0) return 1;
  const double T = (double)total;
  double c0 = std::ceil(mf * T);
  uint64_t c = c0 < 1.0 ? 1 : (c0 > T + 1.0 ? total + 1 : (uint64_t)c0);
  while (c > 1 && (double)(c - 1) / T >= mf) c--;
  while (c <= total && (double)c / T < mf) c++;
  return c;
}

int kmer_count_finish(KmerCountState& S, const HandleView& v, double min_fraction, std::vector<uint32_t>& values, std::vector<uint32_t>& counts,
                      int64_t& distinct, KmerHistogram* histogram) {
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  const uint64_t total = (uint64_t)S.total;
  const uint64_t thr = kmer_line_threshold(total, min_fraction);
  const uint64_t space = 1ULL << (2 * S.k);
  uint64_t cap = thr > total ? 0 : std::min<uint64_t>(total / thr, space);
  if (thr > 0xFFFFFFFFull) cap = 0;
  KCHK(v, S.sel.ensure(std::max<uint64_t>(cap, 1) * sizeof(uint2)));
  KCHK(v, S.distinct.ensure((size_t)S.NB * 4));
  unsigned long long* sc = S.scalars.as<unsigned long long>();
  KCHK(v, hipMemsetAsync(sc + 2, 0, 16, st));
  KcCountArgs a{};
  a.stage = S.arena.as<uint16_t>(); a.segs = S.segs.as<uint64_t>(); a.ngroups = S.ngroups; a.NB = S.NB; a.L = S.L;
  a.kept = S.kept.as<uint2>(); a.kept_off = S.kept_off.as<uint64_t>(); a.kept_n = S.kept_n.as<uint32_t>();
  a.distinct = S.distinct.as<uint32_t>(); a.sel = S.sel.as<uint2>(); a.nsel = sc + 2; a.sel_cap = cap;
  a.thr = (uint32_t)std::min<uint64_t>(thr, 0xFFFFFFFFull);
  a.overflow = (int*)(sc + 3);
  // the histogram: a count above the dense range holds more than KC_HIST_DENSE windows, so at most total / (KC_HIST_DENSE + 1) values have one
  const uint64_t tail_cap = std::min<uint64_t>(total / (KC_HIST_DENSE + 1), space);
  std::vector<unsigned long long> dense;
  unsigned long long ntail = 0;
  if (histogram) {
    KCHK(v, S.hdense.ensure((size_t)KC_HIST_DENSE * 8));
    KCHK(v, S.htail.ensure(std::max<uint64_t>(tail_cap, 1) * 4));
    KCHK(v, hipMemsetAsync(S.hdense.p, 0, (size_t)KC_HIST_DENSE * 8, st));
    KCHK(v, hipMemsetAsync(sc + 4, 0, 8, st));
    a.dense = S.hdense.as<unsigned long long>(); a.tail = S.htail.as<uint32_t>(); a.ntail = sc + 4; a.tail_cap = tail_cap;
    kmer_count_kernel<2><<<S.NB, KC_COUNT_THREADS, 0, st>>>(a);
    dense.resize(KC_HIST_DENSE);
  } else {
    kmer_count_kernel<1><<<S.NB, KC_COUNT_THREADS, 0, st>>>(a);
  }
  KCHK(v, hipGetLastError());
  unsigned long long tail[2] = {0, 0};
  KCHK(v, hipMemcpyAsync(tail, sc + 2, 16, hipMemcpyDeviceToHost, st));
  std::vector<uint32_t> dist((size_t)S.NB);
  KCHK(v, hipMemcpyAsync(dist.data(), S.distinct.p, (size_t)S.NB * 4, hipMemcpyDeviceToHost, st));
  if (histogram) {
    KCHK(v, hipMemcpyAsync(dense.data(), S.hdense.p, (size_t)KC_HIST_DENSE * 8, hipMemcpyDeviceToHost, st));
    KCHK(v, hipMemcpyAsync(&ntail, sc + 4, 8, hipMemcpyDeviceToHost, st));
  }
  KCHK(v, hipStreamSynchronize(st));
  if ((int)tail[1]) { *v.err = "a k-mer occurs more than 4294967295 times: its count would overflow the counter"; return MHAP_E_INVALID; }
  if (tail[0] > cap) { *v.err = "k-mer counter: more selected k-mers than the bound (internal error)"; return MHAP_E_HIP; }
  if (ntail > tail_cap) { *v.err = "k-mer counter: more histogram tail entries than the bound (internal error)"; return MHAP_E_HIP; }
  distinct = 0;
  for (uint32_t d : dist) distinct += d;
  std::vector<uint2> sel((size_t)tail[0]);
  if (!sel.empty()) KCHK(v, hipMemcpy(sel.data(), S.sel.p, sel.size() * sizeof(uint2), hipMemcpyDeviceToHost));
  // file order: descending count, then ascending value
  std::sort(sel.begin(), sel.end(), [](const uint2& x, const uint2& y) { return x.y != y.y ? x.y > y.y : x.x < y.x; });
  values.resize(sel.size()); counts.resize(sel.size());
  for (size_t i = 0; i < sel.size(); i++) { values[i] = sel[i].x; counts[i] = sel[i].y; }
  if (histogram) {
    // ascending count, nonzero entries only: the dense range, then the tail's counts (sorted) with their multiplicities
    std::vector<uint32_t> big((size_t)ntail);
    if (!big.empty()) KCHK(v, hipMemcpy(big.data(), S.htail.p, big.size() * 4, hipMemcpyDeviceToHost));
    std::sort(big.begin(), big.end());
    histogram->counts.clear(); histogram->numbers.clear();
    for (int c = 1; c <= KC_HIST_DENSE; c++)
      if (dense[(size_t)c - 1]) { histogram->counts.push_back((uint32_t)c); histogram->numbers.push_back(dense[(size_t)c - 1]); }
    for (size_t i = 0; i < big.size(); i++) {
      if (i == 0 || big[i] != big[i - 1]) { histogram->counts.push_back(big[i]); histogram->numbers.push_back(0); }
      histogram->numbers.back()++;
    }
  }
  if (kc_prof()) fprintf(stderr, "[kmer] finish: %llu windows, %lld distinct, %zu lines (count >= %llu), %d flushes before\n", (unsigned long long)total,
                         (long long)distinct, sel.size(), (unsigned long long)thr, S.flushes);
  if (kc_prof() && histogram)
    fprintf(stderr, "[kmer] histogram: %zu counts, %llu tail entries (bound %llu)\n", histogram->counts.size(), ntail, (unsigned long long)tail_cap);
  return MHAP_OK;
}

// ---- sequence assessment: the drivers ------------------------------------------------------------------------------------------------
int kmer_count_finish_set(KmerCountState& S, const HandleView& v, uint64_t min_count, KmerSet& out) {
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  const uint64_t space = 1ULL << (2 * S.k);
  out.k = S.k; out.canonical = S.canonical; out.device = v.device; out.total = S.total; out.min_count = min_count;
  out.bytes = (size_t)std::max<uint64_t>((space / 8 + 15) & ~15ULL, 16);
  KCHK(v, hipMalloc(&out.bits, out.bytes));
  // a bucket of 64 values or more writes every one of its words; narrower ones OR into zeroed words, and so does the padding stay zero
  if (S.L < 6 || space / 8 < out.bytes) KCHK(v, hipMemsetAsync(out.bits, 0, out.bytes, st));
  KCHK(v, S.distinct.ensure((size_t)S.NB * 4));
  unsigned long long* sc = S.scalars.as<unsigned long long>();
  KCHK(v, hipMemsetAsync(sc + 2, 0, 16, st));   // [2] the members here, [3] the overflow flag
  KcCountArgs a{};
  a.stage = S.arena.as<uint16_t>(); a.segs = S.segs.as<uint64_t>(); a.ngroups = S.ngroups; a.NB = S.NB; a.L = S.L;
  a.kept = S.kept.as<uint2>(); a.kept_off = S.kept_off.as<uint64_t>(); a.kept_n = S.kept_n.as<uint32_t>();
  a.distinct = S.distinct.as<uint32_t>(); a.overflow = (int*)(sc + 3);
  kmer_set_kernel<<<S.NB, KC_COUNT_THREADS, 0, st>>>(a, min_count, (unsigned long long*)out.bits, sc + 2);
  KCHK(v, hipGetLastError());
  unsigned long long tail[2] = {0, 0};
  KCHK(v, hipMemcpyAsync(tail, sc + 2, 16, hipMemcpyDeviceToHost, st));
  std::vector<uint32_t> dist((size_t)S.NB);
  KCHK(v, hipMemcpyAsync(dist.data(), S.distinct.p, (size_t)S.NB * 4, hipMemcpyDeviceToHost, st));
  KCHK(v, hipStreamSynchronize(st));
  if ((int)tail[1]) { *v.err = "a k-mer occurs more than 4294967295 times: its count would overflow the counter"; return MHAP_E_INVALID; }
  out.members = (int64_t)tail[0];
  out.distinct = 0;
  for (uint32_t d : dist) out.distinct += d;
  if (kc_prof()) fprintf(stderr, "[kmer] set: %lld of %lld distinct %d-mers at count >= %llu, %zu bytes\n", (long long)out.members, (long long)out.distinct, S.k,
                         (unsigned long long)min_count, out.bytes);
  return MHAP_OK;
}

void kmer_set_release(KmerSet& s) {
  if (s.bits) { (void)hipSetDevice(s.device); (void)hipFree(s.bits); }
  s.bits = nullptr; s.bytes = 0;
}

int kmer_set_contains(const HandleView& v, const KmerSet& s, const uint64_t* values, int64_t n, uint8_t* out) {
  if (n <= 0) return MHAP_OK;
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  DevBuf dv, dout;
  auto run = [&]() -> int {
    KCHK(v, dv.ensure((size_t)n * 8));
    KCHK(v, dout.ensure((size_t)n));
    KCHK(v, hipMemcpyAsync(dv.p, values, (size_t)n * 8, hipMemcpyHostToDevice, st));
    kmer_set_contains_kernel<<<(unsigned)((n + KC_THREADS - 1) / KC_THREADS), KC_THREADS, 0, st>>>((const uint32_t*)s.bits, s.k, dv.as<uint64_t>(), n, dout.as<uint8_t>());
    KCHK(v, hipGetLastError());
    KCHK(v, hipMemcpyAsync(out, dout.p, (size_t)n, hipMemcpyDeviceToHost, st));
    KCHK(v, hipStreamSynchronize(st));
    return MHAP_OK;
  };
  const int rc = run();
  dv.release(); dout.release();
  return rc;
}

int kmer_set_compare(const HandleView& v, const KmerSet& a, const KmerSet& b, int64_t counts[3]) {
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  DevBuf dc;
  auto run = [&]() -> int {
    KCHK(v, dc.ensure(24));
    KCHK(v, hipMemsetAsync(dc.p, 0, 24, st));
    const int64_t n16 = (int64_t)(a.bytes / 16);
    const int grid = (int)std::min<int64_t>((n16 + KC_THREADS - 1) / KC_THREADS, 8 * (int64_t)std::max(1, v.num_cus));
    kmer_set_compare_kernel<<<grid, KC_THREADS, 0, st>>>((const uint4*)a.bits, (const uint4*)b.bits, n16, dc.as<unsigned long long>());
    KCHK(v, hipGetLastError());
    unsigned long long got[3] = {0, 0, 0};
    KCHK(v, hipMemcpyAsync(got, dc.p, 24, hipMemcpyDeviceToHost, st));
    KCHK(v, hipStreamSynchronize(st));
    for (int i = 0; i < 3; i++) counts[i] = (int64_t)got[i];
    return MHAP_OK;
  };
  const int rc = run();
  dc.release();
  return rc;
}

int kmer_eval_group(const HandleView& v, const KmerSet& s, const ReadDesc* descs, int64_t n, const void* packed, size_t bytes, KmerEval& out) {
  if (n <= 0) return MHAP_OK;
  (void)hipSetDevice(v.device);
  hipStream_t st = v.stream;
  // the work items: (sequence, tile of KE_TILE positions), the tiles of a sequence in a row; a sequence shorter than k has no window and no tile
  std::vector<int64_t> tile_first((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; i++)
    tile_first[(size_t)i + 1] = tile_first[(size_t)i] + (descs[i].length >= s.k ? ((int64_t)descs[i].length + KE_TILE - 1) / KE_TILE : 0);
  const int64_t ntiles = tile_first[(size_t)n];
  std::vector<int32_t> tile_seq((size_t)ntiles);
  for (int64_t i = 0; i < n; i++) std::fill(tile_seq.begin() + tile_first[(size_t)i], tile_seq.begin() + tile_first[(size_t)i + 1], (int32_t)i);
  const size_t row0 = out.rows.size(), iv_before = out.intervals.size();
  out.rows.resize(row0 + (size_t)n * 5, 0);
  for (int64_t i = 0; i < n; i++) out.rows[row0 + (size_t)i * 5] = descs[i].length;
  if (ntiles == 0) return MHAP_OK;
  const int64_t seq0 = (int64_t)(row0 / 5);
  DevBuf &store = out.scratch[0], &ddescs = out.scratch[1], &dseq = out.scratch[2], &dfirst = out.scratch[3], &rows = out.scratch[4], &umask = out.scratch[5],
         &counts = out.scratch[6], &at = out.scratch[7], &iv = out.scratch[8];   // (kept from group to group; kmer_eval_done frees them)
  auto run = [&]() -> int {
    KCHK(v, store.ensure(std::max<size_t>(bytes, 4)));
    KCHK(v, ddescs.ensure((size_t)n * sizeof(ReadDesc)));
    KCHK(v, dseq.ensure((size_t)ntiles * 4));
    KCHK(v, dfirst.ensure(((size_t)n + 1) * 8));
    KCHK(v, rows.ensure((size_t)n * 32));
    KCHK(v, umask.ensure((size_t)ntiles * (MHAP_WAVE - 1) * 8));
    KCHK(v, counts.ensure((size_t)ntiles * 8));            // begins per tile, then ends per tile
    KCHK(v, at.ensure(((size_t)ntiles + 1) * 16));         // their prefix sums
    KCHK(v, hipMemcpyAsync(store.p, packed, bytes, hipMemcpyHostToDevice, st));
    KCHK(v, hipMemcpyAsync(ddescs.p, descs, (size_t)n * sizeof(ReadDesc), hipMemcpyHostToDevice, st));
    KCHK(v, hipMemcpyAsync(dseq.p, tile_seq.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, st));
    KCHK(v, hipMemcpyAsync(dfirst.p, tile_first.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    KCHK(v, hipMemsetAsync(rows.p, 0, (size_t)n * 32, st));
    KeArgs a{};
    a.store = store.as<uint8_t>(); a.descs = ddescs.as<ReadDesc>(); a.tile_seq = dseq.as<int32_t>(); a.tile_first = dfirst.as<int64_t>(); a.ntiles = ntiles;
    a.bits = (const uint32_t*)s.bits; a.k = s.k; a.canonical = s.canonical;
    a.rows = rows.as<unsigned long long>(); a.umask = umask.as<unsigned long long>();
    const unsigned grid = (unsigned)((ntiles + KE_THREADS / MHAP_WAVE - 1) / (KE_THREADS / MHAP_WAVE));
    const bool prof = kc_prof();
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    if (prof) KCHK(v, hipStreamSynchronize(st));   // (the uploads end here, so that the line below times the kernel alone)
    const double t0 = now();
    kmer_eval_kernel<<<grid, KE_THREADS, 0, st>>>(a);
    KCHK(v, hipGetLastError());
    if (prof) KCHK(v, hipStreamSynchronize(st));
    const double t1 = now();
    int32_t *nbegin = counts.as<int32_t>(), *nend = nbegin + ntiles;
    int64_t *at_begin = at.as<int64_t>(), *at_end = at_begin + ntiles + 1;
    kmer_eval_intervals_kernel<0><<<grid, KE_THREADS, 0, st>>>(a.umask, a.tile_seq, a.tile_first, ntiles, nbegin, nend, nullptr, nullptr, 0, nullptr);
    KCHK(v, hipGetLastError());
    scan_kernel<int32_t><<<1, 1024, 0, st>>>(nbegin, ntiles, at_begin);
    KCHK(v, hipGetLastError());
    scan_kernel<int32_t><<<1, 1024, 0, st>>>(nend, ntiles, at_end);
    KCHK(v, hipGetLastError());
    int64_t nb = 0, ne = 0;
    KCHK(v, hipMemcpyAsync(&nb, at_begin + ntiles, 8, hipMemcpyDeviceToHost, st));
    KCHK(v, hipMemcpyAsync(&ne, at_end + ntiles, 8, hipMemcpyDeviceToHost, st));
    const size_t r0 = out.rows.size() - (size_t)n * 5;
    std::vector<unsigned long long> got((size_t)n * 4);
    KCHK(v, hipMemcpyAsync(got.data(), rows.p, (size_t)n * 32, hipMemcpyDeviceToHost, st));
    KCHK(v, hipStreamSynchronize(st));
    if (nb != ne) { *v.err = "k-mer evaluation: interval begins and ends differ in number (internal error)"; return MHAP_E_HIP; }
    for (int64_t i = 0; i < n; i++)
      for (int f = 0; f < 4; f++) out.rows[r0 + (size_t)i * 5 + 1 + (size_t)f] = (int64_t)got[(size_t)i * 4 + (size_t)f];
    const double t2 = now();
    if (prof) fprintf(stderr, "[kmer] eval group: %lld sequences, %lld tiles, %lld intervals; walk %.2f ms, rows and interval counts %.2f ms\n", (long long)n,
                      (long long)ntiles, (long long)nb, (t1 - t0) * 1e3, (t2 - t1) * 1e3);
    if (nb == 0) return MHAP_OK;
    KCHK(v, iv.ensure((size_t)nb * 24));
    kmer_eval_intervals_kernel<1><<<grid, KE_THREADS, 0, st>>>(a.umask, a.tile_seq, a.tile_first, ntiles, nullptr, nullptr, at_begin, at_end, seq0, iv.as<int64_t>());
    KCHK(v, hipGetLastError());
    const size_t iv0 = out.intervals.size();
    out.intervals.resize(iv0 + (size_t)nb * 3);
    KCHK(v, hipMemcpyAsync(out.intervals.data() + iv0, iv.p, (size_t)nb * 24, hipMemcpyDeviceToHost, st));
    KCHK(v, hipStreamSynchronize(st));
    if (prof) fprintf(stderr, "[kmer] eval group: intervals filled and copied in %.2f ms\n", (now() - t2) * 1e3);
    return MHAP_OK;
  };
  const int rc = run();
  if (rc != MHAP_OK) { out.rows.resize(row0); out.intervals.resize(iv_before); }
  return rc;
}

void kmer_eval_done(const HandleView& v, KmerEval& e) {
  (void)hipSetDevice(v.device);
  (void)hipStreamSynchronize(v.stream);
  for (DevBuf& b : e.scratch) b.release();
}

}  // namespace mhap

// The lane arithmetic of kmer_eval_kernel on the host: the sequence stored as the ingest stores it, every tile's 64 lanes walked in
// turn against a bitmap in host memory.  row: windows, missing, runs, unsupported; umask: 63 words per tile.
extern "C" int mhap_selftest_kmer_eval(const char* seq, int32_t len, int32_t k, int32_t canonical, const uint32_t* bits, int64_t* row, uint64_t* umask) {
  using namespace mhap;
  if (k < 1 || k > 16 || len < 0 || (len > 0 && !seq) || !bits || !row) return MHAP_E_INVALID;
  bool raw = false;
  for (int p = 0; p < len; p++) { uint32_t code; raw = raw || !kmer_code((uint8_t)seq[p], code); }
  std::vector<uint32_t> W((size_t)(raw ? (len + 3) / 4 : (len + 15) / 16) + 1, 0u);
  for (int p = 0; p < len; p++) {
    uint32_t code = 0;
    if (raw) W[(size_t)p >> 2] |= (uint32_t)(uint8_t)seq[p] << (8 * (p & 3));
    else { kmer_code((uint8_t)seq[p], code); W[(size_t)p >> 4] |= code << (2 * (p & 15)); }
  }
  for (int f = 0; f < 4; f++) row[f] = 0;
  const int64_t ntiles = len >= k ? ((int64_t)len + KE_TILE - 1) / KE_TILE : 0;
  for (int64_t t = 0; t < ntiles; t++) {
    unsigned long long V[MHAP_WAVE], P[MHAP_WAVE];
    for (int l = 0; l < MHAP_WAVE; l++) {
      const int64_t s = t * KE_TILE + (int64_t)l * KE_LANE;
      if (raw) ke_lane_states<true>(W.data(), s, len, k, canonical != 0, bits, V[l], P[l]);
      else ke_lane_states<false>(W.data(), s, len, k, canonical != 0, bits, V[l], P[l]);
    }
    for (int l = 0; l < MHAP_WAVE - 1; l++) {
      unsigned long long U;
      const unsigned long long c = ke_lane_counts(V[l], P[l], V[l + 1], P[l + 1], k, U);
      for (int f = 0; f < 4; f++) row[f] += (int64_t)((c >> (16 * f)) & 0xFFFFu);
      if (umask) umask[t * (MHAP_WAVE - 1) + l] = U;
    }
  }
  return MHAP_OK;
}

extern "C" int mhap_selftest_kmer_windows(const char* seq, int32_t len, int32_t k, int32_t canonical, uint64_t* out, uint8_t* valid) {
  using namespace mhap;
  if (k < 1 || k > 16 || len < 0 || (len > 0 && !seq)) return MHAP_E_INVALID;
  const uint32_t mask = kmer_mask(k);
  KmerRoll r;
  for (int p = 0; p < len; p++) {
    uint32_t code;
    const bool ok = kmer_code((uint8_t)seq[p], code);
    kmer_push(r, code, ok, k, mask);
    if (p >= k - 1) {
      if (out) out[p - k + 1] = r.run >= k ? kmer_value(r, canonical != 0) : 0;
      if (valid) valid[p - k + 1] = r.run >= k ? 1 : 0;
    }
  }
  return MHAP_OK;
}
