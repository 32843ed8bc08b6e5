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
#include <hip/hip_runtime.h>

#include <algorithm>
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
  if (over) *a.overflow = 1;
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

}  // namespace mhap

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
