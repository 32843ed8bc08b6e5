// ksim_kernels.hip — pair statistics of KmerStatSimulator (J/main/KmerStatSimulator.java): compareKmers and compareMinHash of a
// pair of reads on the GPU.  The contract is mhap_pair_kmer_stats in include/mhap_hip.h; tests/ksim_ref.py restates it on the CPU.
//
// One workgroup per pair on a persistent grid (pairs taken through an atomic counter, as align_kernels.hip does).  Per pair:
//   1. the two segments and their reverse complements (Utils.rc's table) are copied into the workgroup's scratch as dword-aligned bytes;
//   2. every window of both reads gets a key: (2-bit code << 1) | read for ACGT windows with k <= 31 ("packed"), otherwise a 64-bit hash
//      of the window's bytes with a second word (read << 31 | position) beside it ("hashed"; equal keys are told apart by their bytes);
//   3. a bitonic sort orders the keys by (k-mer, read), so equal k-mers form runs with first-read windows ahead of second-read ones:
//      total = the number of runs, shared = the number of first-read -> second-read steps inside a run whose k-mer is not in the skip set
//      (a binary search in the sorted skip array);
//   4. the same scratch then holds (read << 32) | (murmur3_32 of the canonical k-mer ^ 0x80000000) per window, sorted: each read's
//      signed hashes in ascending order, duplicates kept, so the first min(bottom_k, n) of each are its BottomSketch, and one lane runs
//      BottomSketch.jaccard's merge loop over them.
// The scratch is LDS when the pair fits the workgroup's LDS, else a per-workgroup slice of HBM (the host picks the kernel by length).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

constexpr int KS_T = 256;                    // lanes per workgroup
constexpr uint32_t KS_SENT = 0xFFFFFFFFu;    // position word of a padding slot
constexpr int KS_HASHED = 1;                 // pair flag: hashed keys (else packed 2-bit keys)

__host__ __device__ inline int64_t ks_seg_bytes(int64_t len) { return ((len + 8 + 15) / 16) * 16; }   // a segment copy + fetch4 padding
__host__ __device__ inline int64_t ks_pow2(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }
// scratch bytes of a pair: four segment copies, 8 B of key per slot and, hashed, 4 B of position per slot
__host__ __device__ inline int64_t ks_scratch_bytes(int64_t a_len, int64_t b_len, int k, bool hashed) {
  const int64_t na = a_len >= k ? a_len - k + 1 : 0, nb = b_len >= k ? b_len - k + 1 : 0;
  const int64_t P = ks_pow2(std::max<int64_t>(na + nb, 2));
  return 2 * ks_seg_bytes(a_len) + 2 * ks_seg_bytes(b_len) + 8 * P + (hashed ? 4 * P : 0);
}

__device__ inline uint32_t ks_code(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }

// unsigned byte order of two k-byte strings (String.compareTo on Latin-1 chars)
__device__ inline int ks_cmp(const uint8_t* a, const uint8_t* b, int k) {
  for (int i = 0; i < k; i++)
    if (a[i] != b[i]) return (int)a[i] - (int)b[i];
  return 0;
}
// the window against skip entry e (k bytes each); packed windows are decoded from their code
__device__ inline int ks_cmp_code(uint64_t code, const uint8_t* e, int k) {
  for (int i = 0; i < k; i++) {
    const uint32_t c = (0x54474341u >> (8 * ((code >> (2 * (k - 1 - i))) & 3u))) & 0xFFu;
    if (c != e[i]) return (int)c - (int)e[i];
  }
  return 0;
}

template <bool HASHED>
__device__ inline bool ks_less(const uint64_t* key, const uint32_t* pos, const uint8_t* fa, const uint8_t* fb, int k, int i, int j) {
  const uint64_t ki = key[i], kj = key[j];
  if (ki != kj) return ki < kj;
  if (!HASHED) return false;
  const uint32_t pi = pos[i], pj = pos[j];
  if (pi != KS_SENT && pj != KS_SENT) {
    const int c = ks_cmp((pi >> 31 ? fb : fa) + (pi & 0x7FFFFFFFu), (pj >> 31 ? fb : fa) + (pj & 0x7FFFFFFFu), k);
    if (c) return c < 0;
  }
  return pi < pj;
}

template <bool HASHED>
__device__ void ks_sort(uint64_t* key, uint32_t* pos, const uint8_t* fa, const uint8_t* fb, int k, int P) {
  const int t = threadIdx.x;
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int q = t; q < (P >> 1); q += KS_T) {
        const int i = 2 * stride * (q / stride) + (q % stride), j = i + stride;
        const bool asc = (i & size) == 0;
        if (asc ? ks_less<HASHED>(key, pos, fa, fb, k, j, i) : ks_less<HASHED>(key, pos, fa, fb, k, i, j)) {
          const uint64_t x = key[i]; key[i] = key[j]; key[j] = x;
          if (HASHED) { const uint32_t y = pos[i]; pos[i] = pos[j]; pos[j] = y; }
        }
      }
      __syncthreads();
    }
}

// window i of the concatenation (first read's windows, then the second's) as (read, position)
__device__ inline void ks_window(int i, int na, int& src, int& p) { src = i >= na; p = src ? i - na : i; }

template <bool LDS>
__global__ __launch_bounds__(KS_T) void pair_kmer_stats_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ pairs,
                                                               const int32_t* __restrict__ flags, const int32_t* __restrict__ order, int n_order,
                                                               int* __restrict__ next, uint8_t* __restrict__ scratch, int64_t stride, int k,
                                                               int bottom_k, const uint8_t* __restrict__ skip, int n_skip, uint64_t hash_mask,
                                                               int32_t* __restrict__ out) {
  extern __shared__ __align__(16) uint8_t ks_lds[];
  __shared__ int cur, cnt_total, cnt_shared;
  uint8_t* base = LDS ? ks_lds : scratch + (int64_t)blockIdx.x * stride;
  const int t = threadIdx.x;
  for (;;) {
    if (t == 0) { cur = atomicAdd(next, 1); cnt_total = 0; cnt_shared = 0; }
    __syncthreads();
    const int it = cur;
    if (it >= n_order) return;
    const int pi = order[it];
    const int64_t a_off = pairs[4 * (int64_t)pi], b_off = pairs[4 * (int64_t)pi + 2];
    const int a_len = (int)pairs[4 * (int64_t)pi + 1], b_len = (int)pairs[4 * (int64_t)pi + 3];
    const bool hashed = flags[pi] & KS_HASHED;
    const int na = a_len >= k ? a_len - k + 1 : 0, nb = b_len >= k ? b_len - k + 1 : 0, N = na + nb;
    const int P = (int)ks_pow2(N > 2 ? N : 2);
    uint8_t* fa = base;
    uint8_t* ra = fa + ks_seg_bytes(a_len);
    uint8_t* fb = ra + ks_seg_bytes(a_len);
    uint8_t* rb = fb + ks_seg_bytes(b_len);
    uint64_t* key = (uint64_t*)(rb + ks_seg_bytes(b_len));
    uint32_t* pos = (uint32_t*)(key + P);
    // 1. the segments and their reverse complements, zero padded
    for (int i = t; i < ks_seg_bytes(a_len); i += KS_T) {
      fa[i] = i < a_len ? bases[a_off + i] : 0;
      ra[i] = i < a_len ? (uint8_t)rc_char(bases[a_off + a_len - 1 - i]) : 0;
    }
    for (int i = t; i < ks_seg_bytes(b_len); i += KS_T) {
      fb[i] = i < b_len ? bases[b_off + i] : 0;
      rb[i] = i < b_len ? (uint8_t)rc_char(bases[b_off + b_len - 1 - i]) : 0;
    }
    __syncthreads();
    // 2. keys
    for (int i = t; i < P; i += KS_T) {
      if (i >= N) { key[i] = ~0ULL; if (hashed) pos[i] = KS_SENT; continue; }
      int src, p;
      ks_window(i, na, src, p);
      const uint8_t* w = (src ? fb : fa) + p;
      if (hashed) {
        uint64_t h = 0xcbf29ce484222325ULL;   // FNV-1a over the bytes, then fmix64
        for (int j = 0; j < k; j++) h = (h ^ w[j]) * 0x100000001b3ULL;
        key[i] = fmix64(h) & hash_mask;
        pos[i] = ((uint32_t)src << 31) | (uint32_t)p;
      } else {
        uint64_t c = 0;
        for (int j = 0; j < k; j++) c = (c << 2) | ks_code(w[j]);
        key[i] = (c << 1) | (uint64_t)src;
      }
    }
    __syncthreads();
    // 3. runs of equal k-mers
    if (hashed) ks_sort<true>(key, pos, fa, fb, k, P); else ks_sort<false>(key, pos, fa, fb, k, P);
    int my_total = 0, my_shared = 0;
    for (int i = t; i < N; i += KS_T) {
      bool eq_prev, eq_next = false;
      int src_i, src_n = 0;
      const uint8_t* wi = nullptr;
      if (hashed) {
        const uint32_t p0 = pos[i];
        src_i = p0 >> 31;
        wi = (src_i ? fb : fa) + (p0 & 0x7FFFFFFFu);
        eq_prev = i > 0 && key[i - 1] == key[i] && ks_cmp((pos[i - 1] >> 31 ? fb : fa) + (pos[i - 1] & 0x7FFFFFFFu), wi, k) == 0;
        if (i + 1 < N) {
          const uint32_t p1 = pos[i + 1];
          src_n = p1 >> 31;
          eq_next = key[i + 1] == key[i] && ks_cmp(wi, (src_n ? fb : fa) + (p1 & 0x7FFFFFFFu), k) == 0;
        }
      } else {
        src_i = (int)(key[i] & 1);
        eq_prev = i > 0 && (key[i - 1] >> 1) == (key[i] >> 1);
        if (i + 1 < N) { src_n = (int)(key[i + 1] & 1); eq_next = (key[i + 1] >> 1) == (key[i] >> 1); }
      }
      my_total += !eq_prev;
      if (eq_next && src_i == 0 && src_n == 1) {
        bool in_skip = false;
        int lo = 0, hi = n_skip;   // first entry >= the window
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const int c = hashed ? ks_cmp(skip + (int64_t)mid * k, wi, k) : -ks_cmp_code(key[i] >> 1, skip + (int64_t)mid * k, k);
          if (c < 0) lo = mid + 1; else hi = mid;
        }
        if (lo < n_skip) in_skip = hashed ? ks_cmp(skip + (int64_t)lo * k, wi, k) == 0 : ks_cmp_code(key[i] >> 1, skip + (int64_t)lo * k, k) == 0;
        my_shared += !in_skip;
      }
    }
    if (my_total) atomicAdd(&cnt_total, my_total);
    if (my_shared) atomicAdd(&cnt_shared, my_shared);
    __syncthreads();
    // 4. bottom sketches: canonical murmur3_32 per window (HashUtils.computeSequenceHashes), sorted per read
    for (int i = t; i < P; i += KS_T) {
      if (i >= N) { key[i] = ~0ULL; continue; }
      int src, p;
      ks_window(i, na, src, p);
      const uint8_t* f = src ? fb : fa;
      const uint8_t* r = src ? rb : ra;
      const int n = src ? b_len : a_len, q = n - p - k;
      const bool use_rc = ks_cmp(r + q, f + p, k) < 0;
      const uint32_t h = use_rc ? murmur32_chars<0>((const uint32_t*)r, q, k) : murmur32_chars<0>((const uint32_t*)f, p, k);
      key[i] = ((uint64_t)src << 32) | (uint64_t)(h ^ 0x80000000u);
    }
    __syncthreads();
    ks_sort<false>(key, pos, fa, fb, k, P);
    if (t == 0) {
      const int ka = na < bottom_k ? na : bottom_k, kb = nb < bottom_k ? nb : bottom_k, kk = ka < kb ? ka : kb;
      const uint64_t* A = key;
      const uint64_t* B = key + na;
      int i = 0, j = 0, inter = 0;
      for (int u = 0; u < kk; u++) {
        const uint32_t x = (uint32_t)A[i], y = (uint32_t)B[j];
        if (x < y) i++;
        else if (x > y) j++;
        else { inter++; i++; j++; }
      }
      out[3 * (int64_t)pi + 0] = cnt_shared;
      out[3 * (int64_t)pi + 1] = cnt_total;
      out[3 * (int64_t)pi + 2] = inter;
    }
    __syncthreads();
  }
}

// ---- on-device trials (--rng device) --------------------------------------------------------------------------------------------
// Every draw is splitmix64 of a counter keyed by (seed, trial, role, index, slot), so a trial's reads do not depend on the launch shape or
// the chunk a trial falls in.  Roles of the key: 0 / 1 / 2 the walks of the first read, the shared partner and the random partner; 3 the
// bases of a trial's random 4L sequence (no reference); 4 the random partner's bases (no reference); 5 the record and position picks.
constexpr int KG_T = 256;
enum { KR_GENOME = 3, KR_RANDOM = 4, KR_PICK = 5 };
constexpr int KG_MAX_VISITS = 1 << 16;     // insertions at one base beyond this: the error mix is rejected on the host long before
constexpr int64_t KG_MAX_PICKS = 1 << 20;  // redraws of a record or position (the host checks that an eligible one exists)

__host__ __device__ inline uint64_t ks_splitmix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t ks_rand(uint64_t seed, uint64_t trial, uint32_t role, uint64_t idx, uint32_t slot) {
  return ks_splitmix(ks_splitmix(ks_splitmix(ks_splitmix(seed) ^ trial) ^ (((uint64_t)role << 32) | slot)) ^ idx);
}
__device__ inline double ks_u01(uint64_t r) { return (double)(r >> 11) * 0x1.0p-53; }
__device__ inline uint64_t ks_below(uint64_t r, uint64_t n) { return __umul64hi(r, n); }   // uniform in [0, n)

struct KgParams {
  uint64_t seed; int64_t trial0; int L; int64_t offset; double e, pi, ps; int one_sided, roles;
  const uint8_t* ref; const int64_t* ref_off; const int32_t* ref_len; int n_ref;
};
struct KgPick { int sid, rsid; int64_t fpos, spos, rpos; bool ok; };

// simulate's picks (:349-358, :398-412): a record of >= 4L bases and a position in it, the shared partner's position, a record of >= 2L
// bases and a position not overlapping the first read's on the same record; without a reference firstPos = 0 in a fresh 4L sequence
__device__ KgPick ks_pick(const KgParams& P, uint64_t trial) {
  KgPick k{0, 0, 0, 0, 0, true};
  const int64_t L = P.L;
  if (P.n_ref == 0) { k.spos = P.offset % (4 * L); return k; }
  uint64_t c = 0;
  do { k.sid = (int)ks_below(ks_rand(P.seed, trial, KR_PICK, c++, 0), P.n_ref); } while (P.ref_len[k.sid] < 4 * L && c < KG_MAX_PICKS);
  if (P.ref_len[k.sid] < 4 * L) { k.ok = false; return k; }
  k.fpos = (int64_t)ks_below(ks_rand(P.seed, trial, KR_PICK, c++, 0), P.ref_len[k.sid]);
  k.spos = (k.fpos + P.offset) % P.ref_len[k.sid];
  do { k.rsid = (int)ks_below(ks_rand(P.seed, trial, KR_PICK, c++, 0), P.n_ref); } while (P.ref_len[k.rsid] < 2 * L && c < 2 * KG_MAX_PICKS);
  if (P.ref_len[k.rsid] < 2 * L) { k.ok = false; return k; }
  k.rpos = (int64_t)ks_below(ks_rand(P.seed, trial, KR_PICK, c++, 0), P.ref_len[k.rsid]);
  while (k.rsid == k.sid && std::min(k.fpos + L, k.rpos + L) - std::max(k.fpos, k.rpos) + 1 > 0 && c < 3 * KG_MAX_PICKS)
    k.rpos = (int64_t)ks_below(ks_rand(P.seed, trial, KR_PICK, c++, 0), P.ref_len[k.rsid]);
  k.ok = c < KG_MAX_PICKS && P.ref_len[k.sid] >= 4 * L && P.ref_len[k.rsid] >= 2 * L && !(k.rsid == k.sid && std::min(k.fpos + L, k.rpos + L) - std::max(k.fpos, k.rpos) + 1 > 0);
  return k;
}

// getSequence's walk at one source base: every visit draws the error test (slot 3v), an error its type (3v + 1) and, for a substitution
// or an insertion, its base (3v + 2); an insertion visits the base again.  Writes the emitted bases through `emit` and returns how many.
template <typename F>
__device__ inline int ks_walk(const KgParams& P, uint64_t trial, int role, int64_t j, uint32_t c, double e, double pi, double ps, int* ev, F emit) {
  int n = 0;
  for (int v = 0; v < KG_MAX_VISITS; v++) {
    ev[3]++;
    if (ks_u01(ks_rand(P.seed, trial, role, j, 3 * v)) < e) {
      const double t = ks_u01(ks_rand(P.seed, trial, role, j, 3 * v + 1));
      const uint64_t r = ks_rand(P.seed, trial, role, j, 3 * v + 2);
      if (t < ps) {                 // substitution: one of the other three of ACGT (a non-ACGT base: one of all four)
        const uint32_t code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
        uint32_t b;
        if (code < 4) { b = (uint32_t)ks_below(r, 3); b += b >= code; } else b = (uint32_t)ks_below(r, 4);
        emit(n++, (uint8_t)((0x54474341u >> (8 * b)) & 0xFFu));
        ev[2]++;
        return n;
      }
      if (t < pi + ps) {            // insertion before the base, which is visited again
        emit(n++, (uint8_t)((0x54474341u >> (8 * ks_below(r, 4))) & 0xFFu));
        ev[0]++;
        continue;
      }
      ev[1]++;                      // deletion
      return n;
    }
    emit(n++, (uint8_t)c);
    return n;
  }
  return -1;
}

__device__ inline uint32_t ks_src(const KgParams& P, uint64_t trial, int sid, int64_t pos, int64_t j) {
  if (P.n_ref == 0) {
    const int64_t g = (pos + j) % (4 * (int64_t)P.L);
    return (0x54474341u >> (8 * (ks_rand(P.seed, trial, KR_GENOME, (uint64_t)g, 0) >> 62))) & 0xFFu;
  }
  return P.ref[P.ref_off[sid] + (pos + j) % P.ref_len[sid]];
}

// one workgroup per (trial, role): lane t walks source bases [t * seg, (t + 1) * seg) of the 2L window twice, first counting its
// emissions, then (after a scan of the lanes' counts) writing those that fall into the trimmed window of L bases
__global__ __launch_bounds__(KG_T) void ksim_gen_kernel(KgParams P, uint8_t* __restrict__ reads, int32_t* __restrict__ meta,
                                                        int32_t* __restrict__ events, int* __restrict__ err_trial) {
  __shared__ int64_t tot[KG_T];
  __shared__ int ev_s[4];
  const int t = threadIdx.x, role = (int)(blockIdx.x % P.roles);
  const int64_t lt = blockIdx.x / P.roles;
  const uint64_t trial = (uint64_t)(P.trial0 + lt);
  const int64_t L = P.L;
  uint8_t* out = reads + (lt * P.roles + role) * L;
  const KgPick pk = ks_pick(P, trial);
  if (t == 0 && role == 0 && meta) {
    int32_t* m = meta + 5 * lt;
    m[0] = pk.sid; m[1] = (int32_t)pk.fpos; m[2] = (int32_t)pk.spos; m[3] = pk.rsid; m[4] = (int32_t)pk.rpos;
  }
  if (!pk.ok) { if (t == 0) atomicMin(err_trial, (int)lt); return; }
  if (role == 2 && P.n_ref == 0) {   // buildRandomSequence(L): no errors
    for (int64_t i = t; i < L; i += KG_T) out[i] = (0x54474341u >> (8 * (ks_rand(P.seed, trial, KR_RANDOM, (uint64_t)i, 0) >> 62))) & 0xFFu;
    if (events && t < 4) events[4 * (lt * P.roles + role) + t] = 0;
    return;
  }
  const int sid = role == 2 ? pk.rsid : pk.sid;
  const int64_t pos = role == 0 ? pk.fpos : role == 1 ? pk.spos : pk.rpos;
  const bool err_free = role > 0 && P.one_sided;
  const double e = err_free ? 0.0 : P.e, pi = err_free ? 0.0 : P.pi, ps = err_free ? 0.0 : P.ps;
  const int64_t W = 2 * L, seg = (W + KG_T - 1) / KG_T, lo = std::min<int64_t>(W, t * seg), hi = std::min<int64_t>(W, lo + seg);
  if (t < 4) ev_s[t] = 0;
  int ev[4] = {0, 0, 0, 0};
  int64_t cnt = 0;
  bool bad = false;
  for (int64_t j = lo; j < hi; j++) {
    const int n = ks_walk(P, trial, role, j, ks_src(P, trial, sid, pos, j), e, pi, ps, ev, [](int, uint8_t) {});
    if (n < 0) bad = true; else cnt += n;
  }
  tot[t] = cnt;
  __syncthreads();
  for (int q = 0; q < 4; q++) if (ev[q]) atomicAdd(&ev_s[q], ev[q]);
  if (bad) atomicMin(err_trial, (int)lt);
  __shared__ int64_t Mtot;
  if (t == 0) {   // exclusive scan of the lanes' counts; the total is the read's length before trimming
    int64_t a = 0;
    for (int q = 0; q < KG_T; q++) { const int64_t x = tot[q]; tot[q] = a; a += x; }
    Mtot = a;
  }
  __syncthreads();
  const int64_t M = Mtot;
  if (events && t == 0) for (int q = 0; q < 4; q++) events[4 * (lt * P.roles + role) + q] = ev_s[q];
  if (M < L) { if (t == 0) atomicMin(err_trial, (int)lt); return; }
  const int64_t w0 = role == 0 ? M - L : 0;   // the first read keeps the last L bases, the partners the first L (trimRight)
  int64_t o = tot[t];
  int dummy[4] = {0, 0, 0, 0};
  for (int64_t j = lo; j < hi && o < w0 + L; j++) {
    const int64_t base_o = o;
    const int n = ks_walk(P, trial, role, j, ks_src(P, trial, sid, pos, j), e, pi, ps, dummy, [&](int q, uint8_t b) {
      const int64_t x = base_o + q - w0;
      if (x >= 0 && x < L) out[x] = b;
    });
    o += n > 0 ? n : 0;
  }
}

struct KsBufs {
  DevBuf bases, pairs, flags, order, next, scratch, skip, out;
  void release() { bases.release(); pairs.release(); flags.release(); order.release(); next.release(); scratch.release(); skip.release(); out.release(); }
};

// the buffers of one simulation: grow-only across its calls (chunks), released by mhap_ksim_dev_destroy
struct KsDev {
  mhap_handle* h = nullptr;
  KsBufs B;
  DevBuf reads, meta, events, err, ref, ref_off, ref_len;
  int64_t lds_cap = 0;
  int cus = 0;
  void release() { B.release(); reads.release(); meta.release(); events.release(); err.release(); ref.release(); ref_off.release(); ref_len.release(); }
};

// the pair statistics of n pairs whose bytes are at d_bases on the device; hashed[q] (host): pair q takes hashed keys
int ks_stats(KsDev* d, HandleView& v, const char* who, const uint8_t* d_bases, const int64_t* pairs, int64_t n, const int32_t* hashed, int k,
             int bottom_k, const uint8_t* skip, int64_t n_skip, int32_t* out, int32_t* paths) {
  // MHAP_KSIM_HASH_BITS=b (test switch): every pair takes hashed keys narrowed to b bits, so equal keys of different k-mers occur
  uint64_t mask = ~0ULL;
  bool force_hash = false;
  if (const char* e = getenv("MHAP_KSIM_HASH_BITS")) {
    const int b = atoi(e);
    if (b >= 1 && b <= 64) { force_hash = true; mask = b == 64 ? ~0ULL : ((1ULL << b) - 1); }
  }
  std::vector<int32_t> flags((size_t)n), lds, hbm;
  int64_t lds_need = 0, hbm_need = 0;
  for (int64_t q = 0; q < n; q++) {
    const int64_t* p = pairs + 4 * q;
    const bool hsh = force_hash || hashed[q];
    flags[(size_t)q] = hsh ? KS_HASHED : 0;
    const int64_t need = ks_scratch_bytes(p[1], p[3], k, hsh);
    if (need <= d->lds_cap) { lds.push_back((int32_t)q); lds_need = std::max(lds_need, need); }
    else { hbm.push_back((int32_t)q); hbm_need = std::max(hbm_need, need); }
    if (paths) paths[q] = need <= d->lds_cap ? 1 : 2;
  }
  // the skip set: entries of length k, sorted and de-duplicated in byte order
  std::vector<uint8_t> sk;
  int64_t ns = 0;
  if (n_skip > 0) {
    std::vector<int64_t> idx((size_t)n_skip);
    for (int64_t i = 0; i < n_skip; i++) idx[(size_t)i] = i;
    std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return memcmp(skip + a * k, skip + b * k, (size_t)k) < 0; });
    for (size_t i = 0; i < idx.size(); i++) {
      if (i > 0 && memcmp(skip + idx[i] * k, skip + idx[i - 1] * k, (size_t)k) == 0) continue;
      sk.insert(sk.end(), skip + idx[i] * k, skip + idx[i] * k + k);
      ns++;
    }
  }
  std::vector<int32_t> order(lds);
  order.insert(order.end(), hbm.begin(), hbm.end());
  const int grid_lds = (int)std::min<int64_t>((int64_t)lds.size(), 4LL * d->cus);
  int grid_hbm = (int)std::min<int64_t>((int64_t)hbm.size(), 2LL * d->cus);
  const int64_t stride = (hbm_need + 255) / 256 * 256;
  if (stride > 0) grid_hbm = (int)std::max<int64_t>(1, std::min<int64_t>(grid_hbm, ((int64_t)2 << 30) / stride));   // <= 2 GiB of scratch
  KsBufs& B = d->B;
  auto fail = [&](hipError_t e, const char* what) {
    *v.err = std::string(who) + ": " + what + ": " + hipGetErrorString(e);
    return MHAP_E_HIP;
  };
  hipError_t e;
  if ((e = B.pairs.ensure(32 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.flags.ensure(4 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.order.ensure(4 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.next.ensure(8)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.out.ensure(12 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = B.skip.ensure(std::max<int64_t>((int64_t)sk.size(), 1))) != hipSuccess) return fail(e, "hipMalloc");
  if (stride > 0 && (e = B.scratch.ensure((size_t)stride * grid_hbm)) != hipSuccess) return fail(e, "hipMalloc (scratch)");
  if ((e = hipMemcpyAsync(B.pairs.p, pairs, 32 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemcpyAsync(B.flags.p, flags.data(), 4 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemcpyAsync(B.order.p, order.data(), 4 * n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if (!sk.empty() && (e = hipMemcpyAsync(B.skip.p, sk.data(), sk.size(), hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  if ((e = hipMemsetAsync(B.next.p, 0, 8, v.stream)) != hipSuccess) return fail(e, "memset");
  int* nx = B.next.as<int>();
  if (!lds.empty()) {
    (void)hipFuncSetAttribute((const void*)pair_kmer_stats_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_need);
    hipLaunchKernelGGL(pair_kmer_stats_kernel<true>, dim3(grid_lds), dim3(KS_T), (size_t)lds_need, v.stream, d_bases, B.pairs.as<int64_t>(),
                       B.flags.as<int32_t>(), B.order.as<int32_t>(), (int)lds.size(), nx, (uint8_t*)nullptr, (int64_t)0, k, bottom_k,
                       B.skip.as<uint8_t>(), (int)ns, mask, B.out.as<int32_t>());
  }
  if (!hbm.empty())
    hipLaunchKernelGGL(pair_kmer_stats_kernel<false>, dim3(grid_hbm), dim3(KS_T), 0, v.stream, d_bases, B.pairs.as<int64_t>(),
                       B.flags.as<int32_t>(), B.order.as<int32_t>() + lds.size(), (int)hbm.size(), nx + 1, B.scratch.as<uint8_t>(), stride, k,
                       bottom_k, B.skip.as<uint8_t>(), (int)ns, mask, B.out.as<int32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  if ((e = hipMemcpyAsync(out, B.out.p, 12 * n, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail(e, "kernel");
  return MHAP_OK;
}

int ks_check(HandleView& v, const char* who, int64_t n, int k, int bottom_k, int64_t n_skip, const uint8_t* skip) {
  if (n < 0 || n_skip < 0 || (n_skip > 0 && !skip)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (k < 1 || bottom_k < 0) { *v.err = std::string(who) + ": k must be >= 1 and bottom_k >= 0"; return MHAP_E_INVALID; }
  if (n > INT32_MAX / 2 || n_skip > INT32_MAX) { *v.err = std::string(who) + ": too many pairs or skip k-mers in one call"; return MHAP_E_INVALID; }
  return MHAP_OK;
}

}  // namespace
}  // namespace mhap

using namespace mhap;

extern "C" void* mhap_ksim_dev_create(mhap_handle* h) {
  if (!h) return nullptr;
  HandleView v = handle_view(h);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, v.device) != hipSuccess) { *v.err = "mhap_ksim_dev_create: hipGetDeviceProperties failed"; return nullptr; }
  KsDev* d = new KsDev;
  d->h = h;
  d->lds_cap = std::min<int64_t>((int64_t)prop.sharedMemPerBlock, 160 * 1024) - 64;
  d->cus = v.num_cus;   // (the handle's compute units: MHAP_NUM_CUS caps them)
  return d;
}

extern "C" void mhap_ksim_dev_destroy(void* dev) {
  KsDev* d = (KsDev*)dev;
  if (!d) return;
  (void)hipSetDevice(handle_view(d->h).device);
  d->release();
  delete d;
}

extern "C" int mhap_ksim_dev_pair_stats(void* dev, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t k,
                                        int32_t bottom_k, const uint8_t* skip, int64_t n_skip, int32_t* out, int32_t* paths) {
  KsDev* d = (KsDev*)dev;
  if (!d) return MHAP_E_INVALID;
  HandleView v = handle_view(d->h);
  const char* who = "mhap_pair_kmer_stats";
  int rc = ks_check(v, who, n, k, bottom_k, n_skip, skip);
  if (rc != MHAP_OK) return rc;
  if (n_bases < 0 || (n > 0 && (!pairs || !out)) || (n_bases > 0 && !bases)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  std::vector<int32_t> hashed((size_t)n);
  for (int64_t q = 0; q < n; q++) {
    const int64_t* p = pairs + 4 * q;
    for (int f = 0; f < 2; f++) {
      const int64_t off = p[2 * f], len = p[2 * f + 1];
      if (off < 0 || len < 0 || len > (1 << 28) || off > n_bases - len) {
        *v.err = std::string(who) + ": pair " + std::to_string(q) + " has a segment outside the " + std::to_string(n_bases) + " bases";
        return MHAP_E_INVALID;
      }
    }
    bool hsh = k > 31;
    for (int f = 0; f < 2 && !hsh; f++)
      for (int64_t i = 0; i < p[2 * f + 1] && !hsh; i++) {
        const uint8_t c = bases[p[2 * f] + i];
        hsh = !(c == 'A' || c == 'C' || c == 'G' || c == 'T');
      }
    hashed[(size_t)q] = hsh;
  }
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = d->B.bases.ensure(std::max<int64_t>(n_bases, 1))) != hipSuccess) { *v.err = std::string(who) + ": hipMalloc: " + hipGetErrorString(e); return MHAP_E_HIP; }
  if (n_bases > 0 && (e = hipMemcpyAsync(d->B.bases.p, bases, n_bases, hipMemcpyHostToDevice, v.stream)) != hipSuccess) {
    *v.err = std::string(who) + ": upload: " + hipGetErrorString(e);
    return MHAP_E_HIP;
  }
  return ks_stats(d, v, who, d->B.bases.as<uint8_t>(), pairs, n, hashed.data(), k, bottom_k, skip, n_skip, out, paths);
}

extern "C" int mhap_pair_kmer_stats(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t k,
                                    int32_t bottom_k, const uint8_t* skip, int64_t n_skip, int32_t* out, int32_t* paths) {
  if (!h) return MHAP_E_INVALID;
  void* d = mhap_ksim_dev_create(h);
  if (!d) return MHAP_E_HIP;
  const int rc = mhap_ksim_dev_pair_stats(d, bases, n_bases, pairs, n, k, bottom_k, skip, n_skip, out, paths);
  mhap_ksim_dev_destroy(d);
  return rc;
}

extern "C" int mhap_ksim_dev_trials(void* dev, uint64_t seed, int64_t trial0, int64_t n, int32_t length, int32_t offset, double error_rate,
                                    double ins_pct, double del_pct, double sub_pct, int32_t flags, const uint8_t* ref_bases,
                                    const int64_t* ref_offsets, const int32_t* ref_lengths, int64_t n_ref, int32_t k, int32_t bottom_k,
                                    const uint8_t* skip, int64_t n_skip, int32_t* stats, uint8_t* reads, int32_t* meta, int32_t* events,
                                    int64_t* failed_trial) {
  KsDev* d = (KsDev*)dev;
  if (!d) return MHAP_E_INVALID;
  HandleView v = handle_view(d->h);
  const char* who = "mhap_ksim_dev_trials";
  const bool sim_only = flags & MHAP_KSIM_SIM_ONLY;
  if (failed_trial) *failed_trial = -1;
  if (!sim_only) {
    const int rc = ks_check(v, who, 2 * n, k, bottom_k, n_skip, skip);
    if (rc != MHAP_OK) return rc;
  }
  if (n < 0 || trial0 < 0 || length < 1 || n_ref < 0 || n_ref > INT32_MAX || (n_ref > 0 && (!ref_bases || !ref_offsets || !ref_lengths)) ||
      (!sim_only && n > 0 && !stats) || (int64_t)length > (1 << 26)) {
    *v.err = std::string(who) + ": invalid argument";
    return MHAP_E_INVALID;
  }
  if (n == 0) return MHAP_OK;
  const int roles = sim_only ? 1 : 3;
  if (n * roles > INT32_MAX) { *v.err = std::string(who) + ": too many trials in one call"; return MHAP_E_INVALID; }
  bool any4 = n_ref == 0, any2 = n_ref == 0, acgt = true;
  int64_t ref_total = 0;
  for (int64_t r = 0; r < n_ref; r++) {
    if (ref_lengths[r] < 0 || ref_offsets[r] < 0) { *v.err = std::string(who) + ": negative record"; return MHAP_E_INVALID; }
    any4 |= (int64_t)ref_lengths[r] >= 4LL * length;
    any2 |= (int64_t)ref_lengths[r] >= 2LL * length;
    ref_total = std::max<int64_t>(ref_total, ref_offsets[r] + ref_lengths[r]);
  }
  if (!any4 || !any2) { *v.err = std::string(who) + ": no reference record has 4L bases"; return MHAP_E_INVALID; }
  for (int64_t i = 0; i < ref_total && acgt; i++) { const uint8_t c = ref_bases[i]; acgt = c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
  if (error_rate >= 1.0 && !(sub_pct > 0.0) && ins_pct + sub_pct >= 1.0) { *v.err = std::string(who) + ": every draw inserts"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  auto fail = [&](hipError_t er, const char* what) { *v.err = std::string(who) + ": " + what + ": " + hipGetErrorString(er); return MHAP_E_HIP; };
  const int64_t L = length, rbytes = n * roles * L;
  if ((e = d->reads.ensure(rbytes)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->meta.ensure(20 * n)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->events.ensure(16 * n * roles)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->err.ensure(8)) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->ref.ensure(std::max<int64_t>(ref_total, 1))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->ref_off.ensure(8 * std::max<int64_t>(n_ref, 1))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = d->ref_len.ensure(4 * std::max<int64_t>(n_ref, 1))) != hipSuccess) return fail(e, "hipMalloc");
  if (n_ref > 0) {
    if ((e = hipMemcpyAsync(d->ref.p, ref_bases, ref_total, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
    if ((e = hipMemcpyAsync(d->ref_off.p, ref_offsets, 8 * n_ref, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
    if ((e = hipMemcpyAsync(d->ref_len.p, ref_lengths, 4 * n_ref, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  }
  const int32_t big = INT32_MAX;
  if ((e = hipMemcpyAsync(d->err.p, &big, 4, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail(e, "upload");
  const bool one = flags & MHAP_KSIM_ONE_SIDED;
  KgParams P{seed, trial0, length, (int64_t)offset, error_rate, ins_pct, sub_pct, one ? 1 : 0, roles, d->ref.as<uint8_t>(),
             d->ref_off.as<int64_t>(), d->ref_len.as<int32_t>(), (int)n_ref};
  hipLaunchKernelGGL(ksim_gen_kernel, dim3((unsigned)(n * roles)), dim3(KG_T), 0, v.stream, P, d->reads.as<uint8_t>(), d->meta.as<int32_t>(),
                     d->events.as<int32_t>(), d->err.as<int>());
  if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  int32_t bad = big;
  if ((e = hipMemcpyAsync(&bad, d->err.p, 4, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail(e, "generator kernel");
  if (bad != big) {
    if (failed_trial) *failed_trial = trial0 + bad;
    *v.err = std::string(who) + ": trial " + std::to_string(trial0 + bad) + ": a read came out shorter than " + std::to_string(L) +
             " bases (Java: StringIndexOutOfBoundsException)";
    return MHAP_E_INVALID;
  }
  if (reads && (e = hipMemcpyAsync(reads, d->reads.p, rbytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if (meta && (e = hipMemcpyAsync(meta, d->meta.p, 20 * n, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if (events && (e = hipMemcpyAsync(events, d->events.p, 16 * n * roles, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail(e, "download");
  if (sim_only) {
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail(e, "download");
    return MHAP_OK;
  }
  // the same stats kernel as Java mode, on the reads where the generator left them: (first, shared partner), (first, random partner)
  std::vector<int64_t> pairs((size_t)(8 * n));
  std::vector<int32_t> hashed((size_t)(2 * n), (k > 31 || !acgt) ? 1 : 0);
  for (int64_t t = 0; t < n; t++)
    for (int r = 0; r < 2; r++) {
      int64_t* p = &pairs[(size_t)(8 * t + 4 * r)];
      p[0] = 3 * L * t; p[1] = L; p[2] = 3 * L * t + (r + 1) * L; p[3] = L;
    }
  return ks_stats(d, v, who, d->reads.as<uint8_t>(), pairs.data(), 2 * n, hashed.data(), k, bottom_k, skip, n_skip, stats, nullptr);
}

// which path each pair would take with lds_bytes of LDS per workgroup: path[q] = 1 (LDS) or 2 (HBM), the classification of
// mhap_pair_kmer_stats (whose own `paths` output reports the path actually taken on the device); 0 on success
extern "C" int mhap_pair_kmer_stats_paths(const int64_t* pairs, int64_t n, int32_t k, int64_t lds_bytes, int32_t hashed, int32_t* path) {
  if (n < 0 || k < 1 || (n > 0 && (!pairs || !path))) return MHAP_E_INVALID;
  for (int64_t q = 0; q < n; q++) path[q] = ks_scratch_bytes(pairs[4 * q + 1], pairs[4 * q + 3], k, hashed != 0) <= lds_bytes - 64 ? 1 : 2;
  return MHAP_OK;
}
