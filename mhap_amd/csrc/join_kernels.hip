// join_kernels.hip — gfx950 kernels of the second stage: BottomOverlapSketch.getOverlapInfo per candidate pair (hot loop F of SURVEY §3.1).
//
//   overlap_kernel      : one lane per candidate, literal merge (overlap_lane.hpp): the pairs the join path hands back.
//   overlap_join_kernel : one wavefront per candidate, from the equal-hash join — one template over the joined k-mers a pair may have
//                         (OJ_LEVEL_CAP) and the way waves share a staged query (OJ_ALONE / OJ_PAIR / OJ_TEAM).
//   poshist_kernel      : position histograms of an ordered table, for the join kernel's early "below the threshold".
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kernels.hpp"
#include "overlap_lane.hpp"

namespace mhap {

// =============================================================================================
// Second stage.  Persistent lanes: lane g handles candidates g, g+G, ...  Scratch (3 int arrays of
// maxrec entries per lane) is interleaved across lanes so that lanes of a wave touch adjacent words.
// =============================================================================================
// Per-lane streaming view of one ordered-sketch row: the current 64-byte line (8 entries) sits in LDS
// (lane-interleaved 8-byte words), the next line is already in flight into registers.  lane_overlap only walks
// forward between reset()s, so one line + one prefetch hides the HBM/L2 latency of the otherwise dependent loads.
struct CachedView {
  const uint2* row;      // global row: entry i = (hash, pos)
  int n;
  uint2* lds;            // this lane's slot: entry e of the current line at lds[e * OVL_THREADS]
  int cur, nxt;
  uint2 r[8];
  __device__ inline void init(const int32_t* p, int n_, uint2* lds_) { row = (const uint2*)p; n = n_; lds = lds_; cur = -1; nxt = -1; }
  __device__ inline void reset() {}
  __device__ inline void fetch(int line) {
#pragma unroll
    for (int e = 0; e < 8; e++) r[e] = row[line * 8 + e];
  }
  __device__ inline void get(int i, int& h, int& pos) {
    const int line = i >> 3;
    if (line != cur) {
      if (line != nxt) fetch(line);
#pragma unroll
      for (int e = 0; e < 8; e++) lds[e * OVL_THREADS] = r[e];
      cur = line;
      if ((line + 1) * 8 < n) { fetch(line + 1); nxt = line + 1; } else nxt = -1;
    }
    const uint2 v = lds[(i & 7) * OVL_THREADS];
    h = (int)v.x; pos = (int)v.y;
  }
};

__global__ __launch_bounds__(OVL_THREADS) void overlap_kernel(const Candidate* __restrict__ cand, const unsigned long long* __restrict__ cand_count,
                                                              unsigned long long cand_cap, const int32_t* __restrict__ ordered,
                                                              int64_t ord_stride, const int32_t* __restrict__ meta,
                                                              const int32_t* __restrict__ qordered, int64_t qord_stride,
                                                              const int32_t* __restrict__ qmeta, SearchParams sp,
                                                              const double* __restrict__ score_table, int32_t* __restrict__ scratch,
                                                              int64_t scratch_per_lane, DevRecord* __restrict__ recs,
                                                              unsigned long long* __restrict__ rec_count, unsigned long long rec_cap,
                                                              unsigned long long* __restrict__ compared, int spread) {
  __shared__ uint2 lines[2][8 * OVL_THREADS];
  unsigned long long n = *cand_count;
  if (n > cand_cap) n = cand_cap;
  // spread (a power of two <= 64): only every spread-th lane takes pairs.  A handful of pairs — the few the join kernel hands over —
  // packed 64 to a wavefront run in lockstep through each other's branches (4 147 pairs of a c5rank step: 63 ms, on 65 waves of a
  // machine that holds 20 000); one pair per wavefront, they take as long as the longest of them.
  const int64_t gl = (int64_t)blockIdx.x * OVL_THREADS + threadIdx.x;
  if (gl & (int64_t)(spread - 1)) return;
  const int64_t G = (int64_t)gridDim.x * OVL_THREADS / spread;
  const int64_t g = gl / spread;
  LaneScratch sc;
  sc.base = scratch + g;
  sc.stride = G;
  sc.maxrec = (int32_t)(scratch_per_lane / 3);
  unsigned long long mine = 0;
  for (unsigned long long c = (unsigned long long)g; c < n; c += (unsigned long long)G) {
    const Candidate cd = cand[c];
    const int32_t* qm = qmeta + (int64_t)cd.q * META_W;
    const int32_t* mm = meta + (int64_t)cd.m * META_W;
    CachedView A, B;
    A.init(qordered + (int64_t)cd.q * qord_stride, qm[0], &lines[0][threadIdx.x]);
    B.init(ordered + (int64_t)cd.m * ord_stride, mm[0], &lines[1][threadIdx.x]);
    const LaneOverlap r = lane_overlap(A, qm[1], B, mm[1], sp.max_shift, sc);   // MinHashSearch.java:228
    mine++;
    double score = 0.0;
    if (!r.empty) score = score_table[score_index(r.inter, r.kk)];
    if (score >= sp.threshold) {                                                             // :229
      const unsigned long long slot = atomicAdd(rec_count, 1ULL);
      if (slot < rec_cap) {
        DevRecord d;
        d.q = cd.q; d.m = cd.m; d.score = score; d.raw = r.valid; d.a1 = r.a1; d.a2 = r.a2; d.b1 = r.b1; d.b2 = r.b2; d.pad = 0;
        recs[slot] = d;
      }
    }
  }
  if (mine) atomicAdd(compared, mine);
}


// =============================================================================================
// Second stage, one WAVEFRONT per candidate pair (default path).
//
// Both ordered sketches are sorted by (hash, pos), and everything getOverlapInfo does with them is a function of the
// equal-hash JOIN of the two lists: recordMatchingKmers (both passes) keeps the joined k-mers whose positions pass the
// pass's windows, and the bottom-k Jaccard walk counts the joined k-mers inside [a1,a2]x[b1,b2] whose rank in the
// merged union is below k.  So the wave computes the join once — the query's hashes sit in LDS, every lane binary-
// searches the hash of one entry of the other sketch (coalesced 8-byte loads) — and the rest is a handful of wave-wide
// filters, one rank selection (the median shift = Utils.quickSelect's k-th order statistic) and min/max reductions over
// the few joined k-mers.  Per pair that is ~n log n lane steps instead of the ~4n divergent merge steps per LANE of
// overlap_kernel.
//
// A joined hash that is unique inside both sketches contributes at most one record per pass, independent of all other
// hashes (the two-pointer merge has no run there), and record ORDER only matters to optimizeShifts, which merges
// neighbouring records of one query position, i.e. of one hash.  A hash that is duplicated in either sketch forms a
// "group": the merge's run logic (:460-496), optimizeShifts and the one-to-one pairing of the Jaccard walk are replayed
// literally on the group's few entries (oj_group_merge_lane etc.), and its records join the others.  Pairs
// beyond the caps below (joined k-mers, groups, group length) are appended to `slow` for overlap_kernel's literal merge.
// =============================================================================================
#ifndef MH_OJ_WAVES
#define MH_OJ_WAVES 4
#endif
constexpr int OJ_WAVES = MH_OJ_WAVES;
#ifndef MH_OJ_JCAP
#define MH_OJ_JCAP 128   // (the first pass's capacity only)
#endif
// joined k-mers + group records kept per pair (multiples of 64) by the first pass and the two wider ones: the kernel's JCAP.  Inside the
// kernel OJ_JCAP = JCAP and OJ_R = JCAP / 64, the rounds of one entry per lane (a template parameter of the helpers that loop over them).
constexpr int OJ_LEVEL_CAP[OJ_LEVELS] = {MH_OJ_JCAP, 512, 1536};
int overlap_join_capacity(int level) { return OJ_LEVEL_CAP[level]; }
#ifndef MH_OJ_GCAP
#define MH_OJ_GCAP 16   // 12 / 16 with the 6-KB filter: C5 slice 50.6 / 46.9 ms (75 928 / 3 739 pairs handed to the per-lane kernel), c5rank 1004 / 996, C2 3.64 / 3.63
#endif
constexpr int OJ_GCAP = MH_OJ_GCAP;    // duplicated-hash groups per pair
constexpr int OJ_GLEN = 8;             // entries of one sketch in a group
#ifndef MH_OJ_U
#define MH_OJ_U 3
#endif
constexpr int OJ_U = MH_OJ_U;          // 64-entry blocks of the other sketch in flight per wave
#ifndef MH_OJ_PAD
#define MH_OJ_PAD 0   // (experiment: unused ints per wave, to see what the resident waves per CU are worth)
#endif
constexpr int oj_lds_extra(int jcap) { return 3 * jcap + OJ_GCAP * (6 + 2 * OJ_GLEN) + MH_OJ_PAD; }   // ints per wave besides the query hashes
// Round 4: the other sketch's POSITIONS stay in registers from the join's pass over its row (one per lane and 64-entry block: 24 at
// S = 1536), and a shared query's positions are staged in LDS next to its hashes — the two later passes over both rows that the
// bottom-k Jaccard ranks need (nine pairs in ten get that far: -DMH_OJ_STATS) then read no memory at all.  Before: 36 KB per pair
// (the row, then both rows' positions again), now 12.
#ifndef MH_OJ_KEEP
#define MH_OJ_KEEP 1
#endif
// (Also tried in round 4, on top of this: the WHOLE row of the other sketch loaded at once — 24 loads per lane in flight — and looked up
//  in groups of eight blocks: one memory round trip and six LDS round trips per pair instead of eight and sixteen.  168 VGPRs, three
//  waves per SIMD: C2 4.78 -> 6.63 ms, C5 slice 69 -> 91; capped at 128 VGPRs (four waves): 5.24 / 74.8; at two waves 9.0 / 126.  The
//  kernel's time stays inversely proportional to the waves a CU holds; instruction-level parallelism inside a wave does not replace them.)
constexpr int OJ_KB = 24;              // blocks of the other sketch whose positions are kept (S <= 64 * OJ_KB)

__device__ __forceinline__ int oj_mbcnt(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ int oj_wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int oj_wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ void oj_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// MatchData.performUpdate (:191-215) given the median shift of the current records (have = any records)
__device__ __forceinline__ ShiftStats oj_shift_stats(bool have, int med, int len1, int len2, double max_shift) {
  ShiftStats st;
  if (have) {
    st.med = med;
    const int left = 0 > -med ? 0 : -med;
    const int right = len1 < len2 - med ? len1 : len2 - med;
    int ov = right - left; if (ov < 10) ov = 10;
    const int mx = len1 > len2 ? len1 : len2;
    const int lim = (int)((double)ov * max_shift);
    st.absmax = mx < lim ? mx : lim;
  } else {
    st.med = 0;
    st.absmax = (len1 > len2 ? len1 : len2) + 1;
  }
  return st;
}

#ifdef MH_OJ_STATS
// (diagnostic build: where the pairs of the join kernel end — {nj < 3, no record in pass 1, in pass 2, < 3 valid, below the threshold,
//  accepted, sum of nj, sum of in-window joined k-mers of the scored pairs}; printed by launch_overlap_join's caller through oj_stats_dump)
__device__ unsigned long long g_oj_stats[20];
// (the first pass's pairs only: the wider passes see what it handed over, and their exits are not the workload's)
#define OJ_STAT(k, v) do { if constexpr (OJ_JCAP == OJ_LEVEL_CAP[0]) { if (lane == 0) atomicAdd(&g_oj_stats[k], (unsigned long long)(v)); } } while (0)
#else
#define OJ_STAT(k, v) do { } while (0)
#endif
struct OjWindows { int v1lo, v1hi, v2lo, v2hi, med, absmax; };
__device__ __forceinline__ OjWindows oj_windows(ShiftStats st, int len1, int len2) {   // MatchData :246-276
  const int med = st.med, absmax = st.absmax;
  const int t1 = -med - absmax, t2 = len2 - med + absmax, t3 = med - absmax, t4 = len1 + med + absmax;
  OjWindows w;
  w.v1lo = 0 > t1 ? 0 : t1; w.v1hi = len1 < t2 ? len1 : t2;
  w.v2lo = 0 > t3 ? 0 : t3; w.v2hi = len2 < t4 ? len2 : t4;
  w.med = med; w.absmax = absmax;
  return w;
}

// recordMatchingKmers restricted to one hash value that is duplicated in at least one sketch: pa[0..m) / pb[0..n) are the
// positions of ALL entries with that hash (ascending), and the loop below is the reference's, run on just those entries
// (entries of other hashes end a run exactly like the end of these arrays does).  Run by ONE LANE for its own group: a pair of
// repeat-rich reads has half a dozen groups, and replayed one after the other by the whole wave they were a third of the join
// kernel's time on the C5 slice (-DMH_OJ_NO_GROUPS timing build: 69.0 -> 44.9 ms).  Returns the number of records written to o1/o2:
// at most two for every three entries the walk consumes, so a group's records fit the m + n words its entries reserve (oj_pass).
// (Which of a group's positions — eight words per sketch, 16-byte aligned, read as vectors — lie in the pass's windows becomes a bit
// mask per sketch, so the walk's skips and its runs of consecutive in-window entries are bit scans; only the positions the walk
// stops at are read again.  The literal loop read one LDS word per step, every read waiting for the one before: two replays per
// pair were 13 % of the kernel on the C5 slice.  Keeping all sixteen positions in registers and picking them by index was tried:
// 114 VGPRs in the PAIR shape, 92 bytes of scratch in TEAM, slower everywhere.)
__device__ __forceinline__ uint32_t oj_mask4(const int4 v, int lo, uint32_t width) {
  return (((uint32_t)(v.x - lo) < width) ? 1u : 0u) | (((uint32_t)(v.y - lo) < width) ? 2u : 0u) | (((uint32_t)(v.z - lo) < width) ? 4u : 0u) |
         (((uint32_t)(v.w - lo) < width) ? 8u : 0u);
}
__device__ __forceinline__ uint32_t oj_mask8(const int32_t* p, int cnt, int lo, int hi) {   // bit x: entry x < cnt lies in [lo, hi)
  const uint32_t width = hi > lo ? (uint32_t)(hi - lo) : 0u;
  uint32_t m = oj_mask4(*(const int4*)p, lo, width);
  if (cnt > 4) m |= oj_mask4(*(const int4*)(p + 4), lo, width) << 4;
  return m & ((1u << cnt) - 1u);
}
static_assert(OJ_GLEN == 8, "a group's positions are two int4 per sketch");
__device__ __forceinline__ int oj_group_merge_lane(const int32_t* pa, int m, const int32_t* pb, int n, const OjWindows& w, int32_t* o1, int32_t* o2) {
  const uint32_t w1 = oj_mask8(pa, m, w.v1lo, w.v1hi), w2 = oj_mask8(pb, n, w.v2lo, w.v2hi);
  int i1 = 0, i2 = 0, cnt = 0;
  for (;;) {
    const uint32_t r1 = w1 >> i1, r2 = w2 >> i2;
    if (r1 == 0u || r2 == 0u) break;                    // (entries outside their window are stepped over one by one in the reference: no record on the way)
    i1 += __builtin_ctz(r1); i2 += __builtin_ctz(r2);
    const int p1 = pa[i1], p2 = pb[i2];
    const int diff = (p2 - p1) - w.med;
    if (diff > w.absmax) { i1++; continue; }
    if (diff < -w.absmax) { i2++; continue; }
    o1[cnt] = p1; o2[cnt] = p2;
    cnt++;
    // the in-window entries that follow without a gap (:476-490): the last of either run makes a second record
    const int e1 = __builtin_ctz(~(w1 >> (i1 + 1))), e2 = __builtin_ctz(~(w2 >> (i2 + 1)));
    if (e1 | e2) {
      i1 += e1; i2 += e2;
      o1[cnt] = pa[i1]; o2[cnt] = pb[i2];
      cnt++;
    }
    i1++; i2++;
  }
  return cnt;
}
static_assert(OJ_GCAP <= 64, "lane g replays group g");

// One recordMatchingKmers pass over the join.  Entries [0, nj) are the unique-hash joined k-mers (kept if they pass the
// pass's windows); behind them every group owns as many words as it has entries ([gi[4], gi[4] + m + n), nx words in all: laid out
// when the groups were collected), lane g replays group g into the first of them and marks the rest unused — the order of the
// records matters inside a group only (optimizeShifts), so nothing has to be counted or compacted first.  (Round 4's first version
// replayed every group twice — to count, then, after a prefix sum over the lanes, to store contiguously — and groups of fewer than
// three one after the other by the whole wave.)  Bit r of the result = entry r*64+lane is a record of this pass; count = their number.
template <bool FIRST, int OJ_R>
__device__ __forceinline__ uint32_t oj_pass(int32_t* jp1, int32_t* jp2, int nj, int ng, int nx, int32_t* gi, const int32_t* gpa, const int32_t* gpb,
                                           int len1, int len2, ShiftStats st, int lane, int& count) {
  const OjWindows w = oj_windows(st, len1, len2);
  if (ng) {
    if (lane < ng) {
      const int m = gi[lane * 6 + 2], n = gi[lane * 6 + 3], at = gi[lane * 6 + 4];
#ifdef MH_OJ_NO_GMERGE
      const int k = 0;   // (timing experiment; results are wrong)
#else
      const int k = oj_group_merge_lane(gpa + lane * OJ_GLEN, m, gpb + lane * OJ_GLEN, n, w, jp1 + at, jp2 + at);
#endif
      for (int x = k; x < m + n; x++) jp1[at + x] = INT32_MIN;
      gi[lane * 6 + 5] = k;
    }
    oj_lds_sync();
  }
  uint32_t fl = 0;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < OJ_R; r++) {
    if (r * 64 < nj + nx) {
      const int t = r * 64 + lane;
      bool ok = false;
      if (t < nj) {
        // (the first pass's windows are the whole strands and its shift bound max(len1, len2) + 1: every position pair of [0, len1) x [0, len2) passes)
        if (FIRST) ok = true;
        else {
          const int p1 = jp1[t], p2 = jp2[t];
          const int diff = (p2 - p1) - w.med;
          ok = p1 >= w.v1lo && p1 < w.v1hi && p2 >= w.v2lo && p2 < w.v2hi && !(diff > w.absmax) && !(diff < -w.absmax);
        }
      } else if (t < nj + nx) ok = jp1[t] != INT32_MIN;
      fl |= (ok ? 1u : 0u) << r;
      cnt += __popcll(__ballot(ok));
    }
  }
  count = cnt;
  return fl;
}

// k-th smallest (k = count / 2) of the records' shifts = Utils.quickSelect(shifts, count / 2, count): the value, bit by bit from the
// top — of the records still in the running, those with a 0 in the bit are the smaller ones; the k-th is among them or k moves past
// them.  The records' lanes are scalar masks, so a bit costs two vector instructions per round of 64 records and a handful of scalar
// ones: 15 bits for 10-kb reads.  (Round 3 counted, for every record, the records below it — one LDS broadcast and four vector
// instructions per record and round: with the 40 records of a typical C2 pair, three times the instructions; and this kernel is
// bound by the instructions it issues — at five waves per SIMD more resident waves no longer help it.  That way stays for pairs
// of a dozen records or fewer, where it is the shorter one.)
// A shift is p2 - p1 with 0 <= p1 < len1, 0 <= p2 < len2: biased by 2^lb > max(len1, len2) it is a positive (lb + 1)-bit number.
constexpr int OJ_MED_SMALL = 12;   // up to this many records the median is found by counting (below)
template <int OJ_R>
__device__ __forceinline__ int oj_median_shift(const int32_t* jp1, const int32_t* jp2, int32_t* sh, uint32_t fl, int ntot, int count, int lane, int lb) {
  if (count <= OJ_MED_SMALL) {
    // a handful of records (a pair that shares a repeat's k-mers and nothing else): every record counts the records below it —
    // one LDS broadcast and a few instructions per record, fewer than the lb + 1 bit steps
    int myv[OJ_R], myidx[OJ_R], less[OJ_R];
    int base = 0;
#pragma unroll
    for (int r = 0; r < OJ_R; r++) {
      myv[r] = 0; myidx[r] = 0; less[r] = 0;
      if (r * 64 < ntot) {
        const bool ok = (fl >> r) & 1u;
        const unsigned long long bal = __ballot(ok);
        if (ok) {
          const int t = r * 64 + lane;
          myv[r] = jp2[t] - jp1[t];
          myidx[r] = base + oj_mbcnt(bal);
          sh[myidx[r]] = myv[r];
        }
        base += __popcll(bal);
      }
    }
    oj_lds_sync();
    for (int u = 0; u < count; u++) {
      const int v = sh[u];   // same address in every lane: LDS broadcast
#pragma unroll
      for (int r = 0; r < OJ_R; r++)
        if (r * 64 < ntot) less[r] += (v < myv[r] || (v == myv[r] && u < myidx[r])) ? 1 : 0;
    }
    const int k = count / 2;
    int med = 0;
#pragma unroll
    for (int r = 0; r < OJ_R; r++) {
      if (r * 64 < ntot) {
        const unsigned long long bal = __ballot(((fl >> r) & 1u) && less[r] == k);
        if (bal) med = __builtin_amdgcn_readlane(myv[r], __builtin_amdgcn_readfirstlane(__builtin_ctzll(bal)));
      }
    }
    __builtin_amdgcn_wave_barrier();
    return med;
  }
  uint32_t key[OJ_R];
  unsigned long long in[OJ_R];
  const uint32_t bias = 1u << lb;
#pragma unroll
  for (int r = 0; r < OJ_R; r++) {
    key[r] = 0u; in[r] = 0ULL;
    if (r * 64 < ntot) {
      const bool ok = (fl >> r) & 1u;
      if (ok) { const int t = r * 64 + lane; key[r] = (uint32_t)(jp2[t] - jp1[t]) + bias; }
      in[r] = __builtin_amdgcn_ballot_w64(ok);
    }
  }
  int k = count / 2;
  uint32_t res = 0u;
  for (int b = lb; b >= 0; b--) {
    const uint32_t bit = 1u << b;
    unsigned long long one[OJ_R];
    int c0 = 0;
#pragma unroll
    for (int r = 0; r < OJ_R; r++) {
      one[r] = 0ULL;
      if (r * 64 < ntot) { one[r] = __builtin_amdgcn_ballot_w64((key[r] & bit) != 0u); c0 += __popcll(in[r] & ~one[r]); }
    }
    if (k < c0) {
#pragma unroll
      for (int r = 0; r < OJ_R; r++) in[r] &= ~one[r];
    } else {
      k -= c0; res |= bit;
#pragma unroll
      for (int r = 0; r < OJ_R; r++) in[r] &= one[r];
    }
  }
  return (int)(res - bias);
}

// Rank of entry idx (of the current chunk of OJ_RCH blocks) among the in-window entries ahead of it: lane b of the wave holds block
// b's in-window mask and the in-window count of the blocks before it.
extern "C" __device__ int oj_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");   // v_writelane_b32 (this clang has no builtin for it)
// bit of a hash value in a filter of ts <= 65 536 bits: the low 16 bits of the value (uniform, whatever end of the hash range the sketch keeps)
// scaled onto [0, ts) — ts need not be a power of two, so the filter can take exactly the LDS a workgroup has to spare
__device__ __forceinline__ uint32_t oj_filter_bit(uint32_t h, uint32_t ts) { return (uint32_t)__umul24(h & 0xFFFFu, ts) >> 16; }   // (HIP declares __umul24 as int)
constexpr int OJ_CQ = 256;              // ring of entry indices that passed the query's filter (FILTER shapes; it lives in jp1's words during the join)
static_assert(OJ_CQ * 2 <= OJ_LEVEL_CAP[0] * 4 && OJ_CQ >= 64 * OJ_U + 64, "the ring fits the smallest jp1 and takes a trip's entries on top of an unhandled rest");
constexpr int OJ_RCH = (64 / OJ_U) * OJ_U;   // blocks of a chunk: whole trips of OJ_U blocks, one block per lane
// The last block of a sketch whose length is no multiple of 64: its lanes past the end took part in the ballot with whatever they held.
// Trimmed once after the pass (the block's mask sits in lane `blk`; no later block's prefix depends on it) instead of tested in every block.
__device__ __forceinline__ void oj_trim_last_block(uint32_t& mlo, uint32_t& mhi, int& total, int blk, int valid) {
  const unsigned long long m = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mhi, blk) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mlo, blk);
  const unsigned long long keep = m & ((1ULL << valid) - 1ULL);
  total -= __popcll(m ^ keep);
  mlo = (uint32_t)oj_writelane((int)(uint32_t)keep, blk, (int)mlo);
  mhi = (uint32_t)oj_writelane((int)(uint32_t)(keep >> 32), blk, (int)mhi);
}
__device__ __forceinline__ int oj_rank_from(uint32_t mlo, uint32_t mhi, int mpre, int idx) {
  const int src = (idx >> 6) & 63;
  const uint32_t lo = (uint32_t)__shfl((int)mlo, src), hi = (uint32_t)__shfl((int)mhi, src);
  const int pre = __shfl(mpre, src);
  const unsigned long long m = (((unsigned long long)hi << 32) | (unsigned long long)lo) & ((1ULL << (idx & 63)) - 1ULL);
  return pre + __popcll(m);
}

// Lookup of a hash among the query's sorted hashes, in LDS.  The hashes of a bottom-S sketch are uniform order statistics of
// [first, last], so  bucket(h) = (h - first) * NB / (last - first + 1)  spreads them evenly; st[b] = index of the first entry
// whose bucket is >= b (NB + 1 16-bit words, NB >= 2 S: 0.375 entries per bucket at the defaults).  A lookup reads st[b] and
// st[b + 1], then the bucket's first two hashes — two dependent LDS round trips, the same for every lane — and only a bucket of
// three or more entries (0.7 % of them) costs a lane more.  Equal hashes share a bucket and the scan ascends, so a hit is the
// FIRST entry with that hash, as the lower bound was.  Round 2 found every entry of the other sketch by binary search: eleven
// dependent round trips per entry, 36 % of this kernel at the C5 slice and 24 % at C2 (-DMH_OJ_JOIN_ONLY / -DMH_OJ_NO_SEARCH
// timing builds).  (An open-addressing hash table was tried first: the probe chains' MAXIMUM over the 64 lanes, not their mean,
// sets a wave's time — 8.0 ms at C2 against the binary search's 4.7.)
// ---- position histograms: an exact early "below the threshold" for the join kernel ---------------------------------------------
// Nine in ten pairs of every workload measured end BELOW THE THRESHOLD, after the two extra passes over both rows that the bottom-k
// Jaccard needs (the ranks of the joined k-mers among the in-window entries; -DMH_OJ_STATS: 408 050 of 451 976 pairs at C2,
// 7.1 M of 8.3 M on one rank's share of configs[4]).  A pair's score is score_table[inter, kk] with inter <= J, the joined k-mers
// inside both windows, and kk = min(in-window entries of either sketch).  A cumulative histogram of the positions of a sketch's
// entries (64 bins over the strand, 128 bytes per entry) bounds the in-window counts from below with two 16-bit loads per sketch;
// pass_min[kk] = the smallest inter that reaches the threshold for any kk' >= kk (from the score table itself, on the host: no
// monotonicity is assumed).  J < pass_min[kk_lb] => the pair cannot be accepted whatever the ranks are: it ends EMPTY-scored here.
constexpr int PH_BINS = 64;
__global__ __launch_bounds__(256) void poshist_kernel(const int32_t* __restrict__ ordered, int64_t stride, const int32_t* __restrict__ meta, int64_t n,
                                                      uint16_t* __restrict__ out) {
  __shared__ uint32_t hist[4][PH_BINS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 4 + wv;
  if (e >= n) return;
  const int32_t* mm = meta + e * META_W;
  const int ne = mm[3] == 0 ? mm[0] : 0, len = mm[1];
  const int w = len > 0 ? (len + PH_BINS - 1) / PH_BINS : 1;
  hist[wv][lane] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint2* row = (const uint2*)(ordered + e * stride);
  for (int j = lane; j < ne; j += 64) {
    const int pos = (int)row[j].y;
    int b = pos > 0 ? pos / w : 0;
    b = b < PH_BINS - 1 ? b : PH_BINS - 1;
    atomicAdd(&hist[wv][b], 1u);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  uint32_t v = hist[wv][lane];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(v, off); if (lane >= off) v += t; }
  out[e * PH_BINS + lane] = (uint16_t)v;
}
void launch_poshist(hipStream_t st, const int32_t* ordered, int64_t stride, const int32_t* meta, int64_t n, uint16_t* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(poshist_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, ordered, stride, meta, n, out);
}
// entries with a position in [x, y], from below: the bins that lie inside the window (bin b = positions [b w, (b + 1) w))
__device__ __forceinline__ int ph_count_lb(const uint16_t* __restrict__ ph, int len, int x, int y) {
  if (y < x) return 0;
  const int w = len > 0 ? (len + PH_BINS - 1) / PH_BINS : 1;
  const int fb = (x + w - 1) / w;
  int lb = (y + 1) / w;                      // bins [fb, lb) are inside: whole bins among 0 .. 62 ...
  lb = lb < PH_BINS - 1 ? lb : PH_BINS - 1;
  if (y + 1 >= len) lb = PH_BINS;            // ... and the last one, which holds everything from 63 w on, when the window reaches the strand's end
  if (lb <= fb) return 0;
  return (int)ph[lb - 1] - (fb > 0 ? (int)ph[fb - 1] : 0);
}

struct OjBuckets { int first, last; uint32_t mult; };
__device__ __forceinline__ OjBuckets oj_buckets(int first, int last, int nb) {
  OjBuckets k;
  k.first = first; k.last = last;
  unsigned long long range = (unsigned long long)(uint32_t)(last - first) + 1ULL;
  if (range < 2ULL * (unsigned long long)nb) range = 2ULL * (unsigned long long)nb;   // (keeps mult below 2^32; a degenerate sketch uses fewer buckets)
  k.mult = (uint32_t)(((unsigned long long)nb << 32) / range);
  return k;
}
__device__ __forceinline__ int oj_bucket_of(const OjBuckets& k, int h) { return (int)__umulhi((uint32_t)(h - k.first), k.mult); }
int overlap_join_table_slots(int S) { int t = 1024; while (t < 2 * S) t <<= 1; return t; }
// bits of a query's filter: 8 per entry where LDS bounds the resident waves (PAIR: 12 % of the other sketch's entries pass), 32 where registers do (TEAM: 3 %)
int overlap_join_filter_bits(int S, int waves) {
  int per = waves == 4 ? 32 : 8;   // (power-of-two filters — TEAM, C5 slice: 16 384 / 32 768 / 65 536 bits 57.3 / 55.3 / 53.2 ms; PAIR, C2: 8 192 / 16 384 / 32 768: 4.04 / 3.75 /
                                   //  3.95.  TEAM's 49 152 bits = 6 KB leave the LDS that sixteen groups per pair need with five workgroups on a CU)
  if (const char* e = getenv("MHAP_OJ_FILTER_BPE")) { const int x = atoi(e); if (x >= 1 && x <= 64) per = x; }   // (experiments)
  long long t = ((long long)per * S + 127) & ~127LL;   // (whole 16-byte vectors of LDS)
  if (t < 1024) t = 1024;
  if (t > 65536) t = 65536;                            // (oj_filter_bit maps sixteen bits of the hash)
  return (int)t;
}

typedef int oj_keep_t __attribute__((ext_vector_type(12)));   // (vectors, not an array: with a dynamic index an array of this size goes to scratch in this kernel; two of
                                                              //  twelve: a vector of 24 takes 32 registers, and up to eight elements the compiler picks by compare and select)
static_assert(OJ_KB == 24 && 12 % OJ_U == 0, "two vectors of twelve blocks, whole trips each");
// The kept positions are addressed by a wave-uniform trip number: s_set_gpr_idx_on / v_mov / s_set_gpr_idx_off, three instructions per
// element.  (History: a switch over static indices kept the array in registers too, but the compiler merged its cases through copies of the
// WHOLE array, a dozen to two dozen v_mov per trip of the streaming loop — found in the ISA when a probe showed that loop at 3.5 TB/s where
// bare row gathers reach 6.1, tools/row_gather_probe.hip; and the stores, written as `block < 12 ? first vector : second`, did the same
// between the two vectors until the streaming loops were split by vector — see `trip` in the kernel.)
#define OJ_KEEP_LOAD(it, pbk, posv) { const int b_ = (it) * OJ_U;                                                               \
    if (b_ < 12) { _Pragma("unroll") for (int u_ = 0; u_ < OJ_U; u_++) posv[u_] = pbk[0][b_ + u_]; }                              \
    else if (b_ < 24) { _Pragma("unroll") for (int u_ = 0; u_ < OJ_U; u_++) posv[u_] = pbk[1][b_ - 12 + u_]; }                    \
    else { _Pragma("unroll") for (int u_ = 0; u_ < OJ_U; u_++) posv[u_] = INT32_MIN; } }

// SHARED = true : a WORKGROUP pulls chunks of candidates; for every run of one query inside the chunk its WAVES waves stage the
//                 query's hashes (and, TABLE, build the bucket table) together — one copy in LDS — then take the run's candidates one
//                 by one from an LDS counter.
// SHARED = false: every wave works alone — pulls its own chunks, keeps its own hashes.
// (the shapes in use and what each is for: OJ_ALONE / OJ_PAIR / OJ_TEAM below)
// (the TEAM shape — candidate-rich queries, pairs with many duplicated-hash groups — collects three groups per round, which costs it
//  registers: it is held at 96 VGPRs = five waves per SIMD, 8-16 B of scratch; the other shapes keep the one-group loop and their 93)
#ifndef MH_OJ_TEAM_MINW
#define MH_OJ_TEAM_MINW 5
#endif
#ifndef MH_OJ_MINW
#define MH_OJ_MINW 4   // waves per SIMD the shapes without the table are compiled for
#endif
template <int JCAP, bool SHARED, int WAVES, bool TABLE, bool FILTER>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WAVES == 4 ? MH_OJ_TEAM_MINW : MH_OJ_MINW, 8))) void overlap_join_kernel(const Candidate* __restrict__ cand, const unsigned long long* __restrict__ cand_count,
                                                                     unsigned long long cand_cap, const int32_t* __restrict__ ordered,
                                                                     int64_t ord_stride, const int32_t* __restrict__ meta,
                                                                     const int32_t* __restrict__ qordered, int64_t qord_stride,
                                                                     const int32_t* __restrict__ qmeta, SearchParams sp,
                                                                     const double* __restrict__ score_table, DevRecord* __restrict__ recs,
                                                                     unsigned long long* __restrict__ rec_count, unsigned long long rec_cap,
                                                                     unsigned long long* __restrict__ compared, Candidate* __restrict__ slow,
                                                                     unsigned long long* __restrict__ slow_count, int chunk,
                                                                     unsigned long long* __restrict__ work, int ts,
                                                                     const uint16_t* __restrict__ ph, const uint16_t* __restrict__ qph,
                                                                     const int32_t* __restrict__ pass_min) {
  extern __shared__ int32_t oj_lds[];
  static_assert(JCAP % 64 == 0 && JCAP >= OJ_LEVEL_CAP[0], "whole rounds of one entry per lane; the levels' capacities ascend");
  constexpr int OJ_JCAP = JCAP, OJ_R = JCAP / 64, OJ_LDS_EXTRA = oj_lds_extra(JCAP);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr bool APOS = SHARED && MH_OJ_KEEP;                          // the shared query's positions are staged too
  const bool keepb = MH_OJ_KEEP && sp.S <= 64 * OJ_KB;                 // the other sketch's positions stay in registers
  static_assert(!(TABLE && FILTER) && (!FILTER || SHARED), "one lookup aid per shape; the filter is built by a workgroup");
  const int tabw = TABLE ? (ts / 2 + 4) & ~3 : (FILTER ? ts / 32 : 0);  // ints of the table (ts + 1 shorts, padded: what follows stays 16-byte aligned) / of the filter (ts bits)
  const int spad = (sp.S + 3) & ~3, own = spad + tabw + (APOS ? spad : 0);   // ints of the hashes (+ the table / the filter) (+ the positions)
  int32_t* ah = SHARED ? oj_lds : oj_lds + (size_t)wv * (own + OJ_LDS_EXTRA);   // the query sketch's hashes,
  uint16_t* st = (uint16_t*)(ah + spad);                               // ... (TABLE) the bucket starts over them,
  uint32_t* bm = (uint32_t*)(ah + spad);                               // ... (FILTER) a bit per hash value mod ts,
  int32_t* ap = ah + spad + tabw;                                      // ... (APOS) its positions,
  int32_t* svar = oj_lds + own;                                        // (SHARED) {-, next candidate of the run, chunk start lo, hi}
  int32_t* jp1 = SHARED ? svar + 4 + (size_t)wv * OJ_LDS_EXTRA : ah + own;   // per wave — join: position in the query / in the other sketch,
  int32_t* jp2 = jp1 + OJ_JCAP;
  uint16_t* cq = (uint16_t*)jp1;                                       // (FILTER, during the join: jp1 is filled after it) ring of OJ_CQ entry indices that passed the filter
  uint32_t* jij = (uint32_t*)(jp2 + OJ_JCAP);                          // ... entry indices (i | j << 16)
  int32_t* sh = (int32_t*)jij;                                         // (later) shifts of the current records, median by counting
  int32_t* gi = (int32_t*)(jij + OJ_JCAP);                             // groups: {first i, first j, m, n, first record, records}
  int32_t* gpa = gi + OJ_GCAP * 6;                                     // ... positions of the group's entries in the query
  int32_t* gpb = gpa + OJ_GCAP * OJ_GLEN;                              // ... and in the other sketch
  OjBuckets bk = {0, 0, 0u};
  unsigned long long n = *cand_count;
  if (n > cand_cap) n = cand_cap;
  int curq = -1, nA = 0, len1 = 0;
  const int32_t* qrow = nullptr;
  unsigned long long mine = 0;
  constexpr int NT = SHARED ? 64 * WAVES : 64;                      // threads that stage one query
  const int tid = SHARED ? (int)threadIdx.x : lane;
  // one candidate pair, by the wave
  auto one_candidate = [&](const Candidate cd) {
      const int32_t* mm = meta + (int64_t)cd.m * META_W;
      const int nB = __builtin_amdgcn_readfirstlane(mm[0]), len2 = __builtin_amdgcn_readfirstlane(mm[1]);
      const uint2* brow = (const uint2*)(ordered + (int64_t)cd.m * ord_stride);
      // ---- join ----
      int nj = 0, ng = 0;
      bool bad = false, bad_groups = false;   // bad_groups: handed over for the duplicated-hash group caps (a wider pass would hand the pair on again)
      oj_keep_t pbk[2];      // (keepb) positions of the other sketch: entry blk * 64 + lane in pbk[blk / 12][blk % 12]
      if (nA > 0 && nB > 0) {
        if constexpr (FILTER) {
        // Filter, compact, look up.  1 entry in 40 of the other sketch has a partner in the query (a true overlap; a handful for a pair that
        // shares a repeat), but a wave looked all 64 entries of a block up and went through the found-entry code for nearly every block.
        // Now a block costs one LDS word per entry — the query's filter, a bit per hash value mod ts: 5-9 % of the entries pass — and
        // the indices of those that pass are queued (a ring of OJ_CQ 16-bit words); whenever 64 are waiting they are handled as ONE
        // dense block: entry and neighbours re-read (L2), bisection among the query's hashes, run / group detection.  At S = 1536 that
        // is three or four dense blocks per pair instead of twenty-four sparse ones.
        const int p2 = 1 << (31 - __builtin_clz((unsigned)nA));   // largest power of two <= nA
        int qn = 0, qd = 0, kit = 0;   // entries queued / handled (wave-uniform)
        // (loads past the sketch's end read its last entry again — no bounds branch around a load; what such lanes queue is dropped when the
        //  queue is handled, and the rank pass trims the last block's mask)
        uint2 en[OJ_U];
#pragma unroll
        for (int u = 0; u < OJ_U; u++) { const int j = u * 64 + lane; en[u] = brow[j < nB ? j : nB - 1]; }
        // One trip of the streaming loop (returns false after the row's last one).  The kept positions of a trip go to ONE of the two
        // twelve-element vectors, and which one is static at each of the three places the trip is instantiated from below: written as one
        // loop with `block < 12 ? pbk[0] : pbk[1]` the compiler joined the two cases through copies of a whole vector — six to eighteen
        // v_mov_b64 in every trip (read in the ISA, round 5).
        auto trip = [&](const int j0, auto WHICH) -> bool {
          constexpr int which = decltype(WHICH)::value;   // 0 / 1: the vector this trip's positions are kept in; 2: none (beyond OJ_KB blocks)
          const bool more = j0 < nB && !bad;
          if (more) {
            uint2 e[OJ_U];
            uint32_t w[OJ_U];
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              e[u] = en[u];
              const int jn = j0 + (u + OJ_U) * 64 + lane;
              en[u] = brow[jn < nB ? jn : nB - 1];
            }
            if (keepb && which < 2) {
              const int b_ = (kit - (12 / OJ_U) * which) * OJ_U;   // 0, 3, 6, 9 inside the vector
#pragma unroll
              for (int u = 0; u < OJ_U; u++) pbk[which < 2 ? which : 0][b_ + u] = (int)e[u].y;
              kit++;
            }
            uint32_t fb[OJ_U];
#pragma unroll
            for (int u = 0; u < OJ_U; u++) { fb[u] = oj_filter_bit(e[u].x, (uint32_t)ts); w[u] = bm[fb[u] >> 5]; }
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int jb = j0 + u * 64;
              if (jb < nB) {
#ifdef MH_OJ_NO_SEARCH
                const bool c = (e[u].x ^ e[u].y) == 0x7ffffffeu && w[u] == 0x12345u;   // (timing experiment: the rows are streamed, nothing passes the filter; results are wrong)
#else
                const bool c = ((w[u] >> (fb[u] & 31u)) & 1u) != 0u;
#endif
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(c);
                if (bal) {
                  if (c) cq[(qn + oj_mbcnt(bal)) & (OJ_CQ - 1)] = (uint16_t)(jb + lane);
                  qn += __popcll(bal);
                }
              }
            }
          }
          // whole blocks of queued entries — at the row's end whatever is left.  (A trip adds at most 64 OJ_U entries to at most 63.)
          while (!bad && (qn - qd >= 64 || (!more && qn > qd))) {
            oj_lds_sync();
            const int cnt = qn - qd < 64 ? qn - qd : 64;
            bool act = lane < cnt;
            int j = 0, hb = 0, pb = 0, hprev = 0, hnext = 0;
            if (act) j = cq[(qd + lane) & (OJ_CQ - 1)];
            act = act && j < nB;                       // (the last block's lanes past the sketch's end queue themselves too)
            if (act) {
              const uint2 be = brow[j];
              hb = (int)be.x; pb = (int)be.y;
              if (j > 0) hprev = (int)brow[j - 1].x;
              if (j + 1 < nB) hnext = (int)brow[j + 1].x;
            }
            qd += cnt;
            int l = (ah[p2 - 1] < hb) ? nA - p2 : -1;   // lower bound by bisection: fixed probe sequence for a sorted array of any length
            for (int q = p2 >> 1; q > 0; q >>= 1) l = (ah[l + q] < hb) ? l + q : l;
            l += 1;
            const bool found = act && l < nA && ah[l < nA ? l : 0] == hb;
            if (__builtin_amdgcn_ballot_w64(found)) {
              // the first entry of a run of equal hashes in the other sketch speaks for the run
              const bool leader = found && !(j > 0 && hprev == hb);
              bool grp = false;
              if (leader) grp = (l + 1 < nA && ah[l + 1] == hb) || (j + 1 < nB && hnext == hb);
              const bool reg = leader && !grp;
              const unsigned long long balr = __builtin_amdgcn_ballot_w64(reg), balg = __builtin_amdgcn_ballot_w64(grp);
              if (nj + __popcll(balr) > OJ_JCAP || ng + __popcll(balg) > OJ_GCAP) { bad = true; bad_groups = bad_groups || ng + __popcll(balg) > OJ_GCAP; OJ_STAT(ng + __popcll(balg) > OJ_GCAP ? 15 : 14, 1); }
              else {
                if (reg) {
                  const int idx = nj + oj_mbcnt(balr);
                  jp2[idx] = pb;
                  jij[idx] = (uint32_t)l | ((uint32_t)j << 16);
                }
                if (grp) {
                  const int idx = ng + oj_mbcnt(balg);
                  gi[idx * 6 + 0] = l; gi[idx * 6 + 1] = j;
                }
                nj += __popcll(balr);
                ng += __popcll(balg);
              }
            }
          }
          return more;
        };
        {
          static_assert(12 % OJ_U == 0, "whole trips per kept vector");
          constexpr int TPV = 12 / OJ_U;   // trips per kept vector
          int j0 = 0;
          bool go = true;
          for (int t = 0; go && t < TPV; t++, j0 += 64 * OJ_U) go = trip(j0, std::integral_constant<int, 0>());
          for (int t = 0; go && t < TPV; t++, j0 += 64 * OJ_U) go = trip(j0, std::integral_constant<int, 1>());
          for (; go; j0 += 64 * OJ_U) go = trip(j0, std::integral_constant<int, 2>());
        }
        } else {
        int carry = 0;   // hash of the last entry of the previous OJ_U blocks (run detection across blocks)
        int kit = 0;
        uint2 en[OJ_U];
#pragma unroll
        for (int u = 0; u < OJ_U; u++) { const int j = u * 64 + lane; en[u] = make_uint2(0u, 0u); if (j < nB) en[u] = brow[j]; }
#ifdef MH_OJ_NO_SEARCH
        for (int j0 = 0; j0 < nB && !bad; j0 += 64 * OJ_U) {   // (timing experiment: the rows are streamed, nothing is looked up)
          int acc = 0;
#pragma unroll
          for (int u = 0; u < OJ_U; u++) { acc += (int)en[u].x; const int jn = j0 + (u + OJ_U) * 64 + lane; en[u] = make_uint2(0u, 0u); if (jn < nB) en[u] = brow[jn]; }
          if (acc == 0x7fffffff) bad = true;
        }
        const int jstart = nB;
#else
        const int jstart = 0;
#endif
        // (one trip; the vector its positions are kept in is static at each place it is instantiated from, as in the filter branch above)
        auto trip = [&](const int j0, auto WHICH) {
          constexpr int which = decltype(WHICH)::value;
          // OJ_U blocks of 64 entries at a time: their binary searches (dependent LDS reads) overlap each other and the loads
          // of the next OJ_U blocks
          uint2 e[OJ_U];
          int l[OJ_U];
#pragma unroll
          for (int u = 0; u < OJ_U; u++) {
            e[u] = en[u];
            const int jn = j0 + (u + OJ_U) * 64 + lane;
            en[u] = make_uint2(0u, 0u);
            if (jn < nB) en[u] = brow[jn];
          }
          if (keepb && which < 2) {
            const int b_ = (kit - (12 / OJ_U) * which) * OJ_U;
#pragma unroll
            for (int u = 0; u < OJ_U; u++) pbk[which < 2 ? which : 0][b_ + u] = (int)e[u].y;
            kit++;
          }
          bool found[OJ_U];
          bool anyf = false;
          if constexpr (TABLE) {
            // bucket lookup (above): st[b], st[b + 1], then the bucket's first two hashes — the OJ_U entries' reads are independent
            int i0[OJ_U], i1[OJ_U], x0[OJ_U], x1[OJ_U];
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int hb = (int)e[u].x;
              const int b = (hb >= bk.first && hb <= bk.last) ? oj_bucket_of(bk, hb) : 0;
              i0[u] = st[b]; i1[u] = st[b + 1];
            }
#pragma unroll
            for (int u = 0; u < OJ_U; u++) { x0[u] = ah[i0[u]]; x1[u] = ah[i0[u] + 1]; }   // (past the bucket / the sketch: read, never used)
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int j = j0 + u * 64 + lane;
              const int hb = (int)e[u].x;
              l[u] = -1;
              if (j < nB && hb >= bk.first && hb <= bk.last && i0[u] < i1[u]) {
                if (x0[u] == hb) l[u] = i0[u];
                else if (i0[u] + 1 < i1[u]) {
                  if (x1[u] == hb) l[u] = i0[u] + 1;
                  else for (int i = i0[u] + 2; i < i1[u]; i++) if (ah[i] == hb) { l[u] = i; break; }
                }
              }
              found[u] = l[u] >= 0;
              anyf |= found[u];
            }
          } else {
            // no table (its 8 KB would cost resident waves, and this kernel's time is inversely proportional to them): lower bound of every hash among the query's by binary search, l = last index whose hash
            // is smaller (-1: none).  Fixed probe sequence for a sorted array of any length (the first probe splits [0, nA) into two
            // overlapping halves of p2 entries); the OJ_U searches' dependent LDS reads overlap each other
            const int p2 = 1 << (31 - __builtin_clz((unsigned)nA));   // largest power of two <= nA
#pragma unroll
            for (int u = 0; u < OJ_U; u++) l[u] = (ah[p2 - 1] < (int)e[u].x) ? nA - p2 : -1;
            for (int q = p2 >> 1; q > 0; q >>= 1) {
#pragma unroll
              for (int u = 0; u < OJ_U; u++) l[u] = (ah[l[u] + q] < (int)e[u].x) ? l[u] + q : l[u];
            }
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int j = j0 + u * 64 + lane;
              l[u] += 1;
              found[u] = j < nB && l[u] < nA && ah[l[u] < nA ? l[u] : 0] == (int)e[u].x;
              anyf |= found[u];
            }
          }
#ifdef MH_OJ_NO_FOUND
          { int acc = 0;   // (timing experiment: the lookups are done, what they find is dropped; results are wrong)
#pragma unroll
            for (int u = 0; u < OJ_U; u++) acc ^= l[u] + (found[u] ? 7 : 0);
            if (acc == 0x12345678) bad = true;
            anyf = false; }
#endif
          if (__any(anyf)) {
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              if (!bad && __any(found[u])) {
                const int j = j0 + u * 64 + lane;
                const int hb = (int)e[u].x;
                int hprev = __shfl_up(hb, 1);
                if (lane == 0) hprev = u ? __builtin_amdgcn_readlane((int)e[u ? u - 1 : 0].x, 63) : carry;
                // the first entry of a run of equal hashes in the other sketch speaks for the run
                const bool leader = found[u] && !(j > 0 && hprev == hb);
                int hnext = __shfl_down(hb, 1);
                if (lane == 63 && leader && j + 1 < nB) hnext = (int)brow[j + 1].x;
                bool grp = false;
                if (leader) grp = (l[u] + 1 < nA && ah[l[u] + 1] == hb) || (j + 1 < nB && hnext == hb);
                const bool reg = leader && !grp;
                const unsigned long long balr = __ballot(reg), balg = __ballot(grp);
                if (nj + __popcll(balr) > OJ_JCAP || ng + __popcll(balg) > OJ_GCAP) { bad = true; bad_groups = bad_groups || ng + __popcll(balg) > OJ_GCAP; }
                else {
                  if (reg) {
                    const int idx = nj + oj_mbcnt(balr);
                    jp2[idx] = (int)e[u].y;
                    jij[idx] = (uint32_t)l[u] | ((uint32_t)j << 16);
                  }
                  if (grp) {
                    const int idx = ng + oj_mbcnt(balg);
                    gi[idx * 6 + 0] = l[u]; gi[idx * 6 + 1] = j;
                  }
                  nj += __popcll(balr);
                  ng += __popcll(balg);
                }
              }
            }
          }
          carry = __builtin_amdgcn_readlane((int)e[OJ_U - 1].x, 63);
        };
        {
          constexpr int TPV = 12 / OJ_U;
          int j0 = jstart;
          for (int t = 0; t < TPV && j0 < nB && !bad; t++, j0 += 64 * OJ_U) trip(j0, std::integral_constant<int, 0>());
          for (int t = 0; t < TPV && j0 < nB && !bad; t++, j0 += 64 * OJ_U) trip(j0, std::integral_constant<int, 1>());
          for (; j0 < nB && !bad; j0 += 64 * OJ_U) trip(j0, std::integral_constant<int, 2>());
        }
        }
      }
      oj_lds_sync();
#ifdef MH_OJ_NO_GROUPS
      ng = 0;   // (timing experiment: the duplicated-hash groups are dropped; results are wrong)
#endif
      int gtot = 0;
      if constexpr (WAVES == 4) {
      // collect the groups' entries, THREE groups per round (each round waits for a load from the other sketch's row): lanes 20 t .. 20 t + 8
      // read the query's entries of the round's t-th group, lanes 20 t + 10 .. 20 t + 18 the other sketch's
      for (int g0 = 0; g0 < ng && !bad; g0 += 3) {
        const int t = lane / 20, r = lane - 20 * t;           // lanes 60..63: t = 3, idle
        const int g = g0 + t;
        const bool live = t < 3 && g < ng;
        const int x = r < 10 ? r : r - 10;
        const int lo = live ? gi[g * 6 + 0] : 0, j = live ? gi[g * 6 + 1] : 0;
        const int h = ah[lo];
        const bool a_ok = live && r <= OJ_GLEN && lo + x < nA && ah[lo + x] == h;
        uint2 be = make_uint2(0u, 0u);
        const bool b_in = live && r >= 10 && r <= 10 + OJ_GLEN && j + x < nB;
        if (b_in) be = brow[j + x];
        const bool b_ok = b_in && (int)be.x == h;
        const unsigned long long bala = __ballot(a_ok), balb = __ballot(b_ok);
        const int sh = 20 * (t < 3 ? t : 0);
        const int m = __popcll((bala >> sh) & 0x3FFULL), nn = __popcll((balb >> (sh + 10)) & 0x3FFULL);
        if (__any(live && (m > OJ_GLEN || nn > OJ_GLEN))) { bad = true; bad_groups = true; OJ_STAT(16, 1); break; }
        if (a_ok) gpa[g * OJ_GLEN + x] = APOS ? ap[lo + x] : qrow[2 * (lo + x) + 1];
        if (b_ok) gpb[g * OJ_GLEN + x] = (int)be.y;
        int sz[3];   // entries of the round's groups (wave-uniform)
#pragma unroll
        for (int tt = 0; tt < 3; tt++)
          sz[tt] = g0 + tt < ng ? __popcll((bala >> (20 * tt)) & 0x3FFULL) + __popcll((balb >> (20 * tt + 10)) & 0x3FFULL) : 0;
        // (gi[4]: where the group's records go — behind the joined k-mers, every group as many words as it has entries: oj_pass)
        if (live && r == 0) { gi[g * 6 + 2] = m; gi[g * 6 + 3] = nn; gi[g * 6 + 4] = nj + gtot + (t >= 1 ? sz[0] : 0) + (t >= 2 ? sz[1] : 0); }
        gtot += sz[0] + sz[1] + sz[2];
      }
      } else {
      for (int g = 0; g < ng && !bad; g++) {   // collect the groups' entries: lanes 0..8 the query's, lanes 16..24 the other sketch's
        const int lo = gi[g * 6 + 0], j = gi[g * 6 + 1];
        const int h = ah[lo];
        const int x = lane & 15;
        const bool a_ok = lane <= OJ_GLEN && lo + x < nA && ah[lo + x] == h;
        const bool b_ok = lane >= 16 && lane <= 16 + OJ_GLEN && j + x < nB && (int)brow[j + x].x == h;
        const int m = __popcll(__ballot(a_ok)), nn = __popcll(__ballot(b_ok));
        if (m > OJ_GLEN || nn > OJ_GLEN) { bad = true; bad_groups = true; break; }
        if (a_ok) gpa[g * OJ_GLEN + x] = APOS ? ap[lo + x] : qrow[2 * (lo + x) + 1];
        if (b_ok) gpb[g * OJ_GLEN + x] = (int)brow[j + x].y;
        if (lane == 0) { gi[g * 6 + 2] = m; gi[g * 6 + 3] = nn; gi[g * 6 + 4] = nj + gtot; }
        gtot += m + nn;
      }
      }
      if (!bad && nj + gtot > OJ_JCAP) { bad = true; OJ_STAT(17, 1); }
      if (bad) {
        // (slow_count[OJ_GROUP_BAD]: how many of the pairs handed over were handed over for the group caps — what the host decides a wider pass by)
        if (lane == 0) { const unsigned long long slot = atomicAdd(slow_count, 1ULL); slow[slot] = cd; if (bad_groups) atomicAdd(slow_count + OJ_GROUP_BAD, 1ULL); }
        return;
      }
      mine++;
      // OverlapInfo.EMPTY (score 0, all zero) unless the pair gets through every stage below
      double score = 0.0;
      int valid = 0, a1 = 0, a2 = 0, b1 = 0, b2 = 0;
      do {
#ifdef MH_OJ_JOIN_ONLY
        if (nj >= 0) break;   // (timing experiment: everything after the join skipped; results are wrong)
#endif
        OJ_STAT(6, nj); OJ_STAT(8, ng); OJ_STAT(9, ng > 0 ? 1 : 0); OJ_STAT(10, ng >= 3 ? 1 : 0); OJ_STAT(11, gtot);
        if (ng == 0 && nj < 3) { OJ_STAT(0, 1); break; }   // computeEdges needs three valid records (:126): fewer joined k-mers can only end EMPTY
        int iA[OJ_R], jB[OJ_R];   // the joined k-mers' entry indices move to registers, their LDS words become `sh`
#pragma unroll
        for (int r = 0; r < OJ_R; r++) {
          const int t = r * 64 + lane;
          const uint32_t ij = t < nj ? jij[t] : 0xffffffffu;
          iA[r] = (int)(ij & 0xffffu); jB[r] = (int)(ij >> 16);
          if (t < nj) jp1[t] = APOS ? ap[iA[r]] : qrow[2 * iA[r] + 1];
        }
        oj_lds_sync();
        // ---- recordMatchingKmers twice (:600-606), median shift after each ----
        const int shift_lb = 32 - __builtin_clz((unsigned)((len1 > len2 ? len1 : len2) | 1));   // (2^shift_lb > either length)
        int count = 0;
        const int nx = gtot;   // words behind the joined k-mers that the groups' records may take
        ShiftStats st = oj_shift_stats(false, 0, len1, len2, sp.max_shift);
        uint32_t fl = oj_pass<true, OJ_R>(jp1, jp2, nj, ng, nx, gi, gpa, gpb, len1, len2, st, lane, count);
        if (count <= 0) { OJ_STAT(1, 1); break; }
        st = oj_shift_stats(true, oj_median_shift<OJ_R>(jp1, jp2, sh, fl, nj + nx, count, lane, shift_lb), len1, len2, sp.max_shift);
        fl = oj_pass<false, OJ_R>(jp1, jp2, nj, ng, nx, gi, gpa, gpb, len1, len2, st, lane, count);
        if (count <= 0) { OJ_STAT(2, 1); break; }
        st = oj_shift_stats(true, oj_median_shift<OJ_R>(jp1, jp2, sh, fl, nj + nx, count, lane, shift_lb), len1, len2, sp.max_shift);
        // optimizeShifts (:156-189): neighbouring records of one query position exist only inside a group
        // (lane g walks group g's records and marks the dropped ones, then every lane looks at its own entries)
        int removed = 0;
        if (ng) {
          int rem = 0;
          if (lane < ng) {
            const int start = gi[lane * 6 + 4], k = gi[lane * 6 + 5];
            int red = -1, rp1 = 0, rp2 = 0;
            for (int x = 0; x < k; x++) {
              const int t = start + x;
              const int p1 = jp1[t], p2 = jp2[t];
              if (red >= 0 && rp1 == p1) {
                if (iabs32((rp2 - rp1) - st.med) > iabs32((p2 - p1) - st.med)) { jp1[red] = INT32_MIN; red = t; rp1 = p1; rp2 = p2; }
                else jp1[t] = INT32_MIN;
                rem++;
              } else { red = t; rp1 = p1; rp2 = p2; }
            }
          }
          if (__builtin_amdgcn_ballot_w64(rem != 0)) {
            oj_lds_sync();
#pragma unroll
            for (int r = 0; r < OJ_R; r++) {
              if (r * 64 < nj + nx) {
                const int t = r * 64 + lane;
                const bool gone = ((fl >> r) & 1u) && t >= nj && jp1[t] == INT32_MIN;
                if (gone) fl &= ~(1u << r);
                removed += __popcll(__builtin_amdgcn_ballot_w64(gone));
              }
            }
          }
        }
        OJ_STAT(12, nx); OJ_STAT(13, removed);
        if (removed) {
          count -= removed;
          st = oj_shift_stats(true, oj_median_shift<OJ_R>(jp1, jp2, sh, fl, nj + nx, count, lane, shift_lb), len1, len2, sp.max_shift);
        }
        // computeEdges (:90-137)
        int le1 = INT32_MAX, le2 = INT32_MAX, re1 = INT32_MIN, re2 = INT32_MIN, nvalid = 0;
#pragma unroll
        for (int r = 0; r < OJ_R; r++) {
          if (r * 64 < nj + nx) {
            bool ok = (fl >> r) & 1u;
            if (ok) {
              const int t = r * 64 + lane;
              const int p1 = jp1[t], p2 = jp2[t];
              ok = !(iabs32((p2 - p1) - st.med) > st.absmax);
              if (ok) {
                le1 = p1 < le1 ? p1 : le1; le2 = p2 < le2 ? p2 : le2;
                re1 = p1 > re1 ? p1 : re1; re2 = p2 > re2 ? p2 : re2;
              }
            }
            nvalid += __popcll(__ballot(ok));
          }
        }
        if (nvalid < 3) { OJ_STAT(3, 1); break; }
        le1 = oj_wave_min(le1); le2 = oj_wave_min(le2); re1 = oj_wave_max(re1); re2 = oj_wave_max(re2);
        const double den = (double)(nvalid - 1);
        const int32_t na1 = (int32_t)((uint32_t)nvalid * (uint32_t)le1 - (uint32_t)re1);   // int products wrap like Java's (:131-134)
        const int32_t na2 = (int32_t)((uint32_t)nvalid * (uint32_t)re1 - (uint32_t)le1);
        const int32_t nb1 = (int32_t)((uint32_t)nvalid * (uint32_t)le2 - (uint32_t)re2);
        const int32_t nb2 = (int32_t)((uint32_t)nvalid * (uint32_t)re2 - (uint32_t)le2);
        a1 = (int)java_round((double)na1 / den); if (a1 < 0) a1 = 0;
        a2 = (int)java_round((double)na2 / den); if (a2 > len1) a2 = len1;
        b1 = (int)java_round((double)nb1 / den); if (b1 < 0) b1 = 0;
        b2 = (int)java_round((double)nb2 / den); if (b2 > len2) b2 = len2;
        valid = nvalid;
        if (ph != nullptr) {
          // the early "below the threshold" (poshist_kernel above): J = joined k-mers inside both windows + what the groups can add
          int J = 0;
#pragma unroll
          for (int r = 0; r < OJ_R; r++) {
            if (r * 64 < nj) {
              const int t = r * 64 + lane;
              bool in = false;
              if (t < nj) { const int p1 = jp1[t], p2 = jp2[t]; in = p1 >= a1 && p1 <= a2 && p2 >= b1 && p2 <= b2; }
              J += __popcll(__ballot(in));
            }
          }
          for (int g = 0; g < ng; g++) { const int m = gi[g * 6 + 2], nn = gi[g * 6 + 3]; J += m < nn ? m : nn; }
          const int s1lb = ph_count_lb(qph + (int64_t)cd.q * PH_BINS, len1, a1, a2), s2lb = ph_count_lb(ph + (int64_t)cd.m * PH_BINS, len2, b1, b2);
          const int kklb = s1lb < s2lb ? s1lb : s2lb;
          if (J < pass_min[kklb]) { OJ_STAT(4, 1); break; }     // score stays 0: below any threshold that was asked for
        }
        // ---- computeKBottomSketchJaccard (:304-364): in-window counts, and for every joined k-mer (and every group's first
        // entries) its rank among the in-window entries of either sketch: prefix counts over 64-entry blocks, the lane that
        // holds entry i of the block hands the rank to the lane that holds the joined k-mer ----
        int rA[OJ_R], rB[OJ_R];
#pragma unroll
        for (int r = 0; r < OJ_R; r++) { rA[r] = 0; rB[r] = 0; }
        // lane g < ng speaks for group g
        int giA = 0xffff, gjB = 0xffff, grA = 0, grB = 0, gmin = 0;
        if (lane < ng) {
          giA = gi[lane * 6 + 0]; gjB = gi[lane * 6 + 1];
          const int32_t *pa = gpa + lane * OJ_GLEN, *pb = gpb + lane * OJ_GLEN;
          const int ca = __popc(oj_mask8(pa, gi[lane * 6 + 2], a1, a2 + 1)), cb = __popc(oj_mask8(pb, gi[lane * 6 + 3], b1, b2 + 1));
          gmin = ca < cb ? ca : cb;   // equal hashes pair up one to one in the union walk
        }
        const int jrounds = (nj + 63) >> 6;
        int s1 = 0, s2 = 0;
        // One pass over the positions of either sketch: a block of 64 entries costs its in-window test, the ballot and three
        // v_writelane — lane b of the wave collects block b's mask and the count ahead of it — and the joined k-mers fetch
        // their block's words from that lane afterwards (three shuffles per round of 64 joined k-mers and sketch).  Round 3
        // handed every block's ranks to the joined k-mers as it went: two or three shuffles and ten more instructions per BLOCK.
        int pan[OJ_U], pbn[OJ_U];   // next OJ_U blocks of positions of either sketch, in flight while the current ones are tested
#pragma unroll
        for (int u = 0; u < OJ_U; u++) {
          const int i = u * 64 + lane;
          pan[u] = (!APOS && i < nA) ? qrow[2 * i + 1] : INT32_MIN;
          pbn[u] = (!keepb && i < nB) ? (int)brow[i].y : INT32_MIN;
        }
        for (int cb = 0; cb < nA; cb += 64 * OJ_RCH) {
          uint32_t mlo = 0u, mhi = 0u;
          int mpre = 0;
          const int cend = cb + 64 * OJ_RCH < nA ? cb + 64 * OJ_RCH : nA;
          for (int ib = cb; ib < cend; ib += 64 * OJ_U) {
            int posv[OJ_U];
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              if (APOS) posv[u] = ap[ib + u * 64 + lane];   // (past the sketch: whatever follows in LDS — the last block's ballot is trimmed below)
              else {
                posv[u] = pan[u];
                const int i = ib + (u + OJ_U) * 64 + lane;
                pan[u] = i < nA ? qrow[2 * i + 1] : INT32_MIN;
              }
            }
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int i0 = ib + u * 64;
              if (i0 < nA) {
                // (read from memory, entries past the sketch hold INT32_MIN, and a1 >= 0; a ballot per comparison: the compiler turns a ballot of their conjunction into
                // two more vector instructions)
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(posv[u] >= a1) & __builtin_amdgcn_ballot_w64(posv[u] <= a2);
                const int blk = (i0 - cb) >> 6;
                mlo = (uint32_t)oj_writelane((int)(uint32_t)bal, blk, (int)mlo);
                mhi = (uint32_t)oj_writelane((int)(uint32_t)(bal >> 32), blk, (int)mhi);
                mpre = oj_writelane(s1, blk, mpre);
                s1 += __popcll(bal);
              }
            }
          }
          if (APOS && cend == nA && (nA & 63)) oj_trim_last_block(mlo, mhi, s1, (nA - 1 - cb) >> 6, nA & 63);   // (what the LDS words behind the positions happened to hold)
#pragma unroll
          for (int r = 0; r < OJ_R; r++) {
            if (r < jrounds) {
              const int v = oj_rank_from(mlo, mhi, mpre, iA[r] - cb);
              if (iA[r] >= cb && iA[r] < cend) rA[r] = v;
            }
          }
          if (ng) { const int v = oj_rank_from(mlo, mhi, mpre, giA - cb); if (giA >= cb && giA < cend) grA = v; }
        }
        for (int cb = 0, kit2 = 0; cb < nB; cb += 64 * OJ_RCH) {
          uint32_t mlo = 0u, mhi = 0u;
          int mpre = 0;
          const int cend = cb + 64 * OJ_RCH < nB ? cb + 64 * OJ_RCH : nB;
          for (int jb = cb; jb < cend; jb += 64 * OJ_U, kit2++) {
            int posv[OJ_U];
            if (keepb) { OJ_KEEP_LOAD(kit2, pbk, posv) }
            else {
#pragma unroll
              for (int u = 0; u < OJ_U; u++) {
                posv[u] = pbn[u];
                const int j = jb + (u + OJ_U) * 64 + lane;
                pbn[u] = j < nB ? (int)brow[j].y : INT32_MIN;
              }
            }
#pragma unroll
            for (int u = 0; u < OJ_U; u++) {
              const int j0 = jb + u * 64;
              if (j0 < nB) {
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(posv[u] >= b1) & __builtin_amdgcn_ballot_w64(posv[u] <= b2);
                const int blk = (j0 - cb) >> 6;
                mlo = (uint32_t)oj_writelane((int)(uint32_t)bal, blk, (int)mlo);
                mhi = (uint32_t)oj_writelane((int)(uint32_t)(bal >> 32), blk, (int)mhi);
                mpre = oj_writelane(s2, blk, mpre);
                s2 += __popcll(bal);
              }
            }
          }
          if (keepb && cend == nB && (nB & 63)) oj_trim_last_block(mlo, mhi, s2, (nB - 1 - cb) >> 6, nB & 63);   // (the kept registers of lanes past the sketch's end)
#pragma unroll
          for (int r = 0; r < OJ_R; r++) {
            if (r < jrounds) {
              const int v = oj_rank_from(mlo, mhi, mpre, jB[r] - cb);
              if (jB[r] >= cb && jB[r] < cend) rB[r] = v;
            }
          }
          if (ng) { const int v = oj_rank_from(mlo, mhi, mpre, gjB - cb); if (gjB >= cb && gjB < cend) grB = v; }
        }
        const int kk = s1 < s2 ? s1 : s2;
        // a joined k-mer counts if its index in the merged union (in-window entries of both, joined ones once) is below k:
        // index = rank in the query + rank in the other sketch - joined in-window k-mers ahead of it
        int inter = 0, before = 0;
        bool both[OJ_R];
#pragma unroll
        for (int r = 0; r < OJ_R; r++) {
          both[r] = false;
          if (r < jrounds) {
            const int t = r * 64 + lane;
            if (t < nj) { const int p1 = jp1[t], p2 = jp2[t]; both[r] = p1 >= a1 && p1 <= a2 && p2 >= b1 && p2 <= b2; }
            const unsigned long long bal = __ballot(both[r]);
            int m = before + oj_mbcnt(bal);
            for (int g = 0; g < ng; g++)   // pairs of the groups ahead of it
              m += (__builtin_amdgcn_readlane(giA, g) < iA[r]) ? __builtin_amdgcn_readlane(gmin, g) : 0;
            inter += __popcll(__ballot(both[r] && rA[r] + rB[r] - m < kk));
            before += __popcll(bal);
          }
        }
        int gacc = 0;   // pairs of the groups ahead of group g
        for (int g = 0; g < ng; g++) {
          const int glo = __builtin_amdgcn_readlane(giA, g), gm = __builtin_amdgcn_readlane(gmin, g);
          int ahead = gacc;
#pragma unroll
          for (int r = 0; r < OJ_R; r++)
            if (r < jrounds) ahead += __popcll(__ballot(both[r] && iA[r] < glo));
          const int base = __builtin_amdgcn_readlane(grA, g) + __builtin_amdgcn_readlane(grB, g) - ahead;
          int take = kk - base;                    // the group's pairs sit at union indices base, base+1, ...
          take = take < 0 ? 0 : (take > gm ? gm : take);
          inter += take;
          gacc += gm;
        }
        score = score_table[score_index(inter, kk)];
        OJ_STAT(score >= sp.threshold ? 5 : 4, 1);
        OJ_STAT(7, before);
      } while (0);
      if (score >= sp.threshold && lane == 0) {                                                  // MinHashSearch.java:229
        const unsigned long long slot = atomicAdd(rec_count, 1ULL);
        if (slot < rec_cap) {
          DevRecord d;
          d.q = cd.q; d.m = cd.m; d.score = score; d.raw = valid; d.a1 = a1; d.a2 = a2; d.b1 = b1; d.b2 = b2; d.pad = 0;
          recs[slot] = d;
        }
      }
  };
  // chunks of consecutive candidates (one query's candidates are contiguous) are pulled from a counter: a static split makes the
  // launch's duration depend on every workgroup of the grid being resident at once (one more per CU than fit = a second round)
  const unsigned long long step = SHARED ? (unsigned long long)chunk * WAVES : (unsigned long long)chunk;
  for (;;) {
    unsigned long long c0 = 0;
    if (SHARED) {
      __syncthreads();
      if (threadIdx.x == 0) {
        const unsigned long long v = atomicAdd(work, step);
        svar[2] = (int32_t)(uint32_t)v; svar[3] = (int32_t)(uint32_t)(v >> 32);
      }
      __syncthreads();
      c0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane(svar[3]) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane(svar[2]);
    } else {
      if (lane == 0) c0 = atomicAdd(work, step);
      c0 = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(c0 >> 32)) << 32) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)c0);
    }
    if (c0 >= n) break;
    const unsigned long long c1 = c0 + step < n ? c0 + step : n;
    unsigned long long c = c0, rend = c0;
    while (c < c1) {
      Candidate cd = cand[c];   // wave-uniform values are pinned to SGPRs: loop bounds and branches below become scalar
      cd.q = __builtin_amdgcn_readfirstlane(cd.q); cd.m = __builtin_amdgcn_readfirstlane(cd.m);
      if (SHARED || cd.q != curq) {   // candidates of one query are contiguous: its hashes are staged once per run
        curq = cd.q;
        const int32_t* qm = qmeta + (int64_t)cd.q * META_W;
        nA = __builtin_amdgcn_readfirstlane(qm[0]); len1 = __builtin_amdgcn_readfirstlane(qm[1]);
        qrow = qordered + (int64_t)cd.q * qord_stride;
        if (SHARED) {
          __syncthreads();               // the previous run's waves are done with the hashes and the table
          if (threadIdx.x == 0) svar[1] = 0;
          rend = c1;                     // the run ends at the chunk's first candidate of another query (every wave finds it for itself)
          for (unsigned long long t0 = c + 1; t0 < c1; t0 += 64) {
            const unsigned long long bal = __ballot(t0 + lane < c1 && cand[t0 + lane].q != curq);
            if (bal) { rend = t0 + (unsigned long long)__builtin_ctzll(bal); break; }
          }
        } else __builtin_amdgcn_wave_barrier();
        if (APOS) for (int i = tid; i < nA; i += NT) ap[i] = qrow[2 * i + 1];
        if (FILTER) {
          for (int i = tid; i < tabw; i += NT) bm[i] = 0u;
          __syncthreads();
        }
        if (!TABLE) {
          for (int i = tid; i < nA; i += NT) {
            const int h = qrow[2 * i];
            ah[i] = h;
            if (FILTER) { const uint32_t fb = oj_filter_bit((uint32_t)h, (uint32_t)ts); atomicOr(&bm[fb >> 5], 1u << (fb & 31u)); }
          }
        } else if (nA > 0) {
          bk = oj_buckets(__builtin_amdgcn_readfirstlane(qrow[0]), __builtin_amdgcn_readfirstlane(qrow[2 * (nA - 1)]), ts);
          for (int i = tid; i < nA; i += NT) {   // entry i starts every bucket after its predecessor's up to its own
            const int h = qrow[2 * i];
            ah[i] = h;
            const int b1 = oj_bucket_of(bk, h), b0 = i ? oj_bucket_of(bk, qrow[2 * (i - 1)]) + 1 : 0;
            for (int b = b0; b <= b1; b++) st[b] = (uint16_t)i;
            if (i == nA - 1) for (int b = b1 + 1; b <= ts; b++) st[b] = (uint16_t)nA;
          }
        }
        if (SHARED) __syncthreads(); else oj_lds_sync();
      }
      if (SHARED) {                      // this wave's next candidate of the run
        int ci = 0;
        if (lane == 0) ci = atomicAdd(&svar[1], 1);
        ci = __builtin_amdgcn_readfirstlane(ci);
        // (the loop below keeps `c` at the run's start and walks `cw`; it leaves with c = the run's end)
        for (unsigned long long cw = c + (unsigned long long)(uint32_t)ci; cw < rend;) {
          Candidate cx = cand[cw];
          cx.q = __builtin_amdgcn_readfirstlane(cx.q); cx.m = __builtin_amdgcn_readfirstlane(cx.m);
          one_candidate(cx);
          int cn = 0;
          if (lane == 0) cn = atomicAdd(&svar[1], 1);
          cw = c + (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane(cn);
        }
        c = rend;
      } else {
        one_candidate(cd);
        c++;
      }
    }
  }
  if (mine && lane == 0) atomicAdd(compared, mine);
}

// The three shapes of the join kernel.  Its time is inversely proportional to the waves a CU holds (padding the LDS of the ALONE
// shape by 4 / 12 KB per wave: 4.97 -> 6.66 / 12.5 ms at C2, i.e. 18 -> 12 / 7 waves per CU), and what bounds those is LDS:
//   ALONE  every wave stages its own query (6 KB of hashes at S = 1536) and searches them by bisection: 8.7 KB per wave, 18 waves per CU.
//          For a candidate or fewer per query (a rank of a multi-GPU job: every query against an eighth of the reads).
//   PAIR   two waves share one staged query and take its candidates in turn: 5.6 KB per wave, 28 waves per CU (the VGPR limit) —
//          but a wave now waits for its partner at every run's end, which takes most of that back (C2, 4.5 candidates per query:
//          4.83 ms against 4.94 alone).  For a few candidates per query.
//   TEAM   four waves share the query and a bucket table over its hashes (two LDS round trips per lookup instead of eleven).
//          For tens of candidates per query (repeat-rich reads).
#ifndef MH_OJ_FILTER
#define MH_OJ_FILTER 1   // the shared shapes filter the other sketch's entries through a bitmap of the query's hashes (0: round 3's lookups of every entry)
#endif
enum { OJ_ALONE = 0, OJ_PAIR = 1, OJ_TEAM = 2 };
constexpr int OJ_SHAPE_WAVES[3] = {2, 2, OJ_WAVES};
int overlap_join_waves_per_block(int shape) { return OJ_SHAPE_WAVES[shape]; }
// LDS bytes of one workgroup: the hashes (and the table) once or per wave, the join scratch per wave
size_t overlap_join_lds_bytes(int S, int shape, int level) {
  const size_t sp = (size_t)((S + 3) & ~3), w = (size_t)OJ_SHAPE_WAVES[shape], extra = (size_t)oj_lds_extra(OJ_LEVEL_CAP[level]);
  if (shape == OJ_ALONE) return w * (sp + extra) * 4;
  const size_t aid = MH_OJ_FILTER ? (size_t)overlap_join_filter_bits(S, (int)w) / 32 : (shape == OJ_TEAM ? (size_t)((overlap_join_table_slots(S) / 2 + 4) & ~3) : 0);
  return (sp + (MH_OJ_KEEP ? sp : 0) + aid + 4 + w * extra) * 4;
}
// The instantiations.  The kernel keeps a pair's joined k-mers in JCAP words of LDS and JCAP / 64 rounds of one entry per lane; a pair
// with more of them is handed on, in the end to the per-lane kernel, which is exact and about two hundred times slower per pair.
// 128 is plenty for the reads MHAP was built for — at 15 % error two overlapping 10-kb reads join about 40 of their 1 536 bottom
// 12-mers — and not for better reads: a 12-mer survives in both reads with probability (1 - e)^24, so at 8 % error the average true
// overlap joins about a hundred, at 4 % about three hundred (round 5, 20 000 reads x 10 kb: 57 % / 83 % of the pairs handed over, second
// stage 54 / 149 ms where the join kernel alone would take 3).  Widening the kernel for everybody costs LDS and registers on the path
// BASELINE measures (four rounds per lane: 110 VGPRs in the PAIR shape; eight: 128 + scratch), so the wider capacities are instantiations
// of their own, and the search runs them as further passes over the pairs the pass before hands over: 512, then 1 536 (the whole of a
// default ordered sketch — eight times the first pass's cost per pair, a tenth of the per-lane kernel's: the pass for reads of a few
// per cent error and better).  Only what the last of them hands over in turn (the group caps) goes to the per-lane kernel.
// Level 0 has the three shapes; the wider passes run every wave alone.
// (the shape a level runs: the callers below size the block and its LDS by it, so it holds in a build without asserts too)
static int oj_level_shape(int level, int shape) {
  assert(level >= 0 && level < OJ_LEVELS && (level == 0 || shape == OJ_ALONE));
  return level > 0 ? OJ_ALONE : shape;
}
template <class F> static auto oj_dispatch(int level, int shape, F f) {
  if (level == 1) return f(overlap_join_kernel<OJ_LEVEL_CAP[1], false, OJ_SHAPE_WAVES[OJ_ALONE], false, false>);
  if (level == 2) return f(overlap_join_kernel<OJ_LEVEL_CAP[2], false, OJ_SHAPE_WAVES[OJ_ALONE], false, false>);
  if (shape == OJ_TEAM) return f(overlap_join_kernel<OJ_LEVEL_CAP[0], true, OJ_SHAPE_WAVES[OJ_TEAM], !MH_OJ_FILTER, MH_OJ_FILTER != 0>);
  if (shape == OJ_PAIR) return f(overlap_join_kernel<OJ_LEVEL_CAP[0], true, OJ_SHAPE_WAVES[OJ_PAIR], false, MH_OJ_FILTER != 0>);
  return f(overlap_join_kernel<OJ_LEVEL_CAP[0], false, OJ_SHAPE_WAVES[OJ_ALONE], false, false>);
}
// workgroups of the join kernel one CU holds at this sketch size
int overlap_join_blocks_per_cu(int S, int shape, int level) {
  shape = oj_level_shape(level, shape);
  int n = 0;
  const hipError_t e = oj_dispatch(level, shape, [&](auto kern) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 64 * OJ_SHAPE_WAVES[shape], overlap_join_lds_bytes(S, shape, level)); });
  if (e != hipSuccess || n < 1) n = 1;
  return n;
}

void launch_overlap_join(hipStream_t st, int level, int shape, int nblocks, int chunk, const Candidate* cand, const unsigned long long* cand_count,
                         unsigned long long cand_cap, const int32_t* ordered, int64_t ord_stride, const int32_t* meta, const int32_t* qordered,
                         int64_t qord_stride, const int32_t* qmeta, const SearchParams& sp, const double* score_table, DevRecord* recs,
                         unsigned long long* rec_count, unsigned long long rec_cap, unsigned long long* compared, Candidate* slow,
                         unsigned long long* slow_count, unsigned long long* work, const uint16_t* ph, const uint16_t* qph, const int32_t* pass_min) {
  shape = oj_level_shape(level, shape);
  const int ts = (MH_OJ_FILTER && shape != OJ_ALONE) ? overlap_join_filter_bits(sp.S, OJ_SHAPE_WAVES[shape]) : overlap_join_table_slots(sp.S);
  oj_dispatch(level, shape, [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * OJ_SHAPE_WAVES[shape]), overlap_join_lds_bytes(sp.S, shape, level), st, cand, cand_count, cand_cap, ordered,
                       ord_stride, meta, qordered, qord_stride, qmeta, sp, score_table, recs, rec_count, rec_cap, compared, slow, slow_count, chunk, work, ts,
                       ph, qph, pass_min);
    return 0;
  });
}

void oj_stats_dump() {
#ifdef MH_OJ_STATS
  unsigned long long h[20];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_oj_stats), sizeof h) != hipSuccess) return;
  const double np = (double)(h[0] + h[1] + h[2] + h[3] + h[4] + h[5] + 1);
  fprintf(stderr, "[oj stats] pairs: nj<3 %llu, no record in pass 1 %llu, in pass 2 %llu, <3 valid %llu, below threshold %llu, accepted %llu; mean nj %.2f, mean in-window joined of scored %.2f\n",
          h[0], h[1], h[2], h[3], h[4], h[5], (double)h[6] / np, (double)h[7] / (double)(h[4] + h[5] + 1));
  fprintf(stderr, "[oj stats] groups: per pair %.2f, pairs with groups %llu, with >= 3 %llu, entries in groups per pair %.2f, words reserved for group records per pair %.2f, removed by optimizeShifts per pair %.2f\n",
          (double)h[8] / np, h[9], h[10], (double)h[11] / np, (double)h[12] / np, (double)h[13] / np);
  fprintf(stderr, "[oj stats] handed to the per-lane kernel: more than %d joined k-mers %llu, more than %d groups %llu, a group of more than %d entries %llu, joined k-mers + group entries > %d: %llu\n",
          OJ_LEVEL_CAP[0], h[14], OJ_GCAP, h[15], OJ_GLEN, h[16], OJ_LEVEL_CAP[0], h[17]);
  memset(h, 0, sizeof h);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_oj_stats), h, sizeof h);
#endif
}

void launch_overlap(hipStream_t st, int nblocks, const Candidate* cand, const unsigned long long* cand_count, unsigned long long cand_cap,
                    const int32_t* ordered, int64_t ord_stride, const int32_t* meta, const int32_t* qordered, int64_t qord_stride,
                    const int32_t* qmeta, const SearchParams& sp, const double* score_table, int32_t* scratch, int64_t scratch_per_lane,
                    DevRecord* recs, unsigned long long* rec_count, unsigned long long rec_cap, unsigned long long* compared, int spread) {
  hipLaunchKernelGGL(overlap_kernel, dim3(nblocks), dim3(OVL_THREADS), 0, st, cand, cand_count, cand_cap, ordered, ord_stride, meta,
                     qordered, qord_stride, qmeta, sp, score_table, scratch, scratch_per_lane, recs, rec_count, rec_cap, compared, spread);
}

}  // namespace mhap
