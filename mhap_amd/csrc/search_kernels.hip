// search_kernels.hip — gfx950 kernels for candidate generation (hot loop E of SURVEY §3.1; the second stage is join_kernels.hip).
//
//   candidate_kernel : tiled all-pairs MinHash slot-equality count.  The reference walks an inverted
//                      index (J/impl/MinHashSearch.java:100-147,161-181); the hit count of a pair is by
//                      construction the number of slots whose int sketches are equal
//                      (J/sketch/MinHashSketch.java:237-252), so a brute-force count with the same
//                      `>= numMinMatches` cut and the same id/length filters (:200-225) yields the identical
//                      candidate set.  Integer VALU work (v_cmp_eq + v_addc per slot pair), tiles staged
//                      through LDS, 8x8 register micro-tile per lane, triangular tile skipping in self mode.
//   index_*          : the inverted index over the MinHash slots, its line table and the three query tiers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "kernels.hpp"

namespace mhap {

// count += (a == b): exactly two VALU issues per slot pair (v_cmp_eq -> vcc, v_addc consumes vcc).  Left to the
// compiler the compare lands in arbitrary SGPR pairs (v_cmp_e64 + v_cndmask + add) and spills SGPRs through
// v_writelane/v_readlane inside the hot loop.
#define CMP_ACC4(c, q, m)                                                                                   \
  asm("v_cmp_eq_u32 vcc, %1, %5\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc\n\t"                                    \
      "v_cmp_eq_u32 vcc, %2, %6\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc\n\t"                                    \
      "v_cmp_eq_u32 vcc, %3, %7\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc\n\t"                                    \
      "v_cmp_eq_u32 vcc, %4, %8\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc"                                          \
      : "+v"(c)                                                                                             \
      : "v"((q).x), "v"((q).y), "v"((q).z), "v"((q).w), "v"((m).x), "v"((m).y), "v"((m).z), "v"((m).w)      \
      : "vcc")

constexpr int CAND_LD = CAND_KS + 4;  // padded LDS row (ints): 36 -> conflict-free ds_read_b128 across 16 rows

__device__ inline bool pair_passes(const SearchParams& sp, int64_t qid, int64_t mid, int qlen, int mlen) {
  if (sp.to_self && mid == qid) return false;                                               // MinHashSearch.java:200-201
  if (mlen < sp.min_store_length && qlen < sp.min_store_length) return false;               // :211-212
  if (sp.to_self && mid > qid && mlen >= sp.min_store_length && qlen >= sp.min_store_length) return false;  // :215-219
  if (sp.to_self && mlen < sp.min_store_length && qlen >= sp.min_store_length) return false;                // :222-225
  return true;
}

__global__ __launch_bounds__(256, 2) void candidate_kernel(const int32_t* __restrict__ minhash, int64_t row_stride,
                                                        const int32_t* __restrict__ qminhash, int64_t qrow_stride,
                                                        const int32_t* __restrict__ qlist, int nq, int ne,
                                                        const int64_t* __restrict__ ids, const int64_t* __restrict__ qids,
                                                        const int32_t* __restrict__ meta, const int32_t* __restrict__ qmeta,
                                                        SearchParams sp, int triangular, const long long* __restrict__ rowstart, int ntq,
                                                        long long nblocks_valid, int ntu,
                                                        Candidate* __restrict__ cand, unsigned long long* __restrict__ cand_count,
                                                        unsigned long long cand_cap) {
  __shared__ __attribute__((aligned(16))) int32_t qs[CAND_TQ * CAND_LD];
  __shared__ __attribute__((aligned(16))) int32_t ms[CAND_TM * CAND_LD];
  __shared__ int32_t qent[CAND_TQ];
  // XCD-aware remap: block b runs on XCD b%8; give every XCD a contiguous range of tiles so that
  // consecutive tiles (same query tile, neighbouring index tiles) share that XCD's L2.
  const long long nb8 = (long long)gridDim.x;
  const long long b = (long long)blockIdx.x;
  const long long bp = (b % 8) * (nb8 / 8) + b / 8;
  if (bp >= nblocks_valid) return;
  int t, u;
  if (triangular) {
    // rowstart[t] = first linear tile id of query-tile row t; row t only owns the index tiles that can
    // hold an entry with a smaller read id than the row's largest query (MinHashSearch.java:215-219).
    int lo = 0, hi = ntq;  // find t with rowstart[t] <= bp < rowstart[t+1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (rowstart[mid] <= bp) lo = mid; else hi = mid; }
    t = lo;
    u = (int)(bp - rowstart[t]);
  } else {
    t = (int)(bp / ntu);
    u = (int)(bp % ntu);
  }
  const int q0 = t * CAND_TQ, m0 = u * CAND_TM;
  const int tid = threadIdx.x;
  if (tid < CAND_TQ) qent[tid] = (q0 + tid < nq) ? qlist[q0 + tid] : -1;
  __syncthreads();
  const int tq = tid >> 4, tm = tid & 15;
  int cnt[8][8];
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 8; j++) cnt[i][j] = 0;

  const int H = sp.H;
  const bool vec_ok = ((row_stride & 3) == 0) && ((qrow_stride & 3) == 0);
  // Register-staged software pipeline: the global loads of chunk c+1 are issued before the compare phase of
  // chunk c and land in LDS after it, so HBM/L2 latency hides under ~8k VALU cycles of compares.
  int4 pq[4], pm[4];
  auto fetch = [&](int s0) {
    const bool full = vec_ok && (s0 + CAND_KS <= H);
#pragma unroll
    for (int rep = 0; rep < 4; rep++) {
      const int idx = tid + rep * 256;
      const int row = idx >> 3, c4 = (idx & 7) * 4;
      int4 qv = make_int4(0, 0, 0, 0), mv = make_int4(1, 1, 1, 1);   // never-equal sentinels for absent rows/slots
      const int qe = qent[row];
      const int me = m0 + row;
      if (full) {
        if (qe >= 0) qv = *(const int4*)(qminhash + (int64_t)qe * qrow_stride + s0 + c4);
        if (me < ne) mv = *(const int4*)(minhash + (int64_t)me * row_stride + s0 + c4);
      } else {
        int qa[4] = {0, 0, 0, 0}, ma[4] = {1, 1, 1, 1};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const int s = s0 + c4 + e;
          if (s < H) {
            if (qe >= 0) qa[e] = qminhash[(int64_t)qe * qrow_stride + s];
            if (me < ne) ma[e] = minhash[(int64_t)me * row_stride + s];
          }
        }
        qv = make_int4(qa[0], qa[1], qa[2], qa[3]);
        mv = make_int4(ma[0], ma[1], ma[2], ma[3]);
      }
      pq[rep] = qv; pm[rep] = mv;
    }
  };
  fetch(0);
  for (int s0 = 0; s0 < H; s0 += CAND_KS) {
#pragma unroll
    for (int rep = 0; rep < 4; rep++) {
      const int idx = tid + rep * 256;
      const int row = idx >> 3, c4 = (idx & 7) * 4;
      *(int4*)&qs[row * CAND_LD + c4] = pq[rep];
      *(int4*)&ms[row * CAND_LD + c4] = pm[rep];
    }
    __syncthreads();
    if (s0 + CAND_KS < H) fetch(s0 + CAND_KS);
#pragma unroll 1
    for (int s4 = 0; s4 < CAND_KS; s4 += 4) {
      int4 qv[8], mv[8];
#pragma unroll
      for (int i = 0; i < 8; i++) qv[i] = *(const int4*)&qs[(i * 16 + tq) * CAND_LD + s4];
#pragma unroll
      for (int j = 0; j < 8; j++) mv[j] = *(const int4*)&ms[(j * 16 + tm) * CAND_LD + s4];
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          CMP_ACC4(cnt[i][j], qv[i], mv[j]);
        }
    }
    __syncthreads();
  }
  // emit: flag the (rare) pairs that reach --num-min-matches, then handle them one at a time
  unsigned long long hitmask = 0;
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int j = 0; j < 8; j++)
      if (cnt[i][j] >= sp.num_min_matches) hitmask |= 1ULL << (i * 8 + j);                   // MinHashSearch.java:204
  while (hitmask) {
    const int bit = __ffsll((long long)hitmask) - 1;
    hitmask &= hitmask - 1;
    const int i = bit >> 3, j = bit & 7;
    const int qe = qent[i * 16 + tq];
    const int me = m0 + j * 16 + tm;
    if (qe < 0 || me >= ne) continue;
    const int32_t* qm = qmeta + (int64_t)qe * META_W;
    const int32_t* mm = meta + (int64_t)me * META_W;
    if (qm[3] != 0 || mm[3] != 0) continue;   // placeholder entries (skipped strands) are not in the index
    if (!pair_passes(sp, qids[qe], ids[me], qm[2], mm[2])) continue;
    const unsigned long long slot = atomicAdd(cand_count, 1ULL);
    if (slot < cand_cap) { cand[slot].q = qe; cand[slot].m = me; }
  }
}

void launch_candidates(hipStream_t st, const int32_t* minhash, int64_t row_stride, const int32_t* qminhash, int64_t qrow_stride,
                       const int32_t* qlist, int nq, int ne, const int64_t* ids, const int64_t* qids, const int32_t* meta,
                       const int32_t* qmeta, const SearchParams& sp, const long long* rowstart, long long nblocks_tri,
                       Candidate* cand, unsigned long long* cand_count, unsigned long long cand_cap) {
  if (nq <= 0 || ne <= 0) return;
  const int ntq = (nq + CAND_TQ - 1) / CAND_TQ;
  const int ntu = (ne + CAND_TM - 1) / CAND_TM;
  const int triangular = rowstart != nullptr;
  const long long nblocks = triangular ? nblocks_tri : (long long)ntq * ntu;
  if (nblocks <= 0) return;
  const long long nb8 = ((nblocks + 7) / 8) * 8;
  hipLaunchKernelGGL(candidate_kernel, dim3((unsigned)nb8), dim3(256), 0, st, minhash, row_stride, qminhash, qrow_stride, qlist, nq, ne,
                     ids, qids, meta, qmeta, sp, triangular, rowstart, ntq, nblocks, ntu, cand, cand_count, cand_cap);
}

// =============================================================================================
// Inverted index on the GPU (the reference's structure, J/impl/MinHashSearch.java:100-147,161-181: per MinHash slot a map
// value -> list of stored sequences).  Here: per slot, the postings (mix(value), entry) of all stored entries GROUPED BY BUCKET,
// bucket = top bits of mix(value) (fmix32, a bijection: equal values <=> equal mixes, and the mixes are uniform whatever the
// distribution of the minima), plus a table of bucket ends.  One bucket per stored entry (rounded up to a power of two), so a
// bucket holds 0.5-1 postings on average and a lookup is two dependent loads: the bucket's bounds, then its postings — the ones
// whose mix equals the query's are the hits.  A query counts hits per stored entry in an LDS count table; the hit count of a pair
// equals the number of slots with equal values, so the candidate set is identical to the brute-force count.
//
// Built by a two-level counting sort whose only atomics are in LDS (a global atomic costs this chip ~50 ps of its memory side:
// 102 M of them at C2 are 4-5 ms per pass, measured with the one-level counting sort that was tried first, 11.2 ms in all):
//   1. index_tile_kernel<0>  per tile of IB_TE entries x IB_S slots, LDS histogram over the 128 coarse bins (top 7 bits of the mix)
//   2. index_offsets_kernel  per slot: exclusive scan over (bin, tile) -> where each tile's share of each bin starts
//   3. index_tile_kernel<1>  same tiles: postings to their bin (LDS cursors), 256 contiguous bytes per (tile, slot, bin) on average
//   4. index_bins_kernel     per (slot, bin): the bin's ~ne/128 postings grouped by bucket through an LDS histogram, ends written
// A value shared by many entries (a repeat) simply makes its bucket long: the postings are contiguous and a workgroup streams them
// with coalesced loads.  Rounds 1-2 kept an open-addressing table of (value, entry) words per slot with runs of equal values, an
// overflow pool and a per-value overflow table: 4.3 GB at C2 and 34 GB at C4 against 1.4 / 12.5 GB here (+ the sort's scratch),
// every insert a CAS chain into a random line, and — what cost the C5 slice 40 of its 54 ms of index_query — a lookup had to walk
// to the end of its CLUSTER, which the 16-entry runs of popular values made hundreds of words long for some lane of nearly every
// workgroup (670 loads per wave in the second tier: r03 PMC pass).
// =============================================================================================
__device__ __forceinline__ uint32_t inv_mix(uint32_t v) { return fmix32(v); }
// "table elements processed" (MinHashSearch.java:173) of a query, added to the launch's total.  Round 6: every LANE used to add its own count
// to ONE word — a wave instruction of up to 64 atomic operations on one address, one per query, all through one L2 channel: the timing build
// without it ran the first query tier of an 8-GPU rank in 1.03 ms instead of 1.98 (profiles/r06_iq_timing_builds.txt).  Now a wave adds its
// sum once, to one of IQ_ELEM_SPREAD words picked by the workgroup; index_elements_sum_kernel folds them into the counter the host reads.
constexpr int IQ_ELEM_SPREAD = 256;
__device__ __forceinline__ void iq_add_elements(unsigned long long* __restrict__ spread, unsigned long long mine) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(spread + (blockIdx.x & (IQ_ELEM_SPREAD - 1)), mine);
}
__global__ __launch_bounds__(IQ_ELEM_SPREAD) void index_elements_sum_kernel(unsigned long long* __restrict__ spread, unsigned long long* __restrict__ total) {
  unsigned long long v = spread[threadIdx.x];
  spread[threadIdx.x] = 0ULL;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}
int index_elements_spread_words() { return IQ_ELEM_SPREAD; }
// (Round 4 tried an occupancy bitmap in front of the lookups — 4 bits per bucket, a clear bit ends a lookup after one load instead of two
//  dependent ones; 82 % of the lookups of a C2 query find nothing.  It made the first tier SLOWER: 3.3 -> 4.8 ms at C2, 70.8 -> 78.4 at
//  C4, 2.50 -> 2.42 for one rank of eight.  A wave is one query with eight slots per lane; nearly every wave holds some lane whose bit
//  is set, and for those the chain is three dependent loads instead of two — the wave's time is its slowest lane's.  Removed.)

#ifndef MH_IB_BINS_LOG
#define MH_IB_BINS_LOG 7
#endif
constexpr int IB_BINS_LOG = MH_IB_BINS_LOG, IB_BINS = 1 << IB_BINS_LOG;   // coarse bins per slot: a tile's share of a bin is IB_TE / IB_BINS postings = 256
                                                                          // contiguous bytes (512 bins, 64-byte shares: the scatter took 2.6 ms at C2, its
                                                                          // half-written lines leaving the L2 before their neighbours arrived)
constexpr int IB_S = 8;                                      // slots of one workgroup (32 bytes of every MinHash row it reads)
constexpr int IB_TE = 4096;                                  // entries of one tile (index_tile_entries: 1024 for a small index)
constexpr int IB_THREADS = 256;
// Steps 1 and 3.  Slot-group-major grid: consecutive workgroups are the tiles of one group of IB_S slots.
template <bool SCATTER>
__global__ __launch_bounds__(IB_THREADS) void index_tile_kernel(const int32_t* __restrict__ minhash, int64_t row_stride, const int32_t* __restrict__ meta,
                                                                int ne, int H, int tiles, int te, InvIndex ix) {
  __shared__ uint32_t bins[IB_S][IB_BINS];
  const int g = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int sl = (int)(threadIdx.x % IB_S), s = g * IB_S + sl;
  for (int i = threadIdx.x; i < IB_S * IB_BINS; i += IB_THREADS) {
    const int ss = g * IB_S + i / IB_BINS;
    (&bins[0][0])[i] = (SCATTER && ss < H) ? ix.tile_counts[((size_t)ss * tiles + tile) * IB_BINS + (i % IB_BINS)] : 0u;
  }
  __syncthreads();
  if (s < H) {
    const int e1 = min(ne, (tile + 1) * te);
    for (int e = tile * te + (int)(threadIdx.x / IB_S); e < e1; e += IB_THREADS / IB_S) {
      if (meta[(int64_t)e * META_W + 3] != 0) continue;                  // skipped strands are not stored (addSequence never sees them)
      const uint32_t hv = inv_mix((uint32_t)minhash[(int64_t)e * row_stride + s]);
      const uint32_t at = atomicAdd(&bins[sl][hv >> (32 - IB_BINS_LOG)], 1u);
      if (SCATTER) ix.staged[(size_t)s * ix.slot_stride + at] = make_uint2(hv, (uint32_t)e);
    }
  }
  if (!SCATTER) {
    __syncthreads();
    for (int i = threadIdx.x; i < IB_S * IB_BINS; i += IB_THREADS) {
      const int ss = g * IB_S + i / IB_BINS;
      if (ss < H) ix.tile_counts[((size_t)ss * tiles + tile) * IB_BINS + (i % IB_BINS)] = (&bins[0][0])[i];
    }
  }
}

// Step 2, one workgroup per slot, one thread per bin: tile_counts[s][t][bin] becomes the first posting (within the slot) of tile t's
// share of the bin; bin_start[s][bin] (IB_BINS + 1 words) the bins' bounds.
__global__ __launch_bounds__(IB_BINS) void index_offsets_kernel(InvIndex ix, int tiles) {
  __shared__ uint32_t wsum[IB_BINS / 64];
  const int s = blockIdx.x, bin = threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* c = ix.tile_counts + (size_t)s * tiles * IB_BINS + bin;
  uint32_t total = 0;
  for (int t = 0; t < tiles; t++) total += c[(size_t)t * IB_BINS];
  uint32_t incl = total;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(incl, off); if (lane >= off) incl += v; }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  uint32_t run = incl - total;
  for (int w = 0; w < wv; w++) run += wsum[w];
  uint32_t* bs = ix.bin_start + (size_t)s * (IB_BINS + 1);
  bs[bin] = run;
  if (bin == IB_BINS - 1) bs[IB_BINS] = run + total;
  for (int t = 0; t < tiles; t++) { const uint32_t v = c[(size_t)t * IB_BINS]; c[(size_t)t * IB_BINS] = run; run += v; }
}

// Step 6 (round 6): the LINE table.  A lookup through ends / items is two dependent random accesses — the bucket's bounds, then its
// postings — and in an N-GPU job every rank looks ALL N n queries up against its shard: the one term of a rank's step that does not
// shrink with N.  Line l of slot s packs the postings of the buckets [l << lb, (l + 1) << lb) — 3.5 to 7 of them on average — into ONE
// 64-byte line: the first-tier query reads that line and nothing else.  A packed posting is exact: the line index is the mix's top
// nl_log bits, the posting keeps the other 32 - nl_log (the "tag") above the entry's ebits bits — at most 36 bits (index_line_params):
//   words 0..13   the low 32 bits of 14 postings
//   word 14       the top 4 bits of postings 0..7, word 15 bits 0..23 those of postings 8..13
//   word 15 >> 24 the header: n = postings of the line's buckets (0..28), or 0xFF "look the bucket up in ends / items" (a long bucket: a
//                 repeat — or, one line in ten thousand, more than a pair of lines holds)
// n > 14: the postings beyond the 14th sit in the PARTNER line (l ^ 1: the other half of the same 128-byte block), behind the partner's
// own (header of the partner = its own count < 14), as long as the pair's postings fit the pair's 28 places.
constexpr int IL_CAP = 14;
constexpr uint32_t IL_FALLBACK = 0xFFu;
// one line: its own postings P[me_lo .. me_lo + n_me), and — behind them — what its partner line (n_pt postings from pt_lo) cannot hold
__device__ __forceinline__ void il_build_line(const uint2* __restrict__ P, uint32_t me_lo, uint32_t n_me, uint32_t pt_lo, uint32_t n_pt, uint32_t tmask, uint32_t eb,
                                              uint4* __restrict__ out) {
  const bool fits = n_me + n_pt <= 2u * IL_CAP;
  const uint32_t h = n_me <= (uint32_t)IL_CAP ? n_me : (fits ? n_me : IL_FALLBACK);
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = 0u;
  const uint32_t m = n_me < (uint32_t)IL_CAP ? n_me : (uint32_t)IL_CAP;
  const uint32_t x = (fits && n_pt > (uint32_t)IL_CAP) ? n_pt - IL_CAP : 0u;   // postings of the partner that sit here
  if (h != IL_FALLBACK) {
#pragma unroll
    for (int i = 0; i < IL_CAP; i++) {
      uint32_t src = 0xFFFFFFFFu;
      if ((uint32_t)i < m) src = me_lo + (uint32_t)i; else if ((uint32_t)i - m < x) src = pt_lo + (uint32_t)IL_CAP + ((uint32_t)i - m);
      if (src != 0xFFFFFFFFu) {
        const uint2 v = P[src];
        const unsigned long long W = ((unsigned long long)(v.x & tmask) << eb) | (unsigned long long)v.y;
        w[i] = (uint32_t)W;
        if (i < 8) w[14] |= ((uint32_t)(W >> 32) & 15u) << (4 * i); else w[15] |= ((uint32_t)(W >> 32) & 15u) << (4 * (i - 8));
      }
    }
  }
  w[15] |= h << 24;
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}
// One thread per line.  (Built by index_bins_kernel's own workgroups right after their scatter — the postings come back out of the L2, the
// buckets' ends are the scatter's cursors — it was SLOWER: a (slot, bin) workgroup has 16 to 128 pairs of lines for its 256 threads and every
// thread walks its pair serially: index build 0.91 -> 1.11 ms for a rank of eight at C2, the ordered kernel beside it 0.80 -> 1.0; C1
// 0.148 -> 0.242.  Round 6, EXPERIMENTS.md.)
constexpr int IL_THREADS = 256;
__global__ __launch_bounds__(IL_THREADS) void index_lines_kernel(InvIndex ix, int H) {
  const size_t t = (size_t)blockIdx.x * IL_THREADS + threadIdx.x;
  if (t >= ((size_t)H << ix.nl_log)) return;
  const size_t s = t >> ix.nl_log, l = t & (((size_t)1 << ix.nl_log) - 1);
  const uint32_t* E = ix.ends + s * ((size_t)ix.nb + 1) + ((l & ~(size_t)1) << ix.line_lb);   // ends at the pair's first bucket
  const uint32_t a = E[0], b = E[(size_t)1 << ix.line_lb], c = E[(size_t)2 << ix.line_lb];
  const bool odd = (l & 1) != 0;
  il_build_line(ix.items + s * ix.slot_stride, odd ? b : a, odd ? c - b : b - a, odd ? a : b, odd ? b - a : c - b, 0xFFFFFFFFu >> ix.nl_log, ix.line_ebits,
                (uint4*)(ix.lines + ((s << ix.nl_log) + l) * 16));
}
// Step 4, one workgroup per (slot, bin): the bin's postings move from `staged` to `items` grouped by bucket; the buckets' ends are
// written (ends[s][0] = 0 by bin 0).  sub = buckets per bin (a power of two, <= IB_SUB_MAX).
// (Round 6: the kernel is compiled for three sizes of a bin.  It used to reserve the counters of the largest — 32 KB, five workgroups of 256 lanes
//  per CU — whatever the index: one rank's shard of an 8-GPU job at C2 has 256 buckets and ~195 postings per (slot, bin), 65 536 workgroups of
//  which 1 280 were resident, most of their lanes without a posting: 0.46 ms where an eighth of the one-GPU build is 0.16.  Small bins now take one
//  wavefront and 2 KB each, 32 of them per CU.)
constexpr int IB_SUB_MAX = 8192;
template <int SUBCAP, int IB_FIN_THREADS>
__global__ __launch_bounds__(IB_FIN_THREADS) void index_bins_kernel(InvIndex ix) {
  __shared__ uint32_t cnt[SUBCAP];
  __shared__ uint32_t wsum[IB_FIN_THREADS / 64];
  __shared__ uint32_t s_carry, s_long;
  const int s = blockIdx.x >> IB_BINS_LOG, bin = blockIdx.x & (IB_BINS - 1);
  const int sub = (int)(ix.nb >> IB_BINS_LOG), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t* bs = ix.bin_start + (size_t)s * (IB_BINS + 1) + bin;
  const uint32_t lo = bs[0], n = bs[1] - lo;
  const uint2* in = ix.staged + (size_t)s * ix.slot_stride + lo;
  uint2* out = ix.items + (size_t)s * ix.slot_stride + lo;
  uint32_t* ends = ix.ends + (size_t)s * ((size_t)ix.nb + 1) + (size_t)bin * sub + 1;
  for (int i = threadIdx.x; i < sub; i += IB_FIN_THREADS) cnt[i] = 0;
  if (threadIdx.x == 0) { s_carry = 0; s_long = 0; if (bin == 0) ends[-1] = 0; }
  __syncthreads();
  const uint32_t smask = (uint32_t)sub - 1u;
  for (uint32_t i = threadIdx.x; i < n; i += IB_FIN_THREADS) atomicAdd(&cnt[(in[i].x >> ix.shift) & smask], 1u);
  __syncthreads();
  for (int base = 0; base < sub; base += IB_FIN_THREADS) {      // exclusive scan of the counts; ends = inclusive
    const int i = base + (int)threadIdx.x;
    const uint32_t v = i < sub ? cnt[i] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if (lane >= off) incl += t; }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t before = s_carry, total = 0;
    for (int w = 0; w < IB_FIN_THREADS / 64; w++) { const uint32_t t = wsum[w]; if (w < wv) before += t; total += t; }
    if (i < sub) { cnt[i] = before + incl - v; ends[i] = lo + before + incl; }
    if (v > ix.group_t) s_long = 1;                      // (benign race: every writer stores 1)
    __syncthreads();
    if (threadIdx.x == 0) s_carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) ix.bin_long[blockIdx.x] = s_long;
  for (uint32_t i = threadIdx.x; i < n; i += IB_FIN_THREADS) {
    const uint2 x = in[i];
    out[atomicAdd(&cnt[(x.x >> ix.shift) & smask], 1u)] = x;
  }
}

// Step 5, large indexes only (index_wants_grouping): the postings of every LONG bucket — a value thousands of stored entries share:
// a repeat — are put in ascending order of their entry CLASS (entry >> IB_CLASS_LOG), by a counting sort through `staged` (free again
// once step 4 is done).  The dense query tier counts hits in passes over ranges of stored entries; before this step every pass of a
// repeat-carrying query streamed all of its buckets again and kept the 1/npass that fell into its range (39 passes at 1.25 M entries:
// 14 us per query on one rank's share of BASELINE configs[4], 560 ms for 40 000 queries); with the classes in order a pass finds its
// part of a long bucket by bisection and streams only that.  One workgroup per (slot, bin), like step 4.
constexpr int IB_GROUP_T = 256;          // buckets up to this long are streamed whole by every pass (InvIndex::group_t)
constexpr int IB_CLASS_LOG = 15;         // entries per class: the finest range a dense pass covers (ranges are power-of-two multiples of it; InvIndex::class_log)
constexpr int IB_MAX_CLASSES = 8192;     // class counters in LDS (2^28 entries); an index beyond that is left ungrouped
constexpr int IB_GRP_THREADS = 256;
__global__ __launch_bounds__(IB_GRP_THREADS) void index_group_kernel(InvIndex ix) {
  __shared__ uint32_t cls[IB_MAX_CLASSES];
  __shared__ uint32_t longs[IB_GRP_THREADS];
  __shared__ uint32_t s_nlong, s_carry;
  __shared__ uint32_t wsum[IB_GRP_THREADS / 64];
  const int s = blockIdx.x >> IB_BINS_LOG, bin = blockIdx.x & (IB_BINS - 1);
  const int sub = (int)(ix.nb >> IB_BINS_LOG), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t* ends = ix.ends + (size_t)s * ((size_t)ix.nb + 1) + (size_t)bin * sub;   // ends[i] .. ends[i + 1]: bucket i of this bin
  uint2* items = ix.items + (size_t)s * ix.slot_stride;
  uint2* staged = ix.staged + (size_t)s * ix.slot_stride;
  const int nclass = (int)((ix.ne + (1u << ix.class_log) - 1) >> ix.class_log);
  if (!ix.bin_long[blockIdx.x]) return;                  // (step 4 saw no long bucket in this bin: nearly every bin of an index without repeats)
  for (int w0 = 0; w0 < sub; w0 += IB_GRP_THREADS) {     // windows of IB_GRP_THREADS buckets: the list of a window's long ones cannot overflow
    __syncthreads();
    if (threadIdx.x == 0) s_nlong = 0;
    __syncthreads();
    {
      const int i = w0 + (int)threadIdx.x;
      if (i < sub && ends[i + 1] - ends[i] > ix.group_t) longs[atomicAdd(&s_nlong, 1u)] = (uint32_t)i;
    }
    __syncthreads();
    const uint32_t nl = s_nlong;
    for (uint32_t li = 0; li < nl; li++) {
      const uint32_t b = longs[li], lo = ends[b], n = ends[b + 1] - lo;
      for (int c = threadIdx.x; c < nclass; c += IB_GRP_THREADS) cls[c] = 0;
      if (threadIdx.x == 0) s_carry = 0;
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < n; i += IB_GRP_THREADS) {
        const uint2 x = items[lo + i];
        staged[lo + i] = x;
        atomicAdd(&cls[x.y >> ix.class_log], 1u);
      }
      __syncthreads();
      for (int cb = 0; cb < nclass; cb += IB_GRP_THREADS) {        // exclusive scan of the class counts
        const int c = cb + (int)threadIdx.x;
        const uint32_t v = c < nclass ? cls[c] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = s_carry, total = 0;
        for (int w = 0; w < IB_GRP_THREADS / 64; w++) { const uint32_t t = wsum[w]; if (w < wv) before += t; total += t; }
        if (c < nclass) cls[c] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += total;
        __syncthreads();
      }
      for (uint32_t i = threadIdx.x; i < n; i += IB_GRP_THREADS) {
        const uint2 x = staged[lo + i];
        items[lo + atomicAdd(&cls[x.y >> ix.class_log], 1u)] = x;
      }
      __syncthreads();
    }
  }
}

// lines per slot and posting layout for an index of `entries` entries in nb buckets per slot; false: no line table (a posting would not
// fit its 36 bits, or MHAP_INDEX_LINES=0).  Average postings per line: 3.5 .. 7 (IL_CAP = 14 places, 28 with the partner's)
bool index_line_params(int64_t entries, uint32_t nb, uint32_t& nl_log, uint32_t& lb, uint32_t& ebits) {
  // Default: a line table for an index of 8 192 to 262 144 entries.  Measured in round 6 (EXPERIMENTS.md; hits queued, one build thread per
  // line), index_query / index_build / step, without -> with: rank of eight at C2 (25 000 entries) 1.47 -> 1.03 / 0.78 -> 0.88 / 14.9 -> 14.4 ms;
  // C2 on one GPU (200 000) 2.29 -> 1.79 / 2.94 -> 3.80 / 95.2 -> 94.8 (even: the build runs next to the ordered kernel); rank of eight at C4
  // (250 000) 19.4 -> 11.7 / 3.7 -> 5.0 / 194 -> 189; C4 on one GPU (2 M entries: the middle tier) 76.8 -> 73.5 / 35.3 -> 44.4 / 1466 -> 1471;
  // one rank's share of configs[4] (1.25 M, repeat-rich: the dense tier) 392 -> 405 / 23 -> 29 / 3314 -> 3362; C1 (2 000) 0.041 -> 0.051 /
  // 0.139 -> 0.147 / 0.93 -> 0.98.  So: the sizes where the first tier does the work and the table stays near the caches.
  // MHAP_INDEX_LINES=0 / 1: never / whenever the layout allows.
  const char* e = getenv("MHAP_INDEX_LINES");
  if (e && e[0] == '0') return false;
  if (!(e && e[0] == '1') && (entries < 8192 || entries > 262144)) return false;
  const int64_t per_line = []() { const char* v = getenv("MHAP_INDEX_LINE_LOAD"); const int x = v ? atoi(v) : 0; return (int64_t)(x >= 1 && x <= 14 ? x : 7); }();
  uint32_t nbl = 0;
  while ((1u << nbl) < nb) nbl++;
  uint32_t l = 1;
  while (l < nbl && ((int64_t)1 << l) * per_line < entries) l++;
  if (((int64_t)1 << l) * per_line < entries) return false;          // (an index beyond nb * 7 entries: more than 7 M)
  ebits = 1;
  while (ebits < 32 && ((int64_t)1 << ebits) < entries) ebits++;     // entry < entries <= 2^ebits
  if ((32 - l) + ebits > 36) return false;
  nl_log = l; lb = nbl - l;
  return true;
}
size_t index_line_bytes(int H, uint32_t nl_log) { return (size_t)H * ((size_t)64 << nl_log); }

// Self-check (MHAP_DEBUG_INDEX=1, tests): every stored (entry, slot) finds its posting in its bucket; counts the ones that do not.
__global__ void index_verify_kernel(const int32_t* __restrict__ minhash, int64_t row_stride, const int32_t* __restrict__ meta, int ne, int H, InvIndex ix,
                                    unsigned long long* __restrict__ missing) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)ne * H) return;
  const int e = (int)(t / H), s = (int)(t % H);
  if (meta[(int64_t)e * META_W + 3] != 0) return;
  const uint32_t hv = inv_mix((uint32_t)minhash[(int64_t)e * row_stride + s]);
  const uint32_t* E = ix.ends + (size_t)s * ((size_t)ix.nb + 1) + (hv >> ix.shift);
  const uint2* P = ix.items + (size_t)s * ix.slot_stride;
  // (a grouped index: a long bucket's postings are in ascending class order — checked from this entry's own posting backwards)
  for (uint32_t i = E[0]; i < E[1]; i++)
    if (P[i].x == hv && P[i].y == (uint32_t)e) {
      if (ix.grouped && E[1] - E[0] > ix.group_t && i > E[0] && (P[i - 1].y >> ix.class_log) > (P[i].y >> ix.class_log)) break;
      return;
    }
  atomicAdd(missing, 1ULL);
}
// ... and, through the line table, by the rules of the first query tier (a line that says "see the buckets" counts as found)
__global__ void index_verify_lines_kernel(const int32_t* __restrict__ minhash, int64_t row_stride, const int32_t* __restrict__ meta, int ne, int H, InvIndex ix,
                                          unsigned long long* __restrict__ missing) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)ne * H) return;
  const int e = (int)(t / H), s = (int)(t % H);
  if (meta[(int64_t)e * META_W + 3] != 0) return;
  const uint32_t hv = inv_mix((uint32_t)minhash[(int64_t)e * row_stride + s]);
  const uint32_t lsh = 32u - ix.nl_log, tmask = 0xFFFFFFFFu >> ix.nl_log, eb = ix.line_ebits, emk = (1u << eb) - 1u;
  const uint32_t line = hv >> lsh;
  const uint32_t* L = ix.lines + (((size_t)s << ix.nl_log) + line) * 16;
  const uint32_t hdr = L[15] >> 24;
  if (hdr == IL_FALLBACK) return;
  int found = 0;
  auto scan = [&](const uint32_t* W, uint32_t from, uint32_t to) {
    for (uint32_t i = from; i < to && i < (uint32_t)IL_CAP; i++) {
      const uint32_t nib = ((i < 8 ? W[14] >> (4 * i) : W[15] >> (4 * (i - 8))) & 15u);
      const unsigned long long P = ((unsigned long long)nib << 32) | W[i];
      if ((uint32_t)(P >> eb) == (hv & tmask) && (uint32_t)(P & emk) == (uint32_t)e) found++;
    }
  };
  scan(L, 0u, hdr);
  if (hdr > (uint32_t)IL_CAP) {
    const uint32_t* Q = ix.lines + (((size_t)s << ix.nl_log) + (line ^ 1u)) * 16;
    const uint32_t pn = Q[15] >> 24;
    if (pn >= (uint32_t)IL_CAP) { atomicAdd(missing, 1ULL); return; }
    scan(Q, pn, pn + hdr - (uint32_t)IL_CAP);
  }
  if (found != 1) atomicAdd(missing, 1ULL);
}
void launch_index_verify(hipStream_t st, const int32_t* minhash, int64_t row_stride, const int32_t* meta, int ne, int H, const InvIndex& ix,
                         unsigned long long* missing) {
  const long long total = (long long)ne * H;
  if (total <= 0) return;
  hipLaunchKernelGGL(index_verify_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, minhash, row_stride, meta, ne, H, ix, missing);
  if (ix.lines)
    hipLaunchKernelGGL(index_verify_lines_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, minhash, row_stride, meta, ne, H, ix, missing);
}

// (Round 6: a small index — one rank's shard of an 8-GPU job at C2: 25 000 entries — had 7 tiles x 64 slot groups = 448 workgroups for 256 CUs;
//  tiles of 1 024 entries give it four times as many.  Their shares of a bin are 64 bytes: the scatter's half-written lines — what made 512
//  coarse bins slow at C2 — meet in the caches while the whole staging area is a few hundred MB.)
// (read at every call: tests switch MHAP_INDEX_TILE inside one process; inv_alloc calls this once per index and keeps the answer in
//  InvIndex::tile_entries / tiles, which size tile_counts and which launch_index_build launches with)
int index_tile_entries(int ne) {
  const char* e = getenv("MHAP_INDEX_TILE");
  const int force = e ? atoi(e) : 0;
  if (force >= 256 && force <= IB_TE) return force;
  return ne <= 65536 ? 1024 : IB_TE;
}
int index_coarse_bins() { return IB_BINS; }
int index_max_buckets_log() { return IB_BINS_LOG + 13; }   // IB_SUB_MAX buckets per coarse bin
// (re)build the index for entries [0, ne): ix.ends / items / staged / tile_counts / bin_start, and ix.tile_entries / tiles, set by the caller
// (inv_alloc) for these ne entries.  False: the tiles do not cover ne entries (nothing launched).
bool launch_index_build(hipStream_t st, const int32_t* minhash, int64_t row_stride, const int32_t* meta, int ne, int H, const InvIndex& ix) {
  if ((int64_t)ne * H <= 0) return true;
  const int tiles = (int)ix.tiles, te = (int)ix.tile_entries;
  if (te <= 0 || (int64_t)tiles * te < (int64_t)ne) return false;
  const unsigned grid = (unsigned)tiles * (unsigned)((H + IB_S - 1) / IB_S);
  hipLaunchKernelGGL(index_tile_kernel<false>, dim3(grid), dim3(IB_THREADS), 0, st, minhash, row_stride, meta, ne, H, tiles, te, ix);
  hipLaunchKernelGGL(index_offsets_kernel, dim3((unsigned)H), dim3(IB_BINS), 0, st, ix, tiles);
  hipLaunchKernelGGL(index_tile_kernel<true>, dim3(grid), dim3(IB_THREADS), 0, st, minhash, row_stride, meta, ne, H, tiles, te, ix);
  const int sub = (int)(ix.nb >> IB_BINS_LOG);
  int launched;
  {
    const dim3 g((unsigned)H << IB_BINS_LOG);
    const char* e = getenv("MHAP_INDEX_BINS_SHAPE");   // 0 / 1 / 2: pin a shape that fits (A/B; read at every build: tests switch it inside one process)
    const int force = e ? atoi(e) : -1;
    const int shape = force >= 0 ? force : (sub <= 512 ? 0 : (sub <= 2048 ? 1 : 2));
    if (shape == 0 && sub <= 512) { hipLaunchKernelGGL((index_bins_kernel<512, 64>), g, dim3(64), 0, st, ix); launched = 0; }
    else if (shape <= 1 && sub <= 2048) { hipLaunchKernelGGL((index_bins_kernel<2048, 256>), g, dim3(256), 0, st, ix); launched = 1; }
    else { hipLaunchKernelGGL((index_bins_kernel<IB_SUB_MAX, 256>), g, dim3(256), 0, st, ix); launched = 2; }
  }
  if (ix.grouped) hipLaunchKernelGGL(index_group_kernel, dim3((unsigned)H << IB_BINS_LOG), dim3(IB_GRP_THREADS), 0, st, ix);
  if (ix.lines) {
    const size_t threads = (size_t)H << ix.nl_log;
    hipLaunchKernelGGL(index_lines_kernel, dim3((unsigned)((threads + IL_THREADS - 1) / IL_THREADS)), dim3(IL_THREADS), 0, st, ix, H);
  }
  if (getenv("MHAP_HOST_PROF"))   // which build ran (tests assert it)
    fprintf(stderr, "[index build] entries %d tile_entries %d tiles %d sub %d bins_shape %d grouped %u lines %d\n", ne, te, tiles, sub, launched,
            ix.grouped, ix.lines ? 1 : 0);
  return true;
}
// (called when the index is sized: an index the compact dense tier covers in one pass gains nothing from the order, and the class
//  counters bound the size from above.  MHAP_INDEX_GROUP=0|1 never / always, MHAP_INDEX_GROUP_T, MHAP_INDEX_CLASS_LOG: tests, which
//  have to make a few hundred entries look like a million)
void index_group_params(int64_t entries, InvIndex& ix) {
  // (read at every build: tests switch them inside one process)
  const int force = []() { const char* e = getenv("MHAP_INDEX_GROUP"); return e ? atoi(e) : -1; }();
  const int gt = []() { const char* e = getenv("MHAP_INDEX_GROUP_T"); const int v = e ? atoi(e) : 0; return v > 0 ? v : IB_GROUP_T; }();
  const int cl = []() { const char* e = getenv("MHAP_INDEX_CLASS_LOG"); const int v = e ? atoi(e) : 0; return v > 0 && v <= 24 ? v : IB_CLASS_LOG; }();
  ix.group_t = (uint32_t)gt; ix.class_log = (uint32_t)cl;
  const bool fits = entries <= ((int64_t)IB_MAX_CLASSES << cl);
  ix.grouped = (fits && (force >= 0 ? force != 0 : entries > (1LL << 18))) ? 1u : 0u;   // (more than two passes of the compact dense tier)
}

// One workgroup (one wavefront) per query.  LDS: tbl[CT], a hit-count table of packed words: entry + 1 in the low `ebits` bits (as
// many as the index needs), its saturating hit count in the bits above.
#ifndef MH_IQ_THREADS
#define MH_IQ_THREADS 64
#endif
constexpr int IQ_THREADS = MH_IQ_THREADS;   // lanes per query: 64 / 128 / 256 at C2: 4.04 / 4.30 / 6.35 ms with a 2048-entry two-word table, 3.3 with the
                                  // packed one (one rank of eight: 2.5 / 3.4 / 5.7): one wavefront's barriers are free and its 8 KB let 15 of them share a CU
constexpr int IQ_STACK = 48;      // pending (prefix, bits) parts of a query whose hit set is being split
#ifndef MH_IQ_SPT
#define MH_IQ_SPT 1   // 1 / 2 / 4 at C2 with 128 lanes: 4.7 / 4.7 / 5.7 ms; with 64: 4.08 / 4.07 / 4.44 (the queue's LDS costs resident workgroups)
#endif
constexpr int IQ_SPT = MH_IQ_SPT;   // slots a lane of the first tier looks up per trip (their loads are in flight together)
constexpr int IQ_INLINE = 16;     // a bucket up to this long is read by the lane that looked it up; longer ones are streamed by the workgroup
#ifndef MH_IQ_BIG_CT
#define MH_IQ_BIG_CT 16384   // (0: no further tiers — every hit set that outgrows the first tier's table is split there)
#endif
// Tiers (launch_index_query).  <INV_CT, IQ_THREADS> takes every query; one whose buckets hold more postings than the table can
// count (repeats: thousands of stored entries share a MinHash value with the query), or whose distinct hits outgrow the table, is
// appended to `big` and handed on: to the dense tier (index_query_dense_kernel), on a large index through <INV_CT_MID,
// IQ_THREADS_MID> first.  big == nullptr (MHAP_INDEX_TIERS=1, tests): the hit set is split into hash-partition passes over the
// stored entries instead (split in two until every part fits), which bounds a query's cost by its own postings.
#ifndef MH_IQ_TIMING
#define MH_IQ_TIMING 0   // timing builds of the first query tier (results wrong): 1 no `elements` atomic, 2 no hit counting, 4 no global atomic in the emit
#endif
constexpr int IQ_OV = 64;    // line mode: slots of one query that may fall back to ends / items (more: the query is handed on)
#ifndef MH_IQ_QUAD
#define MH_IQ_QUAD 0   // line mode: 1 = four lanes share a line (one 16-byte quarter each), 0 = a line per lane (four 16-byte loads).  Measured (round 6,
                       // emulated rank of eight at C2 / C2 on one GPU / rank of eight at C4): see EXPERIMENTS.md
#endif
#ifndef MH_IQ_LB
#define MH_IQ_LB 4
#endif
constexpr int IQ_LB = MH_IQ_LB;   // line mode: lines a lane has in flight
constexpr int IQ_PRE = 12;   // slots per lane whose first look is kept (H <= 768 with 64 lanes; twelve elements: the compiler addresses such a vector by a uniform index)
typedef int iq_pre_t __attribute__((ext_vector_type(IQ_PRE)));
template <int INV_CT, int IQ_THREADS, int SPT, bool LINES>
__global__ __launch_bounds__(IQ_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void index_query_kernel(InvIndex ix, const int32_t* __restrict__ qminhash, int64_t qrow_stride,
                                                          const int32_t* __restrict__ qlist, int nq, const int64_t* __restrict__ ids,
                                                          const int64_t* __restrict__ qids, const int32_t* __restrict__ meta,
                                                          const int32_t* __restrict__ qmeta, SearchParams sp,
                                                          Candidate* __restrict__ cand, unsigned long long* __restrict__ cand_count,
                                                          unsigned long long cand_cap, unsigned long long* __restrict__ split_count,
                                                          unsigned long long* __restrict__ elements, int32_t* __restrict__ big,
                                                          unsigned long long* __restrict__ big_count) {
  __shared__ uint32_t tbl[INV_CT];
  static_assert(INV_CT <= 32 * IQ_THREADS, "the emit mask holds 32 table slots per lane");
  __shared__ uint32_t s_distinct, s_over, s_top, s_prefix, s_bits;
  __shared__ uint32_t stack[2 * IQ_STACK];
  __shared__ uint32_t s_nseg[2];
  constexpr int QCAP = IQ_THREADS * SPT;   // a trip looks SPT slots per lane up (their loads in flight together) and may queue as many buckets
  __shared__ uint32_t segraw[QCAP * 4];
  uint2* const seglist = (uint2*)segraw;  // queued long buckets: (first posting within the slot, length),
  uint2* const segkey = seglist + QCAP;   // ... (slot, the query's mix there)
  uint32_t* const hitq = segraw;          // (line mode, before any bucket is queued: the entries whose tag matched, waiting to be counted)
  constexpr int IQ_HQ = QCAP * 4;
  __shared__ unsigned long long segpre[QCAP + 1];
  __shared__ unsigned long long wsum[IQ_THREADS / 64];
  __shared__ unsigned long long s_base;
  const int qi = blockIdx.x;
  if (qi >= nq) return;
  const int qe = qlist[qi];
  const int32_t* qm = qmeta + (int64_t)qe * META_W;
  if (qm[3] != 0) return;   // (a strand that was not sketched is no query: a list made on the device — launch_query_iota — names every row)
  const int64_t qid = qids[qe];
  const int qlen = qm[2];
  const int32_t* qrow = qminhash + (int64_t)qe * qrow_stride;
  const size_t eper = (size_t)ix.nb + 1;
  // (what the first look at the buckets found — the mixed value, the bucket's start and length of the lane's first IQ_PRE slots — stays in
  //  registers for the counting loop below, which used to load the query's value and the bucket's bounds a second time: two of the three
  //  dependent round trips of each of its trips.  C2 3.29 -> 2.87 ms, a rank of eight 2.65 -> 2.17.  Requesting the next trip's postings a
  //  trip ahead on top of it — with the mixed value recomputed, or the kernel drops to three waves per SIMD — gave nothing: 3.03 / 2.18)
  iq_pre_t pre_hv = 0, pre_lo = 0, pre_n = 0;
  bool pre_ok = false;
  // round 6: the index has a LINE table (index_lines_kernel) and this launch hands its large hit sets on: one 64-byte line per lookup
  // instead of bucket bounds + postings; only slots whose line says "long bucket" (a repeat) go through ends / items below
  constexpr bool lmode = LINES;   // (launch_index_query: big != nullptr && ix.lines != nullptr)
  __shared__ uint32_t s_nov;
  __shared__ uint32_t ovlist[IQ_OV];
  if (big != nullptr && !lmode) {
    // first tier: the buckets' lengths alone say whether this table can hold the hits — a repeat-rich query is handed over after
    // H loads instead of after counting until the table overflows
    unsigned long long tot = 0;
    // (two loops: the first IQ_PRE trips write the kept vectors with STATIC element indices.  As one loop with `if (itp < IQ_PRE)` the
    //  element write was compiled to an indexed register move executed for every trip — beyond --num-hashes 768 it wrote past the vectors
    //  into whatever registers followed, and from --num-hashes 2 752 on it hit a live pointer: a memory fault in this kernel, found
    //  by a parameter sweep in round 5)
#pragma unroll
    for (int itp = 0; itp < IQ_PRE; itp++) {
      const int s = (int)threadIdx.x + itp * IQ_THREADS;
      if (s < sp.H) {
        const uint32_t hvp = inv_mix((uint32_t)qrow[s]);
        const uint32_t* E = ix.ends + (size_t)s * eper + (hvp >> ix.shift);
        const uint32_t e0 = E[0], e1 = E[1];
        tot += e1 - e0;
        pre_hv[itp] = (int)hvp; pre_lo[itp] = (int)e0; pre_n[itp] = (int)(e1 - e0);
      }
    }
    for (int s = (int)threadIdx.x + IQ_PRE * IQ_THREADS; s < sp.H; s += IQ_THREADS) {
      const uint32_t hvp = inv_mix((uint32_t)qrow[s]);
      const uint32_t* E = ix.ends + (size_t)s * eper + (hvp >> ix.shift);
      tot += E[1] - E[0];
    }
    pre_ok = true;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = tot;
    __syncthreads();
    tot = 0;
    for (unsigned w = 0; w < IQ_THREADS / 64; w++) tot += wsum[w];
    // (tot counts every posting of the H buckets: the hits plus ~ne/nb strangers per bucket; distinct hits <= hits.  Beyond a
    // quarter over the table's capacity the count would very likely overflow half-way and be thrown away)
    // (in a self search the query's own strand is stored: its H postings are ONE distinct entry — without this term every query of a run at
    //  --num-hashes 2048 was handed over on its own postings alone: index query 4.9 ms for 20 000 queries where the first tier takes 2.4)
    const unsigned long long strangers = (unsigned long long)sp.H * ix.ne / ix.nb + (sp.to_self ? (unsigned long long)sp.H : 0ULL);
    if (tot > strangers + (5ULL * (INV_CT * 3 / 4)) / 4) {
      if (threadIdx.x == 0) big[atomicAdd(big_count, 1ULL)] = qe;
      return;
    }
  }
  if (threadIdx.x == 0) { stack[0] = 0; stack[1] = 0; s_top = 1; }
  __syncthreads();
  for (;;) {
    // ---- next part of the stored entries: those whose hash has `bits` low bits equal to `prefix` (the whole index first) ----
    if (threadIdx.x == 0) {
      if (s_top == 0) s_bits = 0xFFFFFFFFu;
      else { s_top--; s_prefix = stack[2 * s_top]; s_bits = stack[2 * s_top + 1]; }
      s_distinct = 0; s_over = 0; s_nseg[0] = 0; s_nseg[1] = 0; s_nov = 0;
    }
    for (int j = threadIdx.x; j < INV_CT; j += IQ_THREADS) tbl[j] = 0;
    __syncthreads();
    const uint32_t bits = s_bits, prefix = s_prefix;
    if (bits == 0xFFFFFFFFu) break;
    constexpr int CT_LOG = __builtin_ctz((unsigned)INV_CT), MAX_BITS = 32 - CT_LOG;   // part bits sit above the home-slot bits
    const uint32_t pmask = bits >= (uint32_t)MAX_BITS ? (0xFFFFFFFFu >> CT_LOG) : ((1u << bits) - 1u);
    unsigned long long mine = 0;
    // count one hit of stored entry `me` (the id/length rules do not depend on the count: they are applied to the few entries that
    // reach numMinMatches, below, so that the lookup loop's only global loads are the index words)
    // The count is read before it is raised and left alone from `sat` on, so it passes `sat` by at most the adds in flight — one per
    // lane of the workgroup — and the field must hold sat + IQ_THREADS: index_query_tier_ok() keeps a launch out of this kernel when
    // the bits the entries leave are too few for that (the middle tier is given 10 bits, i.e. an index below 2^22 entries).
    const int ebits = 32 - __builtin_clz(ix.ne | 1u);                   // entry + 1 <= ne fits
    const uint32_t emask = ebits >= 32 ? 0xFFFFFFFFu : ((1u << ebits) - 1u), cone = ebits >= 32 ? 0u : (1u << ebits);
    const uint32_t cmax = ebits >= 32 ? 0u : (0xFFFFFFFFu >> ebits);
    const uint32_t sat = (uint32_t)sp.num_min_matches < cmax - (uint32_t)IQ_THREADS ? (uint32_t)sp.num_min_matches : cmax - (uint32_t)IQ_THREADS;
    auto count_hit = [&](int me) {
      if (MH_IQ_TIMING & 2) return;
      // (a self search of one index: the query's own strand is stored — H hits on one table word per query, six in seven of all the hits a
      //  C2 query counts, for the one pair the id rule drops anyway)
      if (sp.own_queries && me == qe) return;
      const uint32_t hm = inv_mix((uint32_t)me);
      if (((hm >> CT_LOG) & pmask) != prefix) return;
      const uint32_t id = (uint32_t)me + 1u;
      uint32_t slot = hm & (INV_CT - 1);
      for (int tries = 0; tries < INV_CT; tries++) {
        uint32_t w = __hip_atomic_load(&tbl[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((w & emask) == 0) {
          if (__hip_atomic_load(&s_distinct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (INV_CT * 3) / 4) { s_over = 1; break; }
          const uint32_t old = atomicCAS(&tbl[slot], 0u, id);
          if (old == 0) { atomicAdd(&s_distinct, 1u); w = id; } else w = old;
        }
        if ((w & emask) == id) { if ((w >> ebits) < sat) atomicAdd(&tbl[slot], cone); break; }
        slot = (slot + 1) & (INV_CT - 1);
      }
    };
    bool handed_over = false;
    int nloop = sp.H;
#if MH_IQ_QUAD
    if (lmode) {
      const uint32_t lsh = 32u - ix.nl_log, tmask = 0xFFFFFFFFu >> ix.nl_log, eb = ix.line_ebits, emk = (1u << eb) - 1u, hsh = 32u - eb;
      const size_t lstride = (size_t)16 << ix.nl_log;   // words of one slot's lines
      // FOUR lanes per lookup, one 16-byte quarter of the line each: a wave's load instruction then touches 16 lines instead of 64 —
      // tools/line_gather_probe.hip: the same 51.2 M lookups out of a 17-GB table (all of C4 on one GPU) take 2.6 ms with a line per lane
      // and 1.06 ms with a line per quad; no difference at 0.13 / 1.1 GB (0.9 ms) — and a lookup in flight costs 4 registers, not 16.
      // Lane 4 g + p holds places 4 p .. 4 p + 3 of group g's line (p = 3: places 12, 13, then the words with the places' top bits
      // and the header, which the other three lanes fetch through a quad broadcast).
      const int part = (int)(threadIdx.x & 3u), grp = (int)(threadIdx.x >> 2);
      constexpr int GPI = IQ_THREADS / 4;     // lookups one wave instruction covers
      auto bcast3 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xFF, 0xF, 0xF, true); };   // quad_perm [3,3,3,3]
      // places [from, to) of the line quarter q (of the lane's part) against the query's tag
      auto scan = [&](const uint4 q, uint32_t w14, uint32_t w15, uint32_t from, uint32_t to, uint32_t qt) {
        const uint32_t nibs = ((part & 2) ? w15 : w14) >> ((part & 1) * 16);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int jx = 0; jx < 4; jx++) {
          const uint32_t place = (uint32_t)(part * 4 + jx);
          const uint32_t tag = (w[jx] >> eb) | (((nibs >> (4 * jx)) & 15u) << hsh);
          if (place < (uint32_t)IL_CAP && place >= from && place < to && tag == qt) { mine++; count_hit((int)(w[jx] & emk)); }
        }
      };
      for (int sb = 0; sb < sp.H; sb += IQ_LB * GPI) {      // (workgroup-uniform bounds; no barrier inside)
        uint4 L[IQ_LB];
        uint32_t hvv[IQ_LB];
#pragma unroll
        for (int u = 0; u < IQ_LB; u++) {
          const int s = sb + u * GPI + grp;
          hvv[u] = 0; L[u] = make_uint4(0u, 0u, 0u, 0u);
          if (s < sp.H) {
            hvv[u] = inv_mix((uint32_t)qrow[s]);
            L[u] = ((const uint4*)(ix.lines + (size_t)s * lstride + ((size_t)(hvv[u] >> lsh) << 4)))[part];
          }
        }
        uint32_t more = 0;   // bit u: lookup u goes on in its partner line
        uint32_t nn[IQ_LB];
#pragma unroll
        for (int u = 0; u < IQ_LB; u++) {
          const int s = sb + u * GPI + grp;
          const uint32_t w14 = bcast3(L[u].z), w15 = bcast3(L[u].w), hdr = w15 >> 24;
          nn[u] = hdr;
          if (s < sp.H && hdr) {
            if (hdr == IL_FALLBACK) {
              if (part == 0) { const uint32_t at = atomicAdd(&s_nov, 1u); if (at < (uint32_t)IQ_OV) ovlist[at] = (uint32_t)s; }
            } else {
              scan(L[u], w14, w15, 0u, hdr, hvv[u] & tmask);
              if (hdr > (uint32_t)IL_CAP) more |= 1u << u;
            }
          }
        }
        if (__builtin_amdgcn_ballot_w64(more != 0u)) {
          // what a line of more than 14 postings could not hold sits in its partner line, behind the partner's own
#pragma unroll
          for (int u = 0; u < IQ_LB; u++)
            if ((more >> u) & 1u)
              L[u] = ((const uint4*)(ix.lines + (size_t)(sb + u * GPI + grp) * lstride + ((size_t)((hvv[u] >> lsh) ^ 1u) << 4)))[part];
#pragma unroll
          for (int u = 0; u < IQ_LB; u++) {
            // (the broadcasts run for the whole wave: a DPP read of a lane that is switched off returns nothing useful)
            const uint32_t w14 = bcast3(L[u].z), w15 = bcast3(L[u].w);
            if ((more >> u) & 1u) { const uint32_t pn = w15 >> 24; scan(L[u], w14, w15, pn, pn + nn[u] - (uint32_t)IL_CAP, hvv[u] & tmask); }
          }
        }
      }
#else
    if (lmode) {
      // (the queue is per WAVE — ballots compact within a wave — so the 256-lane middle tier runs the same code: IQ_HQ / waves words each)
      const uint32_t lsh = 32u - ix.nl_log, tmask = 0xFFFFFFFFu >> ix.nl_log, eb = ix.line_ebits, emk = (1u << eb) - 1u, hsh = 32u - eb;
      const size_t lstride = (size_t)16 << ix.nl_log;   // words of one slot's lines
      // Hits are QUEUED, not counted where they are found: a match is one lane in a hundred per place, and counting it on the spot sent the
      // whole wave through the hit-count table's probe loop (LDS atomics, their waits) 14 places x 8 lookups = 112 times a query — the timing
      // build without the counting ran C2's first tier in 1.05 ms against 2.26 with it (round 6).  The scan is executed by all lanes together
      // (a lane without a line scans the empty range), a ballot compacts the matching entries into hitq, and the queue is counted by a loop in
      // which every lane has a hit to count.
      int hbase = 0;                 // hits waiting in this wave's queue (wave-uniform)
      unsigned long long nhits = 0;  // ... and all hits so far ("table elements processed")
      constexpr int HQW = IQ_HQ / (IQ_THREADS / 64);                 // words of one wave's queue (256)
      static_assert(HQW >= 128, "a place adds up to 64 hits to a queue that is flushed beyond HQW - 64");
      uint32_t* const hq = hitq + (threadIdx.x >> 6) * HQW;
      const int wlane = (int)(threadIdx.x & 63u);
      auto flush_hits = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int i = wlane; i < hbase; i += 64) count_hit((int)hq[i]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        hbase = 0;
      };
      // a posting of place i of line words L: tag above the entry's bits; the place's top 4 bits sit in words 14 / 15
#define IQ_LINE_SCAN(L, from, to, qtag)                                                                                   \
      {                                                                                                                     \
        const uint32_t lw_[14] = {L[0].x, L[0].y, L[0].z, L[0].w, L[1].x, L[1].y, L[1].z, L[1].w, L[2].x, L[2].y, L[2].z, L[2].w, L[3].x, L[3].y}; \
        _Pragma("unroll") for (int i_ = 0; i_ < IL_CAP; i_++) {                                                              \
          const uint32_t nib_ = ((i_ < 8 ? L[3].z >> (4 * i_) : L[3].w >> (4 * (i_ - 8))) & 15u);                            \
          const uint32_t tag_ = (lw_[i_] >> eb) | (nib_ << hsh);                                                             \
          const bool hit_ = (uint32_t)i_ >= (from) && (uint32_t)i_ < (to) && tag_ == (qtag);                                  \
          const unsigned long long bal_ = __builtin_amdgcn_ballot_w64(hit_);                                                  \
          if (bal_) {                                                                                                        \
            if (hit_) hq[hbase + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal_ >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal_, 0u))] = lw_[i_] & emk; \
            const int np_ = __popcll(bal_);                                                                                  \
            hbase += np_; nhits += (unsigned long long)np_;                                                                  \
            if (hbase > HQW - 64) flush_hits();                                                                              \
          }                                                                                                                 \
        }                                                                                                                   \
      }
      for (int sb0 = 0; sb0 < sp.H; sb0 += IQ_LB * IQ_THREADS) {     // (wave-uniform trip count: the scans below are executed by all lanes)
        const int sb = sb0 + (int)threadIdx.x;
        uint4 L[IQ_LB][4];
        uint32_t hvv[IQ_LB], nn[IQ_LB];
#pragma unroll
        for (int u = 0; u < IQ_LB; u++) {
          const int s = sb + u * IQ_THREADS;
          hvv[u] = 0;
          L[u][0] = L[u][1] = L[u][2] = L[u][3] = make_uint4(0u, 0u, 0u, 0u);
          if (s < sp.H) {
            hvv[u] = inv_mix((uint32_t)qrow[s]);
            const uint4* l4 = (const uint4*)(ix.lines + (size_t)s * lstride + ((size_t)(hvv[u] >> lsh) << 4));
            L[u][0] = l4[0]; L[u][1] = l4[1]; L[u][2] = l4[2]; L[u][3] = l4[3];
          }
        }
        bool partner = false;
#pragma unroll
        for (int u = 0; u < IQ_LB; u++) {
          const int s = sb + u * IQ_THREADS;
          const uint32_t hdr = L[u][3].w >> 24;      // (0 for a lane without a slot: nothing to scan)
          nn[u] = 0;
          if (hdr == IL_FALLBACK) {
            const uint32_t at = atomicAdd(&s_nov, 1u);
            if (at < (uint32_t)IQ_OV) ovlist[at] = (uint32_t)s;
          } else nn[u] = hdr;
          const uint32_t qt = hvv[u] & tmask;
          IQ_LINE_SCAN(L[u], 0u, nn[u], qt);
          partner = partner || nn[u] > (uint32_t)IL_CAP;
        }
        if (__builtin_amdgcn_ballot_w64(partner)) {
          // what a line of more than 14 postings could not hold sits in its partner line, behind the partner's own
#pragma unroll
          for (int u = 0; u < IQ_LB; u++)
            if (nn[u] > (uint32_t)IL_CAP) {
              const uint4* l4 = (const uint4*)(ix.lines + (size_t)(sb + u * IQ_THREADS) * lstride + ((size_t)((hvv[u] >> lsh) ^ 1u) << 4));
              L[u][0] = l4[0]; L[u][1] = l4[1]; L[u][2] = l4[2]; L[u][3] = l4[3];
            }
#pragma unroll
          for (int u = 0; u < IQ_LB; u++) {
            const bool pm = nn[u] > (uint32_t)IL_CAP;
            const uint32_t pn = pm ? L[u][3].w >> 24 : 0u, pe = pm ? pn + nn[u] - (uint32_t)IL_CAP : 0u, qt = hvv[u] & tmask;
            IQ_LINE_SCAN(L[u], pn, pe, qt);
          }
        }
      }
      flush_hits();
      if (wlane == 0) mine += nhits;
#undef IQ_LINE_SCAN
#endif
      __syncthreads();
      const uint32_t nov = s_nov;
      if (nov > (uint32_t)IQ_OV) { if (threadIdx.x == 0) s_over = 1; nloop = 0; }   // (a query with that many long buckets is repeat-rich: handed on)
      else {
        nloop = (int)nov;
        if (nov) {
          // the long buckets' lengths say whether this table can hold their hits — the plain path's early hand-over, for the slots the
          // lines sent here (without it a repeat-rich query with a few dozen long buckets streamed all of them before its table
          // overflowed: C5 slice, first tier 4.6 -> 33 ms with the line table)
          unsigned long long tot = 0;
          for (uint32_t i = threadIdx.x; i < nov; i += IQ_THREADS) {
            const uint32_t so = ovlist[i];
            const uint32_t hvp = inv_mix((uint32_t)qrow[so]);
            const uint32_t* E = ix.ends + (size_t)so * eper + (hvp >> ix.shift);
            tot += E[1] - E[0];
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
          if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = tot;
          __syncthreads();
          tot = 0;
          for (unsigned w = 0; w < IQ_THREADS / 64; w++) tot += wsum[w];
          if (tot + s_distinct > (5ULL * (INV_CT * 3 / 4)) / 4) { if (threadIdx.x == 0) s_over = 1; nloop = 0; }
        }
      }
      __syncthreads();
    }
    for (int s0 = 0, it = 0; s0 < nloop; s0 += QCAP, it++) {   // workgroup-uniform trip count (barriers inside)
      uint32_t hv[SPT], lo[SPT], n[SPT];
      int sl[SPT];   // the slot a lane looks up: all of them in turn, or (line mode) the slots whose line said "see the buckets"
#pragma unroll
      for (int u = 0; u < SPT; u++) {
        const int idx = s0 + u * IQ_THREADS + (int)threadIdx.x;
        const int s = lmode ? (idx < nloop ? (int)ovlist[idx] : sp.H) : idx;
        sl[u] = s;
        hv[u] = 0; lo[u] = 0; n[u] = 0;
        if (pre_ok && it * SPT + u < IQ_PRE) {
          if (s < sp.H) { hv[u] = (uint32_t)pre_hv[it * SPT + u]; lo[u] = (uint32_t)pre_lo[it * SPT + u]; n[u] = (uint32_t)pre_n[it * SPT + u]; }
        } else if (s < sp.H) {
          hv[u] = inv_mix((uint32_t)qrow[s]);
          const uint32_t* E = ix.ends + (size_t)s * eper + (hv[u] >> ix.shift);
          lo[u] = E[0]; n[u] = E[1] - lo[u];
        }
      }
      uint2 w[SPT][4];                                                           // the usual bucket in one round trip
#pragma unroll
      for (int u = 0; u < SPT; u++) {
        const uint2* P = ix.items + (size_t)sl[u] * ix.slot_stride + lo[u];
        const uint32_t m = n[u] <= (uint32_t)IQ_INLINE ? n[u] : 0u;
#pragma unroll
        for (int x = 0; x < 4; x++) w[u][x] = (uint32_t)x < m ? P[x] : make_uint2(~hv[u], 0u);
      }
#pragma unroll
      for (int u = 0; u < SPT; u++) {
        const int s = sl[u];
        if (n[u] > (uint32_t)IQ_INLINE) {
          // a long bucket (a value many entries share): queued for the whole workgroup (a repeat's bucket holds tens of thousands
          // of postings: one lane would stream it alone)
          const uint32_t at = atomicAdd(&s_nseg[it & 1], 1u);
          seglist[at] = make_uint2(lo[u], n[u]); segkey[at] = make_uint2((uint32_t)s, hv[u]);
        } else if (n[u]) {
#pragma unroll
          for (int x = 0; x < 4; x++)
            if (w[u][x].x == hv[u]) { if (bits == 0) mine++; count_hit((int)w[u][x].y); }   // "table elements processed" (:173), counted once
          const uint2* P = ix.items + (size_t)s * ix.slot_stride + lo[u];
          for (uint32_t x = 4; x < n[u]; x++) {
            const uint2 y = P[x];
            if (y.x == hv[u]) { if (bits == 0) mine++; count_hit((int)y.y); }
          }
        }
      }
      __syncthreads();
      const uint32_t nseg = s_nseg[it & 1];
      const uint32_t over_now = s_over;
      if (threadIdx.x == 0) s_nseg[(it + 1) & 1] = 0;
      __syncthreads();                       // every lane holds the same (nseg, over_now) before anyone counts again
      if (big != nullptr && over_now) { handed_over = true; break; }            // first tier: the query is handed over, stop counting
      if (nseg) {
        // all queued buckets as ONE index space (exclusive prefix of their lengths in segpre): a trip of the loop below has
        // 8 x IQ_THREADS loads in flight whatever the buckets' lengths — one bucket per trip cost a memory round trip per
        // bucket, and repeat-rich queries queue a hundred short ones
        // (64-bit sums: a thousand buckets of a huge index can hold more than 2^32 postings between them)
        unsigned long long lens[SPT], len = 0;                                    // lane t holds buckets t * SPT .. t * SPT + SPT - 1
#pragma unroll
        for (int u = 0; u < SPT; u++) { const uint32_t q = threadIdx.x * SPT + u; lens[u] = q < nseg ? seglist[q].y : 0u; len += lens[u]; }
        unsigned long long incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned long long v = __shfl_up(incl, off); if ((threadIdx.x & 63) >= (unsigned)off) incl += v; }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned long long wbase = 0, total = 0;
        for (unsigned w = 0; w < IQ_THREADS / 64; w++) { const unsigned long long t = wsum[w]; if (w < (threadIdx.x >> 6)) wbase += t; total += t; }
        unsigned long long run = wbase + incl - len;
#pragma unroll
        for (int u = 0; u < SPT; u++) { const uint32_t q = threadIdx.x * SPT + u; if (q < nseg) segpre[q] = run; run += lens[u]; }
        if (threadIdx.x == 0) segpre[nseg] = total;
        __syncthreads();
        // second tier, whole index, every slot looked up: buckets with more than twice the table's capacity between them (and an
        // index with that many entries) are split before they are streamed: the pass would overflow after streaming everything
        // (the postings are still streamed, to count the ones that match — "table elements processed" — but no hit is counted)
        bool count_only = false;
        if (big == nullptr && bits == 0 && s0 + QCAP >= nloop && (total < ix.ne ? total : (unsigned long long)ix.ne) > 2ULL * (INV_CT * 3 / 4)) { if (threadIdx.x == 0) s_over = 1; count_only = true; }
        uint32_t g = 0;   // bucket of this lane's current posting (its postings come in ascending order)
        for (unsigned long long i0 = threadIdx.x; i0 - threadIdx.x < total; i0 += IQ_THREADS * 8) {
          uint2 e[8];
          uint32_t want[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const unsigned long long i = i0 + (unsigned long long)IQ_THREADS * u;
            e[u] = make_uint2(0u, 0u); want[u] = 1u;                               // (never equal)
            if (i < total) {
              while (i >= segpre[g + 1]) g++;
              const uint2 key = segkey[g];
              e[u] = ix.items[(size_t)key.x * ix.slot_stride + (size_t)seglist[g].x + (size_t)(i - segpre[g])];
              want[u] = key.y;
            }
          }
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (e[u].x == want[u]) { if (bits == 0) mine++; if (!count_only) count_hit((int)e[u].y); }
        }
        if (count_only) break;
        __syncthreads();         // the queue is reused by the next trip's lookups
      }
    }
    (void)handed_over;
    __syncthreads();
    if (!(MH_IQ_TIMING & 1)) iq_add_elements(elements, (s_over && big != nullptr) ? 0ULL : mine);   // (every wave of the workgroup gets here)
    if (s_over && big != nullptr) {
      // first tier: hand the query to the launch with the large count table (it starts over; nothing was emitted yet)
      if (threadIdx.x == 0) big[atomicAdd(big_count, 1ULL)] = qe;
      return;
    }
    if (s_over) {
      // the part's distinct hits outgrow the count table: split it in two and run both halves (exact; every stored entry
      // belongs to exactly one leaf part)
      if (threadIdx.x == 0) {
        if (bits < (uint32_t)MAX_BITS && s_top + 2 <= IQ_STACK) {
          stack[2 * s_top] = prefix; stack[2 * s_top + 1] = bits + 1; s_top++;
          stack[2 * s_top] = prefix | (1u << bits); stack[2 * s_top + 1] = bits + 1; s_top++;
        }
        atomicAdd(split_count, 1ULL);
      }
      __syncthreads();
      continue;
    }
    // emit this part's candidates as ONE contiguous block (one global atomic): the second stage then finds
    // the lanes of a wave sharing the query's ordered-sketch row
    uint32_t mymask = 0;   // bit t set -> table slot threadIdx.x + IQ_THREADS*t is a candidate
    int mycount = 0;
#pragma unroll
    for (int t = 0; t < INV_CT / IQ_THREADS; t++) {
      const int j = threadIdx.x + IQ_THREADS * t;
      const uint32_t w = tbl[j];
      if ((w & emask) != 0 && (int)(w >> ebits) >= sp.num_min_matches) {                          // MinHashSearch.java:204
        const int me = (int)(w & emask) - 1;
        if (pair_passes(sp, qid, ids[me], qlen, meta[(int64_t)me * META_W + 2])) { mymask |= 1u << t; mycount++; }   // :200-225
      }
    }
    __syncthreads();            // s_distinct is dead from here on: reuse it as the block's emit counter
    if (threadIdx.x == 0) s_distinct = 0;
    __syncthreads();
    uint32_t local = 0;
    if (mycount) local = atomicAdd(&s_distinct, (uint32_t)mycount);
    __syncthreads();
    if (threadIdx.x == 0) s_base = (s_distinct && !(MH_IQ_TIMING & 4)) ? atomicAdd(cand_count, (unsigned long long)s_distinct) : 0ULL;
    __syncthreads();
    unsigned long long slot = s_base + local;
#pragma unroll
    for (int t = 0; t < INV_CT / IQ_THREADS; t++) {
      if (mymask & (1u << t)) {
        if (slot < cand_cap) { cand[slot].q = qe; cand[slot].m = (int)(tbl[threadIdx.x + IQ_THREADS * t] & emask) - 1; }
        slot++;
      }
    }
    __syncthreads();
  }
}

// Second tier: DENSE counts.  A query the first tier hands over has thousands of distinct hits — on repeat-rich reads most of the
// index — and a hash table of them in LDS (rounds 1-2: 12 288 entries, beyond that hash-partition passes that each stream all of
// the query's postings again; 21 190 splits per step on the C5 slice) is the wrong structure: 64 KB of LDS hold a saturating
// 16-bit counter for each of 32 768 stored entries, indexed by the entry itself — no keys, no probing, no overflow.  An index
// with more entries is covered in passes over entry ranges of 32 768; the first pass notes which ranges the query's postings
// fall into and the others are skipped.
#ifndef MH_DQ_THREADS
#define MH_DQ_THREADS 512    // 1024 lanes + 65 536-entry ranges (one workgroup per CU) / 512 + 32 768 (two): C5 slice 12.2 / 10.8 ms — one
                            // query's zeroing and scan overlap the other's streaming, at the price of a third range pass over its 80 000 entries
#endif
#ifndef MH_DQ_RANGE_LOG
#define MH_DQ_RANGE_LOG 15
#endif
constexpr int DQ_THREADS = MH_DQ_THREADS, DQ_RANGE_LOG = MH_DQ_RANGE_LOG, DQ_MAX_RANGES = 4096;   // (an index of more than 4096 ranges = 2^28 entries runs every pass)
__global__ __launch_bounds__(DQ_THREADS) void index_query_dense_kernel(InvIndex ix, const int32_t* __restrict__ qminhash, int64_t qrow_stride,
                                                                       const int32_t* __restrict__ qlist, int nq, const int64_t* __restrict__ ids,
                                                                       const int64_t* __restrict__ qids, const int32_t* __restrict__ meta,
                                                                       const int32_t* __restrict__ qmeta, SearchParams sp, Candidate* __restrict__ cand,
                                                                       unsigned long long* __restrict__ cand_count, unsigned long long cand_cap,
                                                                       unsigned long long* __restrict__ split_count, unsigned long long* __restrict__ elements) {
  __shared__ uint32_t cnt[1 << (DQ_RANGE_LOG - 1)];     // two counters per word
  __shared__ uint2 seglist[DQ_THREADS];                 // queued long buckets: (first posting within the slot, length),
  __shared__ uint2 segkey[DQ_THREADS];                  // ... (slot, the query's mix there)
  __shared__ unsigned long long segpre[DQ_THREADS + 1];
  __shared__ unsigned long long wsum[DQ_THREADS / 64];
  __shared__ uint32_t rmask[DQ_MAX_RANGES / 32];        // ranges of stored entries the query's postings fall into
  __shared__ uint32_t s_nseg[2], s_emit;
  __shared__ unsigned long long s_base;
  const int qi = blockIdx.x;
  if (qi >= nq) return;
  const int qe = qlist[qi];
  const int32_t* qm = qmeta + (int64_t)qe * META_W;
  if (qm[3] != 0) return;   // (a strand that was not sketched is no query: a list made on the device — launch_query_iota — names every row)
  const int64_t qid = qids[qe];
  const int qlen = qm[2];
  const int32_t* qrow = qminhash + (int64_t)qe * qrow_stride;
  const size_t eper = (size_t)ix.nb + 1;
  const uint32_t npass = (ix.ne + (1u << DQ_RANGE_LOG) - 1) >> DQ_RANGE_LOG;
  const uint32_t sat = (uint32_t)(sp.num_min_matches < 0xF000 ? (sp.num_min_matches > 0 ? sp.num_min_matches : 1) : 0xF000);   // counts stop here
  for (int j = threadIdx.x; j < DQ_MAX_RANGES / 32; j += DQ_THREADS) rmask[j] = 0;
  unsigned long long mine = 0;
  for (uint32_t pass = 0; pass < npass; pass++) {
    __syncthreads();
    if (pass > 0 && !((rmask[(pass >> 5) & (DQ_MAX_RANGES / 32 - 1)] >> (pass & 31)) & 1u) && npass <= (uint32_t)DQ_MAX_RANGES) continue;   // (uniform)
    const uint32_t span = min(1u << DQ_RANGE_LOG, ix.ne - (pass << DQ_RANGE_LOG));   // stored entries of this range (the last one is partial)
    for (uint32_t j = threadIdx.x; j < (span + 1) / 2; j += DQ_THREADS) cnt[j] = 0;
    if (threadIdx.x == 0) { s_nseg[0] = 0; s_nseg[1] = 0; s_emit = 0; }
    __syncthreads();
    // one hit of stored entry `me`: the counter is read first and left alone once it has reached numMinMatches, so it can pass
    // that by no more than the adds in flight (8 x 1024) and never carries into its neighbour
#define DQ_COUNT_HIT(me_)                                                                                             \
    do {                                                                                                              \
      const uint32_t me = (me_);                                                                                      \
      if (pass == 0) { mine++; const uint32_t r = me >> DQ_RANGE_LOG; if (r) atomicOr(&rmask[(r >> 5) & (DQ_MAX_RANGES / 32 - 1)], 1u << (r & 31)); }   \
      if ((me >> DQ_RANGE_LOG) == pass) {                                                                             \
        const uint32_t wi = (me & ((1u << DQ_RANGE_LOG) - 1)) >> 1;                                                   \
        const int sh = (int)(me & 1u) * 16;                                                                           \
        if (((__hip_atomic_load(&cnt[wi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> sh) & 0xFFFFu) < sat) atomicAdd(&cnt[wi], 1u << sh);   \
      }                                                                                                               \
    } while (0)
    for (int s0 = 0, it = 0; s0 < sp.H; s0 += DQ_THREADS, it++) {   // workgroup-uniform trip count (barriers inside)
      const int s = s0 + (int)threadIdx.x;
      if (s < sp.H) {
        const uint32_t hv = inv_mix((uint32_t)qrow[s]);
        const uint32_t* E = ix.ends + (size_t)s * eper + (hv >> ix.shift);
        const uint32_t lo = E[0], n = E[1] - lo;
        if (n > (uint32_t)IQ_INLINE) {
          const uint32_t at = atomicAdd(&s_nseg[it & 1], 1u);
          seglist[at] = make_uint2(lo, n); segkey[at] = make_uint2((uint32_t)s, hv);
        } else {
          const uint2* P = ix.items + (size_t)s * ix.slot_stride + lo;
          for (uint32_t u = 0; u < n; u++) { const uint2 x = P[u]; if (x.x == hv) DQ_COUNT_HIT(x.y); }
        }
      }
      __syncthreads();
      const uint32_t nseg = s_nseg[it & 1];
      if (threadIdx.x == 0) s_nseg[(it + 1) & 1] = 0;
      __syncthreads();
      if (nseg) {
        // all queued buckets as ONE index space (exclusive prefix of their lengths in segpre): a trip of the loop below has
        // 8 x 1024 loads in flight whatever the buckets' lengths
        unsigned long long len = threadIdx.x < nseg ? seglist[threadIdx.x].y : 0u, incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned long long v = __shfl_up(incl, off); if ((threadIdx.x & 63) >= (unsigned)off) incl += v; }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned long long wbase = 0, total = 0;
        for (unsigned w = 0; w < DQ_THREADS / 64; w++) { const unsigned long long t = wsum[w]; if (w < (threadIdx.x >> 6)) wbase += t; total += t; }
        if (threadIdx.x < nseg) segpre[threadIdx.x] = wbase + incl - len;
        if (threadIdx.x == 0) segpre[nseg] = total;
        __syncthreads();
        uint32_t g = 0;   // bucket of this lane's current posting (its postings come in ascending order)
        for (unsigned long long i0 = threadIdx.x; i0 - threadIdx.x < total; i0 += DQ_THREADS * 8) {
          uint2 e[8];
          uint32_t want[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const unsigned long long i = i0 + (unsigned long long)DQ_THREADS * u;
            e[u] = make_uint2(0u, 0u); want[u] = 1u;                               // (never equal)
            if (i < total) {
              while (i >= segpre[g + 1]) g++;
              const uint2 key = segkey[g];
              e[u] = ix.items[(size_t)key.x * ix.slot_stride + (size_t)seglist[g].x + (size_t)(i - segpre[g])];
              want[u] = key.y;
            }
          }
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (e[u].x == want[u]) DQ_COUNT_HIT(e[u].y);
        }
        __syncthreads();         // the queue is reused by the next trip's lookups
      }
    }
#undef DQ_COUNT_HIT
    __syncthreads();
    if (pass == 0) iq_add_elements(elements, mine);           // "table elements processed" (:173), counted once
    if (pass > 0 && threadIdx.x == 0) atomicAdd(split_count, 1ULL);   // a pass beyond the first = the hit set was split
    // emit this range's candidates as ONE contiguous block (one global atomic)
    constexpr int PER = (1 << DQ_RANGE_LOG) / DQ_THREADS;      // 64 entries per lane: lane t owns entries t * 64 .. t * 64 + 63 of the range
    unsigned long long mymask = 0;
    int mycount = 0;
    const int jmax = threadIdx.x * PER >= span ? 0 : (int)min((uint32_t)PER, span - threadIdx.x * PER + 1) / 2;
    for (int j = 0; j < jmax; j++) {
      const uint32_t w = cnt[threadIdx.x * (PER / 2) + j];
#pragma unroll
      for (int hf = 0; hf < 2; hf++) {
        if ((int)((w >> (16 * hf)) & 0xFFFFu) >= sp.num_min_matches) {                             // MinHashSearch.java:204
          const uint32_t me = (pass << DQ_RANGE_LOG) + threadIdx.x * PER + 2 * j + hf;
          if (me < ix.ne && pair_passes(sp, qid, ids[me], qlen, meta[(int64_t)me * META_W + 2])) { mymask |= 1ULL << (2 * j + hf); mycount++; }   // :200-225
        }
      }
    }
    uint32_t local = 0;
    if (mycount) local = atomicAdd(&s_emit, (uint32_t)mycount);
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_emit ? atomicAdd(cand_count, (unsigned long long)s_emit) : 0ULL;
    __syncthreads();
    unsigned long long slot = s_base + local;
    while (mymask) {
      const int b = __builtin_ctzll(mymask);
      mymask &= mymask - 1;
      if (slot < cand_cap) { cand[slot].q = qe; cand[slot].m = (int)((pass << DQ_RANGE_LOG) + threadIdx.x * PER + b); }
      slot++;
    }
  }
}

// Dense tier, compact form (round 4): --num-hashes <= 512 (one slot per lane) and numMinMatches <= 4 — every BASELINE configuration.
// Differences from the kernel above:
//  * a THERMOMETER of 4 bits per stored entry instead of a 16-bit counter: hit k of an entry sets bit k (atomicOr; the returned word
//    says whether the bit was already there, in which case the next one is tried), "count >= numMinMatches" is one bit.  OR is
//    idempotent, so no add in flight can carry into a neighbour, and 64 KB of LDS cover 131 072 stored entries per pass instead of
//    32 768: a quarter of the passes;
//  * the H buckets are looked up ONCE (registers), not once per pass;
//  * on a grouped index (index_group_kernel) a pass streams only ITS part of a long bucket: the parts' bounds are found by
//    bisection, all passes and buckets at once, before the first pass.  One rank's share of BASELINE configs[4] (1.25 M entries,
//    repeat-carrying queries with 250 000 postings each): every posting is now streamed once instead of 39 times.
constexpr int DQ2_THREADS = 512, DQ2_RANGE_LOG = 17, DQ2_WORDS = 1 << (DQ2_RANGE_LOG - 3), DQ2_MAX_RANGES = 1024, DQ2_BOUNDS = 512;
constexpr uint32_t DQ2_NOGRP = 0x3FFu;
__global__ __launch_bounds__(DQ2_THREADS) void index_query_dense4_kernel(InvIndex ix, const int32_t* __restrict__ qminhash, int64_t qrow_stride,
                                                                         const int32_t* __restrict__ qlist, int nq, const int64_t* __restrict__ ids,
                                                                         const int64_t* __restrict__ qids, const int32_t* __restrict__ meta,
                                                                         const int32_t* __restrict__ qmeta, SearchParams sp, Candidate* __restrict__ cand,
                                                                         unsigned long long* __restrict__ cand_count, unsigned long long cand_cap,
                                                                         unsigned long long* __restrict__ split_count, unsigned long long* __restrict__ elements,
                                                                         const uint32_t range_log /* <= DQ2_RANGE_LOG: entries per pass (tests shrink it) */) {
  __shared__ __align__(16) uint32_t cnt[DQ2_WORDS];    // eight 4-bit thermometers per word
  __shared__ uint2 seglist[DQ2_THREADS];                // queued buckets (longer than IQ_INLINE): (first posting within the slot, length),
  __shared__ uint2 segkey[DQ2_THREADS];                 // ... (slot | bounds row << 16, the query's mix there)
  __shared__ unsigned long long segpre[DQ2_THREADS + 1];
  __shared__ uint32_t bounds[DQ2_BOUNDS];               // per grouped long bucket: npass + 1 offsets, the starts of the passes' parts
  __shared__ unsigned long long wsum[DQ2_THREADS / 64];
  __shared__ uint32_t rmask[DQ2_MAX_RANGES / 32];       // ranges of stored entries the query's postings fall into
  __shared__ uint32_t s_nseg, s_ng, s_emit;
  __shared__ unsigned long long s_base;
  const int qi = blockIdx.x;
  if (qi >= nq) return;
  const int qe = qlist[qi];
  const int32_t* qm = qmeta + (int64_t)qe * META_W;
  if (qm[3] != 0) return;   // (a strand that was not sketched is no query: a list made on the device — launch_query_iota — names every row)
  const int64_t qid = qids[qe];
  const int qlen = qm[2];
  const int32_t* qrow = qminhash + (int64_t)qe * qrow_stride;
  const size_t eper = (size_t)ix.nb + 1;
  const uint32_t npass = (ix.ne + (1u << range_log) - 1) >> range_log;
  const int nmm = sp.num_min_matches < 1 ? 1 : sp.num_min_matches;     // (<= 4: launch_index_query)
  const uint32_t topmask = 0x11111111u << (nmm - 1);
  // ---- the H lookups, once ----
  const int s = (int)threadIdx.x;
  uint32_t hv = 0, lo = 0, n = 0;
  if (s < sp.H) {
    hv = inv_mix((uint32_t)qrow[s]);
    const uint32_t* E = ix.ends + (size_t)s * eper + (hv >> ix.shift);
    lo = E[0]; n = E[1] - lo;
  }
  if (threadIdx.x < DQ2_MAX_RANGES / 32) rmask[threadIdx.x] = 0;
  if (threadIdx.x == 0) { s_nseg = 0; s_ng = 0; }
  __syncthreads();
  const uint32_t per = npass + 1;
  const uint32_t gcap = (ix.grouped && range_log >= ix.class_log && npass > 1 && per <= (uint32_t)DQ2_BOUNDS) ? (uint32_t)DQ2_BOUNDS / per : 0u;
  if (n > (uint32_t)IQ_INLINE) {
    const uint32_t at = atomicAdd(&s_nseg, 1u);
    uint32_t g = DQ2_NOGRP;
    if (gcap && n > ix.group_t) { const uint32_t g2 = atomicAdd(&s_ng, 1u); if (g2 < gcap) g = g2; }   // (no room: streamed whole by every pass)
    seglist[at] = make_uint2(lo, n); segkey[at] = make_uint2((uint32_t)s | (g << 16), hv);
  }
  __syncthreads();
  const uint32_t nseg = s_nseg;
  if (gcap) {
    // bounds[g][p] = first posting of the bucket whose entry lies in range p or beyond (classes ascend within a long bucket)
    for (uint32_t i = threadIdx.x; i < nseg * per; i += DQ2_THREADS) {
      const uint32_t at = i / per, p = i % per, g = segkey[at].x >> 16;
      if (g == DQ2_NOGRP) continue;
      const uint2 sl = seglist[at];
      uint32_t b = 0;
      if (p == npass) b = sl.y;
      else if (p > 0) {
        const uint2* P = ix.items + (size_t)(segkey[at].x & 0xFFFFu) * ix.slot_stride + sl.x;
        uint32_t a = 0, z = sl.y;                                   // first j in [0, n) with class(j) >= p
        while (a < z) { const uint32_t m = (a + z) >> 1; if ((P[m].y >> range_log) < p) a = m + 1; else z = m; }
        b = a;
      }
      bounds[g * per + p] = b;
    }
    __syncthreads();
    const uint32_t ng = s_ng < gcap ? s_ng : gcap;
    if (npass <= (uint32_t)DQ2_MAX_RANGES)
      for (uint32_t i = threadIdx.x; i < ng * npass; i += DQ2_THREADS) {
        const uint32_t g = i / npass, p = i % npass;
        if (p && bounds[g * per + p + 1] > bounds[g * per + p]) atomicOr(&rmask[p >> 5], 1u << (p & 31));
      }
  }
  // a short bucket (read by the lane that looked it up) is read ONCE: its postings with the query's value — none, one or two, nearly
  // always — stay in registers for the passes.  (Every pass read the bucket again, posting after posting, each load waiting for the
  // one before: with ten passes over 1.25 M entries that was a fifth of this kernel.)
  uint32_t in_me0 = 0, in_me1 = 0;
  int in_cnt = 0;
  if (n && n <= (uint32_t)IQ_INLINE) {
    const uint2* P = ix.items + (size_t)s * ix.slot_stride + lo;
    for (uint32_t u0 = 0; u0 < n; u0 += 4) {
      uint2 x[4];
#pragma unroll
      for (int c = 0; c < 4; c++) { x[c] = make_uint2(~hv, 0u); if (u0 + (uint32_t)c < n) x[c] = P[u0 + (uint32_t)c]; }
#pragma unroll
      for (int c = 0; c < 4; c++)
        if (x[c].x == hv) { if (in_cnt == 0) in_me0 = x[c].y; else if (in_cnt == 1) in_me1 = x[c].y; in_cnt++; }
    }
  }
  unsigned long long mine = 0;
  for (uint32_t pass = 0; pass < npass; pass++) {
    __syncthreads();
    if (pass > 0 && npass <= (uint32_t)DQ2_MAX_RANGES && !((rmask[pass >> 5] >> (pass & 31)) & 1u)) continue;   // (uniform)
    const uint32_t span = min(1u << range_log, ix.ne - (pass << range_log));   // stored entries of this range (the last one is partial)
    for (uint32_t j = threadIdx.x * 4; j < (span + 7) / 8; j += DQ2_THREADS * 4) *(uint4*)&cnt[j] = make_uint4(0u, 0u, 0u, 0u);   // (16 bytes per lane: whole vectors, the last one past the span's words too)
    if (threadIdx.x == 0) s_emit = 0;
    __syncthreads();
    // one hit of stored entry `me` (celem: this posting has not been seen by an earlier pass — "table elements processed", :173)
#define DQ2_HIT(me_, celem)                                                                                           \
    do {                                                                                                              \
      const uint32_t me = (me_);                                                                                      \
      if (celem) mine++;                                                                                              \
      if (pass == 0 && npass > 1) { const uint32_t r = me >> range_log; if (r && r < (uint32_t)DQ2_MAX_RANGES) atomicOr(&rmask[r >> 5], 1u << (r & 31)); }   \
      if ((me >> range_log) == pass) {                                                                            \
        const uint32_t wi = (me & ((1u << range_log) - 1)) >> 3;                                                  \
        const int sh = (int)(me & 7u) * 4;                                                                            \
        for (int k = 0; k < nmm; k++) { const uint32_t old = atomicOr(&cnt[wi], (1u << k) << sh); if (!((old >> sh) & (1u << k))) break; }   \
      }                                                                                                               \
    } while (0)
    if (n && n <= (uint32_t)IQ_INLINE) {
      if (in_cnt <= 2) {
        if (in_cnt > 0) DQ2_HIT(in_me0, pass == 0);
        if (in_cnt > 1) DQ2_HIT(in_me1, pass == 0);
      } else {
        const uint2* P = ix.items + (size_t)s * ix.slot_stride + lo;
        for (uint32_t u = 0; u < n; u++) { const uint2 x = P[u]; if (x.x == hv) DQ2_HIT(x.y, pass == 0); }
      }
    }
    if (nseg) {
      // the queued buckets — of a grouped one this pass's part — as ONE index space (exclusive prefix of the lengths in segpre)
      unsigned long long len = 0;
      if (threadIdx.x < nseg) {
        const uint32_t g = segkey[threadIdx.x].x >> 16;
        len = g == DQ2_NOGRP ? seglist[threadIdx.x].y : bounds[g * per + pass + 1] - bounds[g * per + pass];
      }
      unsigned long long incl = len;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const unsigned long long v = __shfl_up(incl, off); if ((threadIdx.x & 63) >= (unsigned)off) incl += v; }
      if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
      __syncthreads();
      unsigned long long wbase = 0, total = 0;
      for (unsigned w = 0; w < DQ2_THREADS / 64; w++) { const unsigned long long t = wsum[w]; if (w < (threadIdx.x >> 6)) wbase += t; total += t; }
      if (threadIdx.x < nseg) segpre[threadIdx.x] = wbase + incl - len;
      if (threadIdx.x == 0) segpre[nseg] = total;
      __syncthreads();
      // this lane's current queue entry, cached in registers: its span of the index space, where its postings start, the query's mix there.
      // (The first version looked all of that up in LDS for every posting — five dependent LDS reads in front of each load, eight
      //  postings per trip one after the other: the address arithmetic took as long as the memory round trip it was meant to keep busy.)
      uint32_t g = 0;
      unsigned long long seg_beg = 0, seg_end = 0;
      const uint2* seg_base = nullptr;
      uint32_t seg_want = 1u;
      bool seg_fresh = false;
      for (unsigned long long i0 = threadIdx.x; i0 - threadIdx.x < total; i0 += DQ2_THREADS * 8) {
        uint2 e[8];
        uint32_t want[8];
        bool fresh[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const unsigned long long i = i0 + (unsigned long long)DQ2_THREADS * u;
          e[u] = make_uint2(0u, 0u); want[u] = 1u; fresh[u] = false;              // (never equal)
          if (i < total) {
            if (i >= seg_end) {                                                    // (its postings come in ascending order)
              while (i >= segpre[g + 1]) g++;
              seg_beg = segpre[g]; seg_end = segpre[g + 1];
              const uint2 key = segkey[g];
              const uint32_t grp = key.x >> 16;
              const uint32_t off = grp == DQ2_NOGRP ? 0u : bounds[grp * per + pass];
              seg_base = ix.items + (size_t)(key.x & 0xFFFFu) * ix.slot_stride + (size_t)seglist[g].x + (size_t)off;
              seg_want = key.y;
              seg_fresh = grp != DQ2_NOGRP || pass == 0;
            }
            e[u] = seg_base[(size_t)(i - seg_beg)];
            want[u] = seg_want;
            fresh[u] = seg_fresh;
          }
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (e[u].x == want[u]) DQ2_HIT(e[u].y, fresh[u]);
      }
    }
#undef DQ2_HIT
    __syncthreads();
    if (pass > 0 && threadIdx.x == 0) atomicAdd(split_count, 1ULL);   // a pass beyond the first = the hit set was split
    // emit this range's candidates as ONE contiguous block (one global atomic).  Lane t owns the four-word vectors t, t + 512, ... of the
    // counters (16-byte LDS accesses, conflict-free; a pass of a repeat-carrying query touches a few thousand of the 131 072 entries, so
    // nearly every vector is skipped on one test: zeroing and sweeping word by word cost a query more LDS instructions than its postings);
    // entries that reached numMinMatches but fail the id / length rules lose their top bit in the first sweep, so the second one only
    // enumerates bits.
    const uint32_t nwords = (span + 7) / 8;
    int mycount = 0;
    for (uint32_t w4 = threadIdx.x * 4; w4 < nwords; w4 += DQ2_THREADS * 4) {
      const uint4 v = *(const uint4*)&cnt[w4];
      if (((v.x | v.y | v.z | v.w) & topmask) == 0u) continue;
      const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int c = 0; c < 4; c++) {
        uint32_t w = vw[c], m = w & topmask;
        if (!m) continue;
        const uint32_t wi = w4 + (uint32_t)c;
        while (m) {
          const int b = __builtin_ctz(m);
          m &= m - 1;
          const uint32_t me = (pass << range_log) + wi * 8 + (uint32_t)(b >> 2);
          if (me < ix.ne && pair_passes(sp, qid, ids[me], qlen, meta[(int64_t)me * META_W + 2])) mycount++;   // MinHashSearch.java:200-225
          else w &= ~(1u << b);
        }
        cnt[wi] = w;
      }
    }
    uint32_t local = 0;
    if (mycount) local = atomicAdd(&s_emit, (uint32_t)mycount);
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_emit ? atomicAdd(cand_count, (unsigned long long)s_emit) : 0ULL;
    __syncthreads();
    unsigned long long slot = s_base + local;
    if (mycount)
      for (uint32_t w4 = threadIdx.x * 4; w4 < nwords; w4 += DQ2_THREADS * 4) {
        const uint4 v = *(const uint4*)&cnt[w4];
        if (((v.x | v.y | v.z | v.w) & topmask) == 0u) continue;
        const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; c++) {
          uint32_t m = vw[c] & topmask;
          while (m) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            if (slot < cand_cap) { cand[slot].q = qe; cand[slot].m = (int)((pass << range_log) + (w4 + (uint32_t)c) * 8 + (uint32_t)(b >> 2)); }
            slot++;
          }
        }
      }
  }
  iq_add_elements(elements, mine);           // "table elements processed" (:173): every posting with the query's value, once
}

bool index_query_tiers() { return MH_IQ_BIG_CT != 0; }
// whether the packed table words of tier 0 (IQ_THREADS lanes) / tier 1 (IQ_THREADS_MID lanes) can count to numMinMatches for an index
// of this many entries: the count field (the bits the entry index leaves) must hold numMinMatches + one add in flight per lane
bool index_query_tier_ok(int tier, int64_t entries, int num_min_matches) {
  if (entries < 1 || entries >= (1LL << 31)) return false;
  int ebits = 1;
  while ((1LL << ebits) <= entries) ebits++;            // entry + 1 <= entries < 2^ebits
  const long long cmax = (1LL << (32 - ebits)) - 1;
  return (long long)num_min_matches + (tier == 0 ? IQ_THREADS : 512) <= cmax;   // (512: an upper bound of the middle tier's lanes)
}

// tier 0: the first tier (one wavefront per query, 2048-entry table); tier 1: the same kernel with an 8192-entry table and 256 lanes
// (queries of a LARGE index that outgrow the first table but have thousands, not hundreds of thousands, of hits: the dense tier would
// make a pass per 32 768 stored entries for them); tier 2: the dense tier.  big / big_count: where tiers 0 and 1 list the queries
// they hand on (nullptr: they split hit sets into hash-partition passes instead).
#ifndef MH_IQ_MID_CT
#define MH_IQ_MID_CT 8192    // 16384 entries + 512 lanes / 8192 + 256 / 4096 + 128 on all of C4: 136 / 81 / 78 ms of index query (more workgroups per
                            // CU again); 8192 holds the 2-3 thousand hits of an ordinary read of a large data set with room to spare
#endif
#ifndef MH_IQ_MID_THREADS
#define MH_IQ_MID_THREADS 256
#endif
constexpr int INV_CT_MID = MH_IQ_MID_CT, IQ_THREADS_MID = MH_IQ_MID_THREADS;
// the query list "every row": qlist[i] = first + i (the kernels above skip the rows whose status says "not sketched").  Round 6: the search of
// device-resident query rows used to wait for the rows' meta words on the host, a host loop over them and the upload of the list it made
// before its first kernel: 0.35 ms of a 2.1-ms search on one rank of eight.
__global__ __launch_bounds__(256) void query_iota_kernel(int32_t* __restrict__ qlist, int first, int n) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) qlist[i] = first + i;
}
void launch_query_iota(hipStream_t st, int32_t* qlist, int first, int n) {
  if (n > 0) hipLaunchKernelGGL(query_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, qlist, first, n);
}
void launch_index_query(hipStream_t st, const InvIndex& ix, const int32_t* qminhash, int64_t qrow_stride,
                        const int32_t* qlist, int nq, const int64_t* ids, const int64_t* qids, const int32_t* meta, const int32_t* qmeta,
                        const SearchParams& sp, Candidate* cand, unsigned long long* cand_count, unsigned long long cand_cap,
                        unsigned long long* split_count, unsigned long long* elements_total, int32_t* big, unsigned long long* big_count, int tier,
                        unsigned long long* elements) {
  // elements: index_elements_spread_words() zeroed words the kernels add to; folded into *elements_total (and zeroed again) behind the launch
  if (nq <= 0) return;
  struct Fold { hipStream_t st; unsigned long long* s; unsigned long long* t; ~Fold() { hipLaunchKernelGGL(index_elements_sum_kernel, dim3(1), dim3(IQ_ELEM_SPREAD), 0, st, s, t); } } fold{st, elements, elements_total};
  if (tier == 0 && big != nullptr && ix.lines != nullptr)
    hipLaunchKernelGGL((index_query_kernel<INV_CT, IQ_THREADS, IQ_SPT, true>), dim3((unsigned)nq), dim3(IQ_THREADS), 0, st, ix, qminhash, qrow_stride, qlist, nq, ids, qids,
                       meta, qmeta, sp, cand, cand_count, cand_cap, split_count, elements, big, big_count);
  else if (tier == 0)
    hipLaunchKernelGGL((index_query_kernel<INV_CT, IQ_THREADS, IQ_SPT, false>), dim3((unsigned)nq), dim3(IQ_THREADS), 0, st, ix, qminhash, qrow_stride, qlist, nq, ids, qids,
                       meta, qmeta, sp, cand, cand_count, cand_cap, split_count, elements, big, big_count);
  else if (tier == 1 && big != nullptr && ix.lines != nullptr)
    hipLaunchKernelGGL((index_query_kernel<INV_CT_MID, IQ_THREADS_MID, 1, true>), dim3((unsigned)nq), dim3(IQ_THREADS_MID), 0, st, ix, qminhash, qrow_stride, qlist, nq,
                       ids, qids, meta, qmeta, sp, cand, cand_count, cand_cap, split_count, elements, big, big_count);
  else if (tier == 1)
    hipLaunchKernelGGL((index_query_kernel<INV_CT_MID, IQ_THREADS_MID, 1, false>), dim3((unsigned)nq), dim3(IQ_THREADS_MID), 0, st, ix, qminhash, qrow_stride, qlist, nq,
                       ids, qids, meta, qmeta, sp, cand, cand_count, cand_cap, split_count, elements, big, big_count);
  else {
    const bool old_dense = []() { const char* e = getenv("MHAP_DENSE_TIER"); return e && strcmp(e, "counters") == 0; }();   // (the 16-bit-counter kernel for every case: tests)
    const uint32_t range_log = []() { const char* e = getenv("MHAP_DENSE_RANGE_LOG"); const int v = e ? atoi(e) : 0; return (uint32_t)(v >= 3 && v <= DQ2_RANGE_LOG ? v : DQ2_RANGE_LOG); }();
    if (sp.H <= DQ2_THREADS && sp.num_min_matches <= 4 && !old_dense)
      hipLaunchKernelGGL(index_query_dense4_kernel, dim3((unsigned)nq), dim3(DQ2_THREADS), 0, st, ix, qminhash, qrow_stride, qlist, nq, ids, qids, meta, qmeta, sp,
                         cand, cand_count, cand_cap, split_count, elements, range_log);
    else
      hipLaunchKernelGGL(index_query_dense_kernel, dim3((unsigned)nq), dim3(DQ_THREADS), 0, st, ix, qminhash, qrow_stride, qlist, nq, ids, qids, meta, qmeta, sp,
                         cand, cand_count, cand_cap, split_count, elements);
  }
}
int index_query_dense_ranges(int64_t entries) { return (int)((entries + (1 << DQ_RANGE_LOG) - 1) >> DQ_RANGE_LOG); }

}  // namespace mhap
