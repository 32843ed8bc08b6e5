// graph_kernels.hip — the string graph of the realigned overlaps (mhap_graph_begin / _add / _finish / _copy_* / _free), its unitigs
// (mhap_graph_unitigs / _copy_unitigs / _copy_layout / _copy_links / _spell; the kernels' list is in front of them), the cleaning of
// the graph in rounds (mhap_graph_clean / _copy_dropped / _copy_removed; its kernels' list is in front of them too) and the GFA link lines.  The contract — the class of a record, the arcs of a dovetail, contained reads, the arc list, the reduction and the final
// arcs — is the prose of include/mhap_hip.h ("string graph"); tests/string_graph_ref.py restates it.
//
// add: the host finds every record's two reads (and refuses the call before anything is queued), packs the record into 32 bytes and
// queues one upload and classify_kernel, one lane per record: the class, the contained flags (atomicOr) and the dovetail's two arcs,
// which are written over the record's own 32 bytes — slots 2 q and 2 q + 1 of the add's chunk, u = -1 where there is no arc.  Nothing
// waits: the packed records stay on the host until an event behind the kernel has passed, which later calls look at.
//
// finish: the list is built from the chunks as they are, so it may be repeated and records may follow it.
//   count_kernel     surviving arcs (neither read contained) per u                         -> scan_kernel -> the segments of `tmp`
//   scatter_kernel   the surviving arcs into their segments, in any order
//   dedup_kernel     one wave per u: an arc is kept when no arc of its (u, v) precedes it in (len, slot) -> scan -> the final segments
//   place_kernel     one wave per u: a kept arc's place is the number of kept arcs before it in (len, v), counted; its place in the
//                    by-target order (bt_v ascending, bt_pos = the place in list order) is counted the same way
//   reduce_kernel    one wave per v: the outer loop over w_i is sequential, the lanes take w_i's arcs 64 at a time; the mark of a target
//                    x of v is found by a binary search of v's by-target order, so there is no table and no capacity
//   finish_kernel    one lane per arc: the complement through the same search, the row, the counts
// Counting is exact for any degree and quadratic in it; the degrees of an overlap graph are a few times the coverage.
#include <hip/hip_runtime.h>

#include <deque>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "graph_class.hpp"
#include "mhap_internal.hpp"
#include "read_table.hpp"

namespace mhap {
namespace {

// counts: records, the six classes, contained reads, arcs, reduced, final
enum { GC_RECORDS = 0, GC_CLASS0 = 1, GC_CONTAINED = 7, GC_ARCS = 8, GC_REDUCED = 9, GC_FINAL = 10 };

// (GItem, the record as it goes up, the class codes and the parameters are graph_class.hpp's)
struct GArc { int32_t u, v, len, q; };   // two of them over a GItem; u = -1: no arc
static_assert(sizeof(GArc) == 16, "an item is two arcs");

__global__ __launch_bounds__(256) void classify_kernel(int4* __restrict__ items, int64_t n, int32_t q0, const int32_t* __restrict__ lengths,
                                                       GParams P, uint8_t* __restrict__ cls, uint32_t* __restrict__ contained,
                                                       unsigned long long* __restrict__ counts) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int c = -1;
  if (q < n) {
    const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
    const int32_t A = w0.x, B = w0.y >> 1, o = w0.y & 1;
    const double score = __hiloint2double(w1.w, w1.z);
    GArc e0{-1, 0, 0, 0}, e1{-1, 0, 0, 0};
    GGeom g;
    c = graph_class(A, B, o, w0.z, w0.w, w1.x, w1.y, score, lengths[A], lengths[B], P, g);
    if (c == G_A_CONTAINED) atomicOr(contained + A, 1u);
    else if (c == G_B_CONTAINED) atomicOr(contained + B, 1u);
    else if (c == G_DOVETAIL) {
      const int32_t lab = q0 + (int32_t)q;
      if (g.qs > g.tl5) { e0 = GArc{2 * A, 2 * B + o, g.qs - g.tl5, lab}; e1 = GArc{2 * B + (1 - o), 2 * A + 1, g.tl3 - g.q3, lab}; }
      else { e0 = GArc{2 * B + o, 2 * A, g.tl5 - g.qs, lab}; e1 = GArc{2 * A + 1, 2 * B + (1 - o), g.q3 - g.tl3, lab}; }
    }
    items[2 * q] = make_int4(e0.u, e0.v, e0.len, e0.q);
    items[2 * q + 1] = make_int4(e1.u, e1.v, e1.len, e1.q);
    cls[q] = (uint8_t)c;
  }
  for (int k = 0; k < G_CLASSES; k++) {   // one add per wave and class
    const unsigned long long m = __ballot(c == k);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + GC_CLASS0 + k, (unsigned long long)__popcll(m));
  }
}

__device__ inline bool survives(const GArc& a, const uint32_t* __restrict__ contained) {
  return a.u >= 0 && !contained[a.u >> 1] && !contained[a.v >> 1];
}

__global__ __launch_bounds__(256) void count_kernel(const GArc* __restrict__ arcs, int64_t n, const uint32_t* __restrict__ contained,
                                                    int32_t* __restrict__ deg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const GArc a = arcs[i];
  if (survives(a, contained)) atomicAdd(deg + a.u, 1);
}

__global__ __launch_bounds__(256) void scatter_kernel(const GArc* __restrict__ arcs, int64_t n, const uint32_t* __restrict__ contained,
                                                      const int64_t* __restrict__ start, int32_t* __restrict__ fill, GArc* __restrict__ tmp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const GArc a = arcs[i];
  if (survives(a, contained)) tmp[start[a.u] + atomicAdd(fill + a.u, 1)] = a;
}

// one wave per u over its segment of tmp: keep[a] = no arc of the same v precedes a in (len, slot); kdeg[u] = the arcs kept
__global__ __launch_bounds__(64) void dedup_kernel(const GArc* __restrict__ tmp, const int64_t* __restrict__ start, uint8_t* __restrict__ keep,
                                                   int32_t* __restrict__ kdeg) {
  const int64_t u = blockIdx.x, s = start[u], e = start[u + 1];
  const int lane = threadIdx.x;
  int kept = 0;
  for (int64_t a0 = s; a0 < e; a0 += 64) {
    const int64_t a = a0 + lane;
    bool k = a < e;
    if (k) {
      const GArc x = tmp[a];
      for (int64_t b = s; b < e && k; b++) {
        const GArc y = tmp[b];
        if (y.v == x.v && (y.len < x.len || (y.len == x.len && b < a))) k = false;
      }
      keep[a] = k ? 1 : 0;
    }
    kept += __popcll(__ballot(k));
  }
  if (lane == 0) kdeg[u] = kept;
}

// one wave per u: the kept arcs to their places in (len, v) order, and the by-target order of the segment
__global__ __launch_bounds__(64) void place_kernel(const GArc* __restrict__ tmp, const uint8_t* __restrict__ keep, const int64_t* __restrict__ start,
                                                   const int64_t* __restrict__ fstart, int32_t* __restrict__ U, int32_t* __restrict__ V,
                                                   int32_t* __restrict__ LEN, int32_t* __restrict__ Q, int32_t* __restrict__ bt_v,
                                                   int32_t* __restrict__ bt_pos) {
  const int64_t u = blockIdx.x, s = start[u], e = start[u + 1], f = fstart[u];
  for (int64_t a = s + threadIdx.x; a < e; a += 64) {
    if (!keep[a]) continue;
    const GArc x = tmp[a];
    int32_t rank = 0, trank = 0;   // (kept arcs of one u have different v)
    for (int64_t b = s; b < e; b++) {
      if (!keep[b]) continue;
      const GArc y = tmp[b];
      rank += (y.len < x.len || (y.len == x.len && y.v < x.v)) ? 1 : 0;
      trank += y.v < x.v ? 1 : 0;
    }
    U[f + rank] = (int32_t)u; V[f + rank] = x.v; LEN[f + rank] = x.len; Q[f + rank] = x.q;
    bt_v[f + trank] = x.v; bt_pos[f + trank] = rank;
  }
}

// the list index of the arc v -> x, v's segment being [f0, f1); -1 when there is none
__device__ inline int64_t find_arc(const int32_t* __restrict__ bt_v, const int32_t* __restrict__ bt_pos, int64_t f0, int64_t f1, int32_t x) {
  int64_t lo = f0, hi = f1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (bt_v[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (lo < f1 && bt_v[lo] == x) ? f0 + bt_pos[lo] : -1;
}

// one wave per vertex v; mark[i] != 0: the target of arc i is ELIMINATED (zeroed before the launch: every target IN_PLAY)
__global__ __launch_bounds__(64) void reduce_kernel(const int64_t* __restrict__ fstart, const int32_t* __restrict__ V, const int32_t* __restrict__ LEN,
                                                    const int32_t* __restrict__ bt_v, const int32_t* __restrict__ bt_pos, int32_t fuzz,
                                                    int32_t* mark) {
  const int64_t v = blockIdx.x, f0 = fstart[v], f1 = fstart[v + 1];
  if (f0 == f1) return;
  const int lane = threadIdx.x;
  const int64_t longest = (int64_t)LEN[f1 - 1] + fuzz;
  for (int64_t i = f0; i < f1; i++) {   // pass 1: sequential, a step sees the marks of the steps before it
    __syncthreads();
    // (the marks are set by atomics, which are done in L2: the load goes there too, not to a line this CU may hold)
    if (__hip_atomic_load(mark + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) continue;
    const int64_t lw = LEN[i], ws = fstart[V[i]], we = fstart[V[i] + 1];
    for (int64_t k0 = ws; k0 < we; k0 += 64) {
      const int64_t k = k0 + lane;
      const bool in = k < we && lw + LEN[k] <= longest;   // lengths ascend within a segment: once false, false for the rest
      if (in) {
        const int64_t j = find_arc(bt_v, bt_pos, f0, f1, V[k]);
        if (j >= 0) atomicOr(mark + j, 1);
      }
      if (__any(!in)) break;
    }
  }
  __syncthreads();
  for (int64_t i = f0; i < f1; i++) {   // pass 2: whatever the marks, so in any order
    const int64_t ws = fstart[V[i]], we = fstart[V[i] + 1];
    for (int64_t k0 = ws; k0 < we; k0 += 64) {
      const int64_t k = k0 + lane;
      const bool in = k < we && (k == ws || LEN[k] < fuzz);
      if (in) {
        const int64_t j = find_arc(bt_v, bt_pos, f0, f1, V[k]);
        if (j >= 0) atomicOr(mark + j, 1);
      }
      if (__any(!in)) break;
    }
  }
}

// one lane per arc: its row {u, v, len, ol, q, reduced, final}
__global__ __launch_bounds__(256) void finish_kernel(int64_t n, const int64_t* __restrict__ fstart, const int32_t* __restrict__ U,
                                                     const int32_t* __restrict__ V, const int32_t* __restrict__ LEN, const int32_t* __restrict__ Q,
                                                     const int32_t* __restrict__ bt_v, const int32_t* __restrict__ bt_pos,
                                                     const int32_t* __restrict__ mark, const int32_t* __restrict__ lengths,
                                                     int32_t* __restrict__ rows, unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool red = false, fin = false;
  if (i < n) {
    const int32_t u = U[i], v = V[i], len = LEN[i];
    const int64_t j = find_arc(bt_v, bt_pos, fstart[v ^ 1], fstart[(v ^ 1) + 1], u ^ 1);
    red = mark[i] != 0;
    fin = !red && j >= 0 && mark[j] == 0;
    int32_t* r = rows + 7 * i;
    r[0] = u; r[1] = v; r[2] = len; r[3] = lengths[u >> 1] - len; r[4] = Q[i]; r[5] = red ? 1 : 0; r[6] = fin ? 1 : 0;
  }
  const unsigned long long mr = __ballot(red), mf = __ballot(fin);
  if ((threadIdx.x & 63) == 0) {
    if (mr) atomicAdd(counts + GC_REDUCED, (unsigned long long)__popcll(mr));
    if (mf) atomicAdd(counts + GC_FINAL, (unsigned long long)__popcll(mf));
  }
}

__global__ __launch_bounds__(256) void flags_kernel(const uint32_t* __restrict__ contained, int64_t n, unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long m = __ballot(i < n && contained[i] != 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + GC_CONTAINED, (unsigned long long)__popcll(m));
}

// ---- unitigs ("unitigs" in the string-graph section of include/mhap_hip.h; tests/unitig_ref.py restates it) -------------------------
//   outdeg_kernel    one lane per vertex over its segment of the list: the final arcs, and the target and index of the only one
//   next_kernel      one lane per vertex: next, span, and prev of the target (which has one arc in, so one writer)
//   rank_init / rank_round   pointer doubling towards the head: (pointer, members, bases) between a vertex and the vertex it points at;
//                    a head points at itself with (0, 0), so it is a fixed point and every round reads one buffer and writes the other
//   cyc_init / min_round     a vertex whose pointer has not reached a head is on a cycle; the same doubling carries the smallest vertex
//                    of the 2^k vertices that end at it; cut_init makes that vertex a head and the rank rounds run once more
//   tails_kernel     the last member tells its head the tail, the members and the bases;  select_kernel keeps a head by the rule
//   three scans      the unitig's number, its first member, its first base;  *_scatter: the tables in their canonical places
//   linkflag_kernel -> scan -> link_scatter: the final arcs that are not joined, in list order
//   spell_kernel     one workgroup per SPELL_CHUNK bytes of the output, 16 per lane, found in the members by binary search: two lanes
//                    search all members for the tile's ends, every lane then searches between them
enum { UC_CIRCULAR = 0, UC_JOINED = 1, UC_LONGEST = 2, UC_DEVICE = 3 };
enum { SPELL_CHUNK = MHAP_SPELL_CHUNK, SPELL_T = SPELL_CHUNK / 16 };

// The masks of a build.  `dropped` (one byte per read) and `removed` (one byte per arc) are the state of the graph cleaning: with
// MASKED a vertex is in play when its read is neither contained nor dropped and an arc counts when it is final and not removed;
// without, the two pointers are not read and the kernels are those of the uncleaned unitigs.
template <bool MASKED>
__device__ inline bool counted(const int32_t* __restrict__ rows, const uint8_t* __restrict__ removed, int64_t i) {
  if (MASKED) return rows[7 * i + 6] != 0 && removed[i] == 0;
  return rows[7 * i + 6] != 0;
}

template <bool MASKED>
__global__ __launch_bounds__(256) void outdeg_kernel(int64_t nv, const int64_t* __restrict__ fstart, const int32_t* __restrict__ V,
                                                     const int32_t* __restrict__ rows, const uint8_t* __restrict__ removed,
                                                     int32_t* __restrict__ fout, int32_t* __restrict__ cand, int32_t* __restrict__ carc) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  int32_t n = 0, c = -1, a = -1;
  for (int64_t i = fstart[v], e = fstart[v + 1]; i < e; i++)
    if (counted<MASKED>(rows, removed, i)) { n++; c = V[i]; a = (int32_t)i; }
  fout[v] = n; cand[v] = c; carc[v] = a;
}

// prev is -1 everywhere before the launch
__global__ __launch_bounds__(256) void next_kernel(int64_t nv, const int32_t* __restrict__ fout, const int32_t* __restrict__ cand,
                                                   const int32_t* __restrict__ carc, const int32_t* __restrict__ LEN,
                                                   const int32_t* __restrict__ lengths, int32_t* __restrict__ next, int32_t* __restrict__ prev,
                                                   int32_t* __restrict__ span, unsigned long long* __restrict__ ucounts) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool joined = false;
  if (v < nv) {
    int32_t w = -1, sp = lengths[v >> 1];
    if (fout[v] == 1) {
      const int32_t c = cand[v];
      if (fout[c ^ 1] == 1) { w = c; sp = LEN[carc[v]]; prev[c] = (int32_t)v; joined = true; }   // (c has one arc in: this one)
    }
    next[v] = w; span[v] = sp;
  }
  const unsigned long long m = __ballot(joined);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ucounts + UC_JOINED, (unsigned long long)__popcll(m));
}

// P < 0: the vertex of a contained or dropped read, which is in no unitig
template <bool MASKED>
__global__ __launch_bounds__(256) void rank_init_kernel(int64_t nv, const uint32_t* __restrict__ contained, const uint8_t* __restrict__ dropped,
                                                        const int32_t* __restrict__ prev,
                                                        const int32_t* __restrict__ span, int32_t* __restrict__ P, uint32_t* __restrict__ R,
                                                        unsigned long long* __restrict__ O) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t p = prev[v];
  if (contained[v >> 1] || (MASKED && dropped[v >> 1])) { P[v] = -1; R[v] = 0; O[v] = 0; }
  else if (p < 0) { P[v] = (int32_t)v; R[v] = 0; O[v] = 0; }
  else { P[v] = p; R[v] = 1; O[v] = (unsigned long long)span[p]; }
}

// (on a cycle the sums mean nothing and may wrap, which is why they are unsigned; cut_init starts them again)
__global__ __launch_bounds__(256) void rank_round_kernel(int64_t nv, const int32_t* __restrict__ Pi, const uint32_t* __restrict__ Ri,
                                                         const unsigned long long* __restrict__ Oi, int32_t* __restrict__ Po,
                                                         uint32_t* __restrict__ Ro, unsigned long long* __restrict__ Oo) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t p = Pi[v];
  if (p < 0) { Po[v] = -1; Ro[v] = 0; Oo[v] = 0; return; }
  Po[v] = Pi[p]; Ro[v] = Ri[v] + Ri[p]; Oo[v] = Oi[v] + Oi[p];
}

__global__ __launch_bounds__(256) void cyc_init_kernel(int64_t nv, const int32_t* __restrict__ P, const int32_t* __restrict__ prev,
                                                       uint8_t* __restrict__ cyc, int32_t* __restrict__ Q, int32_t* __restrict__ M) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t p = P[v];
  const bool c = p >= 0 && prev[p] >= 0;   // after the rounds a chain's vertex points at its head, which has no prev
  cyc[v] = c ? 1 : 0; Q[v] = c ? prev[v] : -1; M[v] = (int32_t)v;
}

__global__ __launch_bounds__(256) void min_round_kernel(int64_t nv, const uint8_t* __restrict__ cyc, const int32_t* __restrict__ Qi,
                                                        const int32_t* __restrict__ Mi, int32_t* __restrict__ Qo, int32_t* __restrict__ Mo) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  if (!cyc[v]) { Qo[v] = -1; Mo[v] = Mi[v]; return; }
  const int32_t q = Qi[v];
  Qo[v] = Qi[q]; Mo[v] = min(Mi[v], Mi[q]);
}

// the cycle is cut in front of its smallest vertex; a lane writes its own entries only
__global__ __launch_bounds__(256) void cut_init_kernel(int64_t nv, const uint8_t* __restrict__ cyc, const int32_t* __restrict__ M,
                                                       const int32_t* __restrict__ prev, const int32_t* __restrict__ span, int32_t* __restrict__ P,
                                                       uint32_t* __restrict__ R, unsigned long long* __restrict__ O) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv || !cyc[v]) return;
  const int32_t p = prev[v];
  if (M[v] == (int32_t)v) { P[v] = (int32_t)v; R[v] = 0; O[v] = 0; }
  else { P[v] = p; R[v] = 1; O[v] = (unsigned long long)span[p]; }
}

// cnt and ulen are 0 everywhere before the launch; a chain has one last member, so a head has one writer
__global__ __launch_bounds__(256) void tails_kernel(int64_t nv, const int32_t* __restrict__ P, const uint32_t* __restrict__ R,
                                                    const unsigned long long* __restrict__ O, const int32_t* __restrict__ next,
                                                    const int32_t* __restrict__ span, const uint8_t* __restrict__ cyc, const int32_t* __restrict__ M,
                                                    int32_t* __restrict__ tail, int32_t* __restrict__ cnt, int64_t* __restrict__ ulen) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t h = P[v];
  if (h < 0) return;
  if (next[v] < 0 || (cyc[v] && next[v] == M[v])) { tail[h] = (int32_t)v; cnt[h] = (int32_t)(R[v] + 1); ulen[h] = (int64_t)(O[v] + (unsigned long long)span[v]); }
}

__global__ __launch_bounds__(256) void select_kernel(int64_t nv, const int32_t* __restrict__ P, const uint8_t* __restrict__ cyc,
                                                     const int32_t* __restrict__ M, const int32_t* __restrict__ tail, int32_t* __restrict__ kept,
                                                     int32_t* __restrict__ cnt, int64_t* __restrict__ ulen, unsigned long long* __restrict__ ucounts) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool k = false, circ = false;
  if (v < nv) {
    if (P[v] == (int32_t)v) {
      circ = cyc[v] != 0;
      k = circ ? M[v] < M[v ^ 1] : (int32_t)v < (tail[v] ^ 1);
      if (!k) { cnt[v] = 0; ulen[v] = 0; }
      else atomicMax(ucounts + UC_LONGEST, (unsigned long long)ulen[v]);
    }
    kept[v] = k ? 1 : 0;
  }
  const unsigned long long m = __ballot(k && circ);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(ucounts + UC_CIRCULAR, (unsigned long long)__popcll(m));
}

template <bool MASKED>
__global__ __launch_bounds__(256) void linkflag_kernel(int64_t n, const int32_t* __restrict__ rows, const uint8_t* __restrict__ removed,
                                                       const int32_t* __restrict__ next, int32_t* __restrict__ islink) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t* r = rows + 7 * i;
  islink[i] = (counted<MASKED>(rows, removed, i) && next[r[0]] != r[1]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void unitig_scatter_kernel(int64_t nv, const int32_t* __restrict__ kept, const int64_t* __restrict__ unum,
                                                             const int64_t* __restrict__ mstart, const int64_t* __restrict__ ulen,
                                                             const uint8_t* __restrict__ cyc, int64_t* __restrict__ u_start,
                                                             int64_t* __restrict__ u_len, uint8_t* __restrict__ u_circ) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv || !kept[v]) return;
  const int64_t k = unum[v];
  u_start[k] = mstart[v]; u_len[k] = ulen[v]; u_circ[k] = cyc[v];
}

__global__ __launch_bounds__(256) void member_scatter_kernel(int64_t nv, const int32_t* __restrict__ P, const uint32_t* __restrict__ R,
                                                             const unsigned long long* __restrict__ O, const int32_t* __restrict__ span,
                                                             const int32_t* __restrict__ kept, const int64_t* __restrict__ mstart,
                                                             const int64_t* __restrict__ bstart, int32_t* __restrict__ m_vertex,
                                                             int64_t* __restrict__ m_offset, int32_t* __restrict__ m_span, int64_t* __restrict__ m_dst) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
  const int32_t h = P[v];
  if (h < 0 || !kept[h]) return;
  const int64_t at = mstart[h] + R[v];
  m_vertex[at] = (int32_t)v; m_offset[at] = (int64_t)O[v]; m_span[at] = span[v]; m_dst[at] = bstart[h] + (int64_t)O[v];
}

// a link leaves the tail of a unitig or of a twin and enters the head of one: the chain of u or of u ^ 1 is the kept one
__global__ __launch_bounds__(256) void link_scatter_kernel(int64_t n, const int32_t* __restrict__ rows, const int32_t* __restrict__ islink,
                                                           const int64_t* __restrict__ lstart, const int32_t* __restrict__ P,
                                                           const int32_t* __restrict__ kept, const int64_t* __restrict__ unum,
                                                           int32_t* __restrict__ links) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !islink[i]) return;
  const int32_t* r = rows + 7 * i;
  int32_t* o = links + 6 * lstart[i];
  for (int e = 0; e < 2; e++) {
    const int32_t x = r[e], h = P[x];
    const bool own = kept[h] != 0;
    o[2 * e] = (int32_t)unum[own ? h : P[x ^ 1]];
    o[2 * e + 1] = own ? 0 : 1;
  }
  o[4] = r[3]; o[5] = (int32_t)i;
}

__device__ inline uint32_t rc_word(uint32_t x, const uint8_t* tab) {   // the four bytes reversed and complemented
  return (uint32_t)tab[x >> 24] | ((uint32_t)tab[(x >> 16) & 255] << 8) | ((uint32_t)tab[(x >> 8) & 255] << 16) | ((uint32_t)tab[x & 255] << 24);
}

// One lane per 16 bytes of the output, which begins on a 16-byte boundary.  Where the 16 bytes come from one member and the words
// around their source lie inside `bases`, they are loaded as aligned words, shifted into place and stored as one uint4; otherwise
// (a member boundary, the last bytes of the output, the ends of `bases`) they are gathered byte by byte.  Every byte has one writer.
__global__ __launch_bounds__(SPELL_T) void spell_kernel(const uint8_t* __restrict__ bases, int64_t n_bases, const int64_t* __restrict__ roff,
                                                        const int32_t* __restrict__ lengths, int64_t n_members,
                                                        const int32_t* __restrict__ m_vertex, const int32_t* __restrict__ m_span,
                                                        const int64_t* __restrict__ m_dst, int64_t total, uint8_t* __restrict__ out) {
  __shared__ uint8_t tab[256];
  static_assert(SPELL_T == 256, "one lane per entry of the table");
  __shared__ int64_t edge[2];   // the members that begin at or before the tile's first byte, and at or before its last
  tab[threadIdx.x] = (uint8_t)rc_char(threadIdx.x);
  const int64_t tile0 = (int64_t)blockIdx.x * SPELL_CHUNK;
  if (threadIdx.x < 2) {
    const int64_t b = threadIdx.x == 0 ? tile0 : min(tile0 + SPELL_CHUNK, total) - 1;
    int64_t lo = 0, hi = n_members;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (m_dst[mid] <= b) lo = mid + 1; else hi = mid;
    }
    edge[threadIdx.x] = lo;
  }
  __syncthreads();
  const int64_t b0 = tile0 + 16 * (int64_t)threadIdx.x;
  if (b0 >= total) return;
  const int nb = (int)min((int64_t)16, total - b0);
  int64_t lo = edge[0], hi = edge[1];   // the last member that begins at or before b0 (members of span 0 before it begin there too)
  while (lo < hi) {                     // (a tile lies in a few members: a step or two)
    const int64_t mid = (lo + hi) >> 1;
    if (m_dst[mid] <= b0) lo = mid + 1; else hi = mid;
  }
  int64_t at = lo - 1;
  int32_t v = m_vertex[at], sp = m_span[at], L = lengths[v >> 1];
  int64_t off = roff[v >> 1], j = b0 - m_dst[at];
  uint32_t w[4] = {0, 0, 0, 0};
  bool done = false;
  if (nb == 16 && j + 16 <= sp) {
    const int64_t s = (v & 1) ? off + L - 16 - j : off + j;
    const uint8_t* a = bases + s;
    const unsigned mis = (unsigned)((uintptr_t)a & 3);
    if (mis == 0) {
      const uint32_t* p = (const uint32_t*)a;
      w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; w[3] = p[3];
      done = true;
    } else if (s >= (int64_t)mis && s - mis + 20 <= n_bases) {
      const uint32_t* p = (const uint32_t*)(a - mis);
      const uint32_t x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3], x4 = p[4];
      const unsigned sh = 8 * mis;
      w[0] = (x0 >> sh) | (x1 << (32 - sh)); w[1] = (x1 >> sh) | (x2 << (32 - sh));
      w[2] = (x2 >> sh) | (x3 << (32 - sh)); w[3] = (x3 >> sh) | (x4 << (32 - sh));
      done = true;
    }
    if (done && (v & 1)) {
      const uint32_t t0 = rc_word(w[3], tab), t1 = rc_word(w[2], tab), t2 = rc_word(w[1], tab), t3 = rc_word(w[0], tab);
      w[0] = t0; w[1] = t1; w[2] = t2; w[3] = t3;
    }
  }
  if (!done) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
      if (t < nb) {
        while (j >= sp && at + 1 < n_members) {   // (b0 + t < total: a member with this byte follows)
          at++;
          v = m_vertex[at]; sp = m_span[at]; L = lengths[v >> 1]; off = roff[v >> 1]; j = 0;
        }
        const uint32_t c = (v & 1) ? (uint32_t)tab[bases[off + L - 1 - j]] : (uint32_t)bases[off + j];
        w[t >> 2] |= c << (8 * (t & 3));
        j++;
      }
    }
  }
  if (nb == 16) *(uint4*)(out + b0) = make_uint4(w[0], w[1], w[2], w[3]);
  else
    for (int t = 0; t < nb; t++) out[b0 + t] = (uint8_t)(w[t >> 2] >> (8 * (t & 3)));
}

// ---- graph cleaning ("graph cleaning" in the string-graph section of include/mhap_hip.h; tests/graph_clean_ref.py restates it) -----
// A round builds the unitigs of the graph as it stands (the kernels above, with the dropped and removed bytes as masks, into tables
// of their largest possible sizes, so that nothing waits for a size) and decides on that snapshot.  x = 2 X + o is an oriented unitig.
//   origin_kernel    one lane per x: the rows of the link table that leave x.  The table is in arc-list order and an oriented unitig
//                    has one tail vertex, so they are the rows whose arc lies in that vertex's segment: two binary searches
//   degree_kernel    one lane per x: out-degree = its rows, in-degree = the rows of x ^ 1 (every link's complement is in the table),
//                    and the tip-candidate flag
//   tip_kernel       one lane per unitig: the candidate's out-links, and for each target its in-links, looking for a holder
//   bubble_kernel    one lane per unitig: its S and E, then S's out-links for a better sibling between the same two
//   drop_kernel      one lane per member: finds its unitig by binary search and, where that is removed, writes its own read
//   removed_kernel   one lane per arc
// A lane decides from the snapshot only and writes its own element only.  The loops over links are lane-serial: a unitig end has as
// many links as its read keeps final arcs after the reduction, one to a handful at any coverage, and the loops are exact for any
// number of them (a star of hundreds of tips costs the lanes at its centre that many steps, no more).
enum { CC_ROUNDS = 0, CC_TIPS, CC_TIP_READS, CC_BUBBLES, CC_BUBBLE_READS, CC_ARCS };

struct UTables {   // the unitigs of a round where the kernels find them; the sizes stay on the device
  const int64_t *nu, *nm, *nl;
  const int64_t *u_start, *u_len;
  const uint8_t* u_circ;
  const int32_t *m_vertex, *links;
};

__device__ inline int64_t members_of(const UTables& U, int64_t X) { return (X + 1 < *U.nu ? U.u_start[X + 1] : *U.nm) - U.u_start[X]; }

// rank(A) > rank(B) for two different unitigs: (members, bases, -number)
__device__ inline bool outranks(const UTables& U, int64_t A, int64_t B) {
  const int64_t ma = members_of(U, A), mb = members_of(U, B);
  if (ma != mb) return ma > mb;
  if (U.u_len[A] != U.u_len[B]) return U.u_len[A] > U.u_len[B];
  return A < B;
}

// the first link row whose arc is >= a
__device__ inline int32_t first_link_from(const int32_t* __restrict__ links, int64_t nl, int64_t a) {
  int64_t lo = 0, hi = nl;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (links[6 * mid + 5] < a) lo = mid + 1; else hi = mid;
  }
  return (int32_t)lo;
}

__global__ __launch_bounds__(256) void origin_kernel(UTables U, const int64_t* __restrict__ fstart, int32_t* __restrict__ lo,
                                                     int32_t* __restrict__ hi) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, X = x >> 1;
  if (X >= *U.nu) return;
  int32_t a = 0, b = 0;
  if (!U.u_circ[X]) {
    const int32_t t = (x & 1) ? (U.m_vertex[U.u_start[X]] ^ 1) : U.m_vertex[U.u_start[X] + members_of(U, X) - 1];
    a = first_link_from(U.links, *U.nl, fstart[t]);
    b = first_link_from(U.links, *U.nl, fstart[t + 1]);
  }
  lo[x] = a; hi[x] = b;
}

__global__ __launch_bounds__(256) void degree_kernel(UTables U, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                     int32_t tip_reads, uint8_t* __restrict__ cand) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x, X = x >> 1;
  if (X >= *U.nu) return;
  const int32_t out = hi[x] - lo[x], in = hi[x ^ 1] - lo[x ^ 1];
  cand[x] = (!U.u_circ[X] && members_of(U, X) <= tip_reads && in == 0 && out >= 1) ? 1 : 0;
}

__global__ __launch_bounds__(256) void tip_kernel(UTables U, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                  const uint8_t* __restrict__ cand, uint8_t* __restrict__ verdict,
                                                  unsigned long long* __restrict__ counts) {
  const int64_t T = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool tip = false;
  if (T < *U.nu) {
    const int o = cand[2 * T] ? 0 : cand[2 * T + 1] ? 1 : -1;   // (a candidate in at most one orientation)
    tip = o >= 0;
    for (int32_t l = tip ? lo[2 * T + o] : 0, le = tip ? hi[2 * T + o] : 0; l < le && tip; l++) {
      const int64_t y = 2 * (int64_t)U.links[6 * l + 2] + U.links[6 * l + 3];
      bool held = false;   // the in-links of y are the out-links of y ^ 1: a row (y ^ 1) -> (W, 1 - w) is the in-link from (W, w)
      for (int32_t m = lo[y ^ 1], me = hi[y ^ 1]; m < me && !held; m++) {
        const int64_t W = U.links[6 * m + 2], w = 1 - U.links[6 * m + 3];
        held = W != T && (!cand[2 * W + w] || outranks(U, W, T));
      }
      tip = held;
    }
    verdict[T] = tip ? 1 : 0;
  }
  const unsigned long long m = __ballot(tip);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + CC_TIPS, (unsigned long long)__popcll(m));
}

// x is a branch between S and E: one link in, one out, short enough; returns E (-1: no branch) and sets S
__device__ inline int64_t branch_ends(const UTables& U, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int32_t bubble_bases,
                                      int64_t x, int64_t* S) {
  const int64_t B = x >> 1;
  if (U.u_circ[B] || U.u_len[B] > bubble_bases || hi[x] - lo[x] != 1 || hi[x ^ 1] - lo[x ^ 1] != 1) return -1;
  const int32_t* out = U.links + 6 * (int64_t)lo[x];
  const int32_t* in = U.links + 6 * (int64_t)lo[x ^ 1];
  const int64_t E = 2 * (int64_t)out[2] + out[3], s = 2 * (int64_t)in[2] + (1 - in[3]);
  if ((E >> 1) == B || (s >> 1) == B) return -1;
  *S = s;
  return E;
}

// (runs behind tip_kernel, which has written every verdict; a tip has no link in and a branch has one, so no unitig is both)
__global__ __launch_bounds__(256) void bubble_kernel(UTables U, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                     int32_t bubble_bases, uint8_t* __restrict__ verdict, unsigned long long* __restrict__ counts) {
  const int64_t B = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool pop = false;
  if (B < *U.nu) {
    int64_t S = 0, S2 = 0;
    const int64_t E = branch_ends(U, lo, hi, bubble_bases, 2 * B, &S);   // (seen from the twin the verdict is the same: one side is enough)
    if (E >= 0)
      for (int32_t m = lo[S], me = hi[S]; m < me && !pop; m++) {
        const int64_t y = 2 * (int64_t)U.links[6 * m + 2] + U.links[6 * m + 3];
        pop = (y >> 1) != B && branch_ends(U, lo, hi, bubble_bases, y, &S2) == E && S2 == S && outranks(U, y >> 1, B);
      }
    if (pop) verdict[B] = 2;
  }
  const unsigned long long m = __ballot(pop);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + CC_BUBBLES, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void drop_kernel(UTables U, const uint8_t* __restrict__ verdict, uint8_t* __restrict__ dropped,
                                                   unsigned long long* __restrict__ counts) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int what = 0;
  if (m < *U.nm) {
    int64_t lo = 0, hi = *U.nu;   // the last unitig that begins at or before m
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (U.u_start[mid] <= m) lo = mid + 1; else hi = mid;
    }
    what = verdict[lo - 1];
    if (what) dropped[U.m_vertex[m] >> 1] = (uint8_t)what;
  }
  const unsigned long long t = __ballot(what == 1), b = __ballot(what == 2);
  if ((threadIdx.x & 63) == 0) {
    if (t) atomicAdd(counts + CC_TIP_READS, (unsigned long long)__popcll(t));
    if (b) atomicAdd(counts + CC_BUBBLE_READS, (unsigned long long)__popcll(b));
  }
}

// removed[i] = the arc is final and one of its reads is dropped; the count takes the arcs that were not removed before
__global__ __launch_bounds__(256) void removed_kernel(int64_t n, const int32_t* __restrict__ rows, const uint8_t* __restrict__ dropped,
                                                      uint8_t* __restrict__ removed, unsigned long long* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool fresh = false;
  if (i < n) {
    const int32_t* r = rows + 7 * i;
    const bool gone = r[6] && (dropped[r[0] >> 1] || dropped[r[1] >> 1]);
    fresh = gone && !removed[i];
    removed[i] = gone ? 1 : 0;
  }
  const unsigned long long m = __ballot(fresh);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + CC_ARCS, (unsigned long long)__popcll(m));
}

}  // namespace
}  // namespace mhap

using namespace mhap;

// The table of reads, the lookup of a record's reads and the queued uploads are read_table.hpp's ReadTable.  An add keeps a chunk of its
// own (the records stay on the device until the session goes), so the table's one `items` buffer, and with it queue_add / commit_add,
// are not used here.
struct mhap_graph_session : ReadTable {
  GParams P{};
  int64_t n_arcs = -1;                                    // n_arcs < 0: no finish yet
  struct Chunk { DevBuf items, cls; int64_t n = 0; };     // items: the add's records, then its arc slots
  std::deque<Chunk> chunks;
  DevBuf contained, counts;                               // counts: MHAP_GRAPH_COUNTS x uint64, the classes summed over the adds
  DevBuf deg, fill, start, fstart, tmp, keep, U, V, LEN, Q, bt_v, bt_pos, mark, rows;
  // unitigs: rebuilt by every mhap_graph_unitigs, invalid (n_unitigs < 0) from the next finish on
  int64_t n_contained = 0, finish_records = 0, n_unitigs = -1, n_members = 0, n_links = 0, n_ubases = 0;
  DevBuf fout, cand, carc, unext, uprev, uspan, uP[2], uR[2], uO[2], uQ[2], uM[2], cyc, tail, cnt, ulen, kept, unum, mstart, bstart, islink, lstart,
      ucounts, u_start, u_len, u_circ, m_vertex, m_offset, m_span, m_dst, links, d_roff, d_bases, spelled;
  int64_t last_counts[MHAP_UNITIG_COUNTS] = {0};          // the counts of the unitigs now served
  int u_cur = 0;                                          // which of uP / uR / uO the last build's ranks ended in
  // cleaning: the dropped and removed bytes hold from a mhap_graph_clean to the next finish
  bool cleaned = false;
  uint64_t unitig_gen = 0;                                // bumped whenever the served unitigs go or change: a consensus session's key
  DevBuf dropped, removed, ccounts, o_lo, o_hi, o_cand, verdict;
  void release() {
    release_table();
    for (auto& c : chunks) { c.items.release(); c.cls.release(); }
    chunks.clear();
    for (DevBuf* b : {&contained, &counts, &deg, &fill, &start, &fstart, &tmp, &keep, &U, &V, &LEN, &Q, &bt_v, &bt_pos, &mark, &rows,
                       &fout, &cand, &carc, &unext, &uprev, &uspan, &uP[0], &uP[1], &uR[0], &uR[1], &uO[0], &uO[1], &uQ[0], &uQ[1], &uM[0], &uM[1], &cyc,
                       &tail, &cnt, &ulen, &kept, &unum, &mstart, &bstart, &islink, &lstart, &ucounts, &u_start, &u_len, &u_circ, &m_vertex, &m_offset,
                       &m_span, &m_dst, &links, &d_roff, &d_bases, &spelled, &dropped, &removed, &ccounts, &o_lo, &o_hi, &o_cand, &verdict}) b->release();
  }
};

extern "C" void mhap_graph_default_params(mhap_graph_params* p) {
  if (!p) return;
  p->max_hang = 1000; p->int_frac_permille = 800; p->min_ovlp = 2000; p->fuzz = 1000; p->min_identity = 0.0;
}

extern "C" int mhap_graph_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_graph_params* params,
                                mhap_graph_session** session) {
  const char* who = "mhap_graph_begin";
  if (session) *session = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!session || n_reads < 0 || (n_reads > 0 && (!read_ids || !lengths))) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (n_reads >= ((int64_t)1 << 30)) { *v.err = std::string(who) + ": 2^30 reads or more"; return MHAP_E_INVALID; }
  mhap_graph_params p;
  mhap_graph_default_params(&p);
  if (params) p = *params;
  if (p.max_hang < 0 || p.int_frac_permille < 0 || p.int_frac_permille > 1000 || p.min_ovlp < 0 || p.fuzz < 0) {
    *v.err = std::string(who) + ": max_hang, min_ovlp and fuzz must be >= 0 and int_frac_permille in [0, 1000]";
    return MHAP_E_INVALID;
  }
  for (int64_t i = 0; i < n_reads; i++)
    if (lengths[i] < 0) { *v.err = std::string(who) + ": read " + std::to_string(i) + " has a negative length"; return MHAP_E_INVALID; }
  mhap_graph_session* s = new mhap_graph_session();
  s->P = GParams{p.max_hang, p.int_frac_permille, p.min_ovlp, p.fuzz, p.min_identity};
  (void)hipSetDevice(v.device);
  const size_t rb = 4 * (size_t)std::max<int64_t>(n_reads, 1);
  hipError_t e = s->begin_table(v, h, read_ids, lengths, n_reads);
  if (e == hipSuccess) e = s->contained.ensure(rb);
  if (e == hipSuccess) e = s->counts.ensure(8 * MHAP_GRAPH_COUNTS);
  if (e == hipSuccess) e = hipMemsetAsync(s->contained.p, 0, rb, v.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->counts.p, 0, 8 * MHAP_GRAPH_COUNTS, v.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
  if (e != hipSuccess) {
    s->release();
    delete s;
    return hip_fail(v, who, "the table of reads", e);
  }
  *session = s;
  return MHAP_OK;
}

extern "C" int mhap_graph_add(mhap_graph_session* s, const mhap_record* recs, int64_t n) {
  const char* who = "mhap_graph_add";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (n < 0 || (n > 0 && !recs)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (s->n_records + n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records"; return MHAP_E_INVALID; }
  s->reap(false);
  if (n == 0) return MHAP_OK;
  mhap_graph_session::Pending p;
  if (!graph_pack_records(s, who, recs, n, p.host, *v.err)) return MHAP_E_INVALID;
  (void)hipSetDevice(v.device);
  mhap_graph_session::Chunk c;
  hipError_t e = c.items.ensure(sizeof(GItem) * (size_t)n);
  if (e == hipSuccess) e = c.cls.ensure((size_t)n);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p.ev, hipEventDisableTiming);
  if (e != hipSuccess) { c.items.release(); c.cls.release(); return hip_fail(v, who, "hipMalloc of the records", e); }
  e = hipMemcpyAsync(c.items.p, p.host.data(), sizeof(GItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(classify_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, c.items.as<int4>(), n, (int32_t)s->n_records,
                       s->d_lengths.as<int32_t>(), s->P, c.cls.as<uint8_t>(), s->contained.as<uint32_t>(), s->counts.as<unsigned long long>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(p.ev, v.stream);
  if (e != hipSuccess) {   // nothing of this call stays; the upload may be in flight, so it is waited for before its source goes
    (void)hipStreamSynchronize(v.stream);
    (void)hipEventDestroy(p.ev);
    c.items.release(); c.cls.release();
    return hip_fail(v, who, "upload or launch", e);
  }
  c.n = n;
  s->chunks.push_back(c);
  s->pending.push_back(std::move(p));
  s->n_records += n;
  return MHAP_OK;
}

extern "C" int mhap_graph_finish(mhap_graph_session* s, int64_t* counts) {
  const char* who = "mhap_graph_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  s->n_arcs = -1;
  s->n_unitigs = -1;
  s->unitig_gen++;
  s->cleaned = false;   // (a clean starts from zeroed bytes: nothing to zero here)
  const int64_t nv = 2 * s->n_reads;
  hipError_t e = hipSuccess;
  auto fail = [&](const char* what) { return hip_fail(v, who, what, e); };
  unsigned long long* d_counts = s->counts.as<unsigned long long>();
  // the counts of this finish start from the classes the adds have summed
  if ((e = hipMemsetAsync(d_counts + GC_CONTAINED, 0, 8 * (MHAP_GRAPH_COUNTS - GC_CONTAINED), v.stream)) != hipSuccess) return fail("memset");
  const size_t vb = 4 * (size_t)(nv + 1), sb = 8 * (size_t)(nv + 1);
  if ((e = s->deg.ensure(vb)) != hipSuccess || (e = s->fill.ensure(vb)) != hipSuccess || (e = s->start.ensure(sb)) != hipSuccess ||
      (e = s->fstart.ensure(sb)) != hipSuccess) return fail("hipMalloc of the vertex tables");
  if ((e = hipMemsetAsync(s->deg.p, 0, vb, v.stream)) != hipSuccess || (e = hipMemsetAsync(s->fill.p, 0, vb, v.stream)) != hipSuccess) return fail("memset");
  if (s->n_reads > 0) hipLaunchKernelGGL(flags_kernel, dim3(blocks256(s->n_reads)), dim3(256), 0, v.stream, s->contained.as<uint32_t>(), s->n_reads, d_counts);
  for (auto& c : s->chunks)
    hipLaunchKernelGGL(count_kernel, dim3(blocks256(2 * c.n)), dim3(256), 0, v.stream, c.items.as<GArc>(), 2 * c.n, s->contained.as<uint32_t>(),
                       s->deg.as<int32_t>());
  hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->deg.as<int32_t>(), nv, s->start.as<int64_t>());
  if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
  int64_t n_live = 0, n_arcs = 0;
  if ((e = hipMemcpyAsync(&n_live, s->start.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
  s->reap(true);   // the stream is empty: every upload has been read
  if (n_live > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 arcs"; return MHAP_E_INVALID; }
  const size_t lb = (size_t)std::max<int64_t>(n_live, 1);
  if ((e = s->tmp.ensure(sizeof(GArc) * lb)) != hipSuccess || (e = s->keep.ensure(lb)) != hipSuccess) return fail("hipMalloc of the arcs");
  for (auto& c : s->chunks)
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks256(2 * c.n)), dim3(256), 0, v.stream, c.items.as<GArc>(), 2 * c.n, s->contained.as<uint32_t>(),
                       s->start.as<int64_t>(), s->fill.as<int32_t>(), s->tmp.as<GArc>());
  if (nv > 0) hipLaunchKernelGGL(dedup_kernel, dim3((unsigned)nv), dim3(64), 0, v.stream, s->tmp.as<GArc>(), s->start.as<int64_t>(), s->keep.as<uint8_t>(),
                                 s->deg.as<int32_t>());   // (deg has been scanned: it now takes the kept arcs per u)
  hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->deg.as<int32_t>(), nv, s->fstart.as<int64_t>());
  if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
  if ((e = hipMemcpyAsync(&n_arcs, s->fstart.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
  const size_t ab = 4 * (size_t)std::max<int64_t>(n_arcs, 1);
  for (DevBuf* b : {&s->U, &s->V, &s->LEN, &s->Q, &s->bt_v, &s->bt_pos, &s->mark})
    if ((e = b->ensure(ab)) != hipSuccess) return fail("hipMalloc of the arc list");
  if ((e = s->rows.ensure(7 * ab)) != hipSuccess) return fail("hipMalloc of the arc list");
  if ((e = hipMemsetAsync(s->mark.p, 0, ab, v.stream)) != hipSuccess) return fail("memset");
  if (n_arcs > 0) {
    hipLaunchKernelGGL(place_kernel, dim3((unsigned)nv), dim3(64), 0, v.stream, s->tmp.as<GArc>(), s->keep.as<uint8_t>(), s->start.as<int64_t>(),
                       s->fstart.as<int64_t>(), s->U.as<int32_t>(), s->V.as<int32_t>(), s->LEN.as<int32_t>(), s->Q.as<int32_t>(),
                       s->bt_v.as<int32_t>(), s->bt_pos.as<int32_t>());
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)nv), dim3(64), 0, v.stream, s->fstart.as<int64_t>(), s->V.as<int32_t>(), s->LEN.as<int32_t>(),
                       s->bt_v.as<int32_t>(), s->bt_pos.as<int32_t>(), s->P.fuzz, s->mark.as<int32_t>());
    hipLaunchKernelGGL(finish_kernel, dim3(blocks256(n_arcs)), dim3(256), 0, v.stream, n_arcs, s->fstart.as<int64_t>(), s->U.as<int32_t>(),
                       s->V.as<int32_t>(), s->LEN.as<int32_t>(), s->Q.as<int32_t>(), s->bt_v.as<int32_t>(), s->bt_pos.as<int32_t>(),
                       s->mark.as<int32_t>(), s->d_lengths.as<int32_t>(), s->rows.as<int32_t>(), d_counts);
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
  }
  unsigned long long hc[MHAP_GRAPH_COUNTS];
  if ((e = hipMemcpyAsync(hc, d_counts, sizeof hc, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
  for (int k = 0; k < MHAP_GRAPH_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[GC_RECORDS] = s->n_records;
  counts[GC_ARCS] = n_arcs;
  s->n_arcs = n_arcs;
  s->n_contained = (int64_t)hc[GC_CONTAINED];
  s->finish_records = s->n_records;
  return MHAP_OK;
}

extern "C" int mhap_graph_info(const mhap_graph_session* s, int64_t* n_reads, int64_t* n_records, int64_t* n_arcs) {
  if (!s) return MHAP_E_INVALID;
  if (n_reads) *n_reads = s->n_reads;
  if (n_records) *n_records = s->n_records;
  if (n_arcs) *n_arcs = s->n_arcs;
  return MHAP_OK;
}

extern "C" int mhap_graph_copy_arcs(mhap_graph_session* s, int32_t* rows) {
  const char* who = "mhap_graph_copy_arcs";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->n_arcs < 0) { *v.err = std::string(who) + ": no mhap_graph_finish has completed"; return MHAP_E_INVALID; }
  if (s->n_arcs == 0) return MHAP_OK;
  if (!rows) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return s->download(who, rows, s->rows.p, 28 * (size_t)s->n_arcs);
}

extern "C" int mhap_graph_copy_classes(mhap_graph_session* s, uint8_t* classes) {
  const char* who = "mhap_graph_copy_classes";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->n_records == 0) return MHAP_OK;
  if (!classes) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  int64_t at = 0;
  for (auto& c : s->chunks) {
    const int rc = s->download(who, classes + at, c.cls.p, (size_t)c.n);
    if (rc != MHAP_OK) return rc;
    at += c.n;
  }
  return MHAP_OK;
}

extern "C" int mhap_graph_copy_read_flags(mhap_graph_session* s, uint8_t* flags) {
  const char* who = "mhap_graph_copy_read_flags";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->n_reads == 0) return MHAP_OK;
  if (!flags) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  std::vector<uint32_t> w((size_t)s->n_reads);
  const int rc = s->download(who, w.data(), s->contained.p, 4 * w.size());
  if (rc != MHAP_OK) return rc;
  for (int64_t r = 0; r < s->n_reads; r++) flags[r] = w[(size_t)r] ? 1 : 0;
  return MHAP_OK;
}

namespace {

// The refusals mhap_graph_unitigs and mhap_graph_clean share.
int need_finish(mhap_graph_session* s, const HandleView& v, const char* who) {
  if (s->n_arcs < 0) { *v.err = std::string(who) + ": no mhap_graph_finish has completed"; return MHAP_E_INVALID; }
  if (s->n_records != s->finish_records) {   // (an add may have set contained flags the list does not know of)
    *v.err = std::string(who) + ": records were added after the last mhap_graph_finish";
    return MHAP_E_INVALID;
  }
  return MHAP_OK;
}

// A unitig build in two halves, queued without a wait, over the vertices and arcs the masks leave (both null: the uncleaned graph).
// Front: everything up to the four numbering scans, whose last entries are the sizes.  Back: the tables in their places; they must
// hold the sizes of this build (mhap_graph_unitigs reads the sizes in between, a cleaning round allocates for the largest possible).
int unitigs_front(mhap_graph_session* s, const HandleView& v, const char* who, const uint8_t* dropped, const uint8_t* removed) {
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  hipError_t e = hipSuccess;
  auto fail = [&](const char* what) { return hip_fail(v, who, what, e); };
  const size_t v4 = 4 * (size_t)nv, v8 = 8 * (size_t)nv, s8 = 8 * (size_t)(nv + 1), a4 = 4 * (size_t)std::max<int64_t>(na, 1), as8 = 8 * (size_t)(na + 1);
  for (DevBuf* b : {&s->fout, &s->cand, &s->carc, &s->unext, &s->uprev, &s->uspan, &s->uP[0], &s->uP[1], &s->uR[0], &s->uR[1], &s->uQ[0], &s->uQ[1],
                    &s->uM[0], &s->uM[1], &s->tail, &s->cnt, &s->kept})
    if ((e = b->ensure(v4)) != hipSuccess) return fail("hipMalloc of the vertex tables");
  for (DevBuf* b : {&s->uO[0], &s->uO[1], &s->ulen})
    if ((e = b->ensure(v8)) != hipSuccess) return fail("hipMalloc of the vertex tables");
  for (DevBuf* b : {&s->unum, &s->mstart, &s->bstart})
    if ((e = b->ensure(s8)) != hipSuccess) return fail("hipMalloc of the vertex tables");
  if ((e = s->cyc.ensure((size_t)nv)) != hipSuccess || (e = s->ucounts.ensure(8 * UC_DEVICE)) != hipSuccess || (e = s->islink.ensure(a4)) != hipSuccess ||
      (e = s->lstart.ensure(as8)) != hipSuccess) return fail("hipMalloc of the vertex tables");
  unsigned long long* d_uc = s->ucounts.as<unsigned long long>();
  if ((e = hipMemsetAsync(s->uprev.p, 0xFF, v4, v.stream)) != hipSuccess || (e = hipMemsetAsync(s->tail.p, 0xFF, v4, v.stream)) != hipSuccess ||
      (e = hipMemsetAsync(s->cnt.p, 0, v4, v.stream)) != hipSuccess || (e = hipMemsetAsync(s->ulen.p, 0, v8, v.stream)) != hipSuccess ||
      (e = hipMemsetAsync(d_uc, 0, 8 * UC_DEVICE, v.stream)) != hipSuccess) return fail("memset");
  const dim3 gv(blocks256(nv)), b256(256);
  const bool masks = dropped != nullptr;   // (both or neither)
  hipLaunchKernelGGL(masks ? outdeg_kernel<true> : outdeg_kernel<false>, gv, b256, 0, v.stream, nv, s->fstart.as<int64_t>(), s->V.as<int32_t>(),
                     s->rows.as<int32_t>(), removed, s->fout.as<int32_t>(), s->cand.as<int32_t>(), s->carc.as<int32_t>());
  hipLaunchKernelGGL(next_kernel, gv, b256, 0, v.stream, nv, s->fout.as<int32_t>(), s->cand.as<int32_t>(), s->carc.as<int32_t>(), s->LEN.as<int32_t>(),
                     s->d_lengths.as<int32_t>(), s->unext.as<int32_t>(), s->uprev.as<int32_t>(), s->uspan.as<int32_t>(), d_uc);
  // the rounds: 2^rounds >= the vertices in play, which no chain and no cycle exceeds; nothing waits between them
  const int64_t in_play = std::max<int64_t>(2, 2 * (s->n_reads - s->n_contained));
  int rounds = 1;
  while (((int64_t)1 << rounds) < in_play) rounds++;
  int cur = 0;
  auto rank_rounds = [&]() {
    for (int r = 0; r < rounds; r++, cur ^= 1)
      hipLaunchKernelGGL(rank_round_kernel, gv, b256, 0, v.stream, nv, s->uP[cur].as<int32_t>(), s->uR[cur].as<uint32_t>(),
                         s->uO[cur].as<unsigned long long>(), s->uP[cur ^ 1].as<int32_t>(), s->uR[cur ^ 1].as<uint32_t>(),
                         s->uO[cur ^ 1].as<unsigned long long>());
  };
  hipLaunchKernelGGL(masks ? rank_init_kernel<true> : rank_init_kernel<false>, gv, b256, 0, v.stream, nv, s->contained.as<uint32_t>(), dropped, s->uprev.as<int32_t>(), s->uspan.as<int32_t>(),
                     s->uP[0].as<int32_t>(), s->uR[0].as<uint32_t>(), s->uO[0].as<unsigned long long>());
  rank_rounds();
  hipLaunchKernelGGL(cyc_init_kernel, gv, b256, 0, v.stream, nv, s->uP[cur].as<int32_t>(), s->uprev.as<int32_t>(), s->cyc.as<uint8_t>(),
                     s->uQ[0].as<int32_t>(), s->uM[0].as<int32_t>());
  int mc = 0;
  for (int r = 0; r < rounds; r++, mc ^= 1)
    hipLaunchKernelGGL(min_round_kernel, gv, b256, 0, v.stream, nv, s->cyc.as<uint8_t>(), s->uQ[mc].as<int32_t>(), s->uM[mc].as<int32_t>(),
                       s->uQ[mc ^ 1].as<int32_t>(), s->uM[mc ^ 1].as<int32_t>());
  const int32_t* M = s->uM[mc].as<int32_t>();
  hipLaunchKernelGGL(cut_init_kernel, gv, b256, 0, v.stream, nv, s->cyc.as<uint8_t>(), M, s->uprev.as<int32_t>(), s->uspan.as<int32_t>(),
                     s->uP[cur].as<int32_t>(), s->uR[cur].as<uint32_t>(), s->uO[cur].as<unsigned long long>());
  rank_rounds();
  s->u_cur = cur;   // where the ranks ended: the back half reads them
  const int32_t* P = s->uP[cur].as<int32_t>();
  const uint32_t* R = s->uR[cur].as<uint32_t>();
  const unsigned long long* O = s->uO[cur].as<unsigned long long>();
  hipLaunchKernelGGL(tails_kernel, gv, b256, 0, v.stream, nv, P, R, O, s->unext.as<int32_t>(), s->uspan.as<int32_t>(), s->cyc.as<uint8_t>(), M,
                     s->tail.as<int32_t>(), s->cnt.as<int32_t>(), s->ulen.as<int64_t>());
  hipLaunchKernelGGL(select_kernel, gv, b256, 0, v.stream, nv, P, s->cyc.as<uint8_t>(), M, s->tail.as<int32_t>(), s->kept.as<int32_t>(),
                     s->cnt.as<int32_t>(), s->ulen.as<int64_t>(), d_uc);
  hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->kept.as<int32_t>(), nv, s->unum.as<int64_t>());
  hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->cnt.as<int32_t>(), nv, s->mstart.as<int64_t>());
  hipLaunchKernelGGL(scan_kernel<int64_t>, dim3(1), dim3(1024), 0, v.stream, s->ulen.as<int64_t>(), nv, s->bstart.as<int64_t>());
  if (na > 0) hipLaunchKernelGGL(masks ? linkflag_kernel<true> : linkflag_kernel<false>, dim3(blocks256(na)), b256, 0, v.stream, na,
                                 s->rows.as<int32_t>(), removed, s->unext.as<int32_t>(), s->islink.as<int32_t>());
  hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->islink.as<int32_t>(), na, s->lstart.as<int64_t>());
  if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
  return MHAP_OK;
}

// the tables for nu unitigs, nm members and nl links
int unitigs_tables(mhap_graph_session* s, const HandleView& v, const char* who, int64_t nu, int64_t nm, int64_t nl) {
  const size_t ub = (size_t)std::max<int64_t>(nu, 1), mb = (size_t)std::max<int64_t>(nm, 1), lb = (size_t)std::max<int64_t>(nl, 1);
  hipError_t e;
  if ((e = s->u_start.ensure(8 * ub)) != hipSuccess || (e = s->u_len.ensure(8 * ub)) != hipSuccess || (e = s->u_circ.ensure(ub)) != hipSuccess ||
      (e = s->m_vertex.ensure(4 * mb)) != hipSuccess || (e = s->m_offset.ensure(8 * mb)) != hipSuccess || (e = s->m_span.ensure(4 * mb)) != hipSuccess ||
      (e = s->m_dst.ensure(8 * mb)) != hipSuccess || (e = s->links.ensure(24 * lb)) != hipSuccess) return hip_fail(v, who, "hipMalloc of the unitigs", e);
  return MHAP_OK;
}

int unitigs_back(mhap_graph_session* s, const HandleView& v, const char* who, bool links) {
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  const dim3 gv(blocks256(nv)), b256(256);
  const int32_t* P = s->uP[s->u_cur].as<int32_t>();
  const uint32_t* R = s->uR[s->u_cur].as<uint32_t>();
  const unsigned long long* O = s->uO[s->u_cur].as<unsigned long long>();
  hipLaunchKernelGGL(unitig_scatter_kernel, gv, b256, 0, v.stream, nv, s->kept.as<int32_t>(), s->unum.as<int64_t>(), s->mstart.as<int64_t>(),
                     s->ulen.as<int64_t>(), s->cyc.as<uint8_t>(), s->u_start.as<int64_t>(), s->u_len.as<int64_t>(), s->u_circ.as<uint8_t>());
  hipLaunchKernelGGL(member_scatter_kernel, gv, b256, 0, v.stream, nv, P, R, O, s->uspan.as<int32_t>(), s->kept.as<int32_t>(), s->mstart.as<int64_t>(),
                     s->bstart.as<int64_t>(), s->m_vertex.as<int32_t>(), s->m_offset.as<int64_t>(), s->m_span.as<int32_t>(), s->m_dst.as<int64_t>());
  if (links) hipLaunchKernelGGL(link_scatter_kernel, dim3(blocks256(na)), b256, 0, v.stream, na, s->rows.as<int32_t>(), s->islink.as<int32_t>(),
                                s->lstart.as<int64_t>(), P, s->kept.as<int32_t>(), s->unum.as<int64_t>(), s->links.as<int32_t>());
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? hip_fail(v, who, "launch", e) : MHAP_OK;
}

// The unitigs the copy and spell calls serve, built anew over what the masks leave; counts: MHAP_UNITIG_COUNTS.
int build_unitigs(mhap_graph_session* s, const HandleView& v, const char* who, const uint8_t* dropped, const uint8_t* removed, int64_t* counts) {
  s->n_unitigs = -1;
  s->unitig_gen++;
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) counts[k] = 0;
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) s->last_counts[k] = 0;
  if (nv == 0) { s->n_unitigs = s->n_members = s->n_links = s->n_ubases = 0; return MHAP_OK; }
  hipError_t e = hipSuccess;
  auto fail = [&](const char* what) { return hip_fail(v, who, what, e); };
  int rc = unitigs_front(s, v, who, dropped, removed);
  if (rc != MHAP_OK) return rc;
  int64_t nu = 0, nm = 0, nb = 0, nl = 0;
  if ((e = hipMemcpyAsync(&nu, s->unum.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&nm, s->mstart.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&nb, s->bstart.as<int64_t>() + nv, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipMemcpyAsync(&nl, s->lstart.as<int64_t>() + na, 8, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
  if ((rc = unitigs_tables(s, v, who, nu, nm, nl)) != MHAP_OK || (rc = unitigs_back(s, v, who, nl > 0)) != MHAP_OK) return rc;
  unsigned long long hc[UC_DEVICE];
  if ((e = hipMemcpyAsync(hc, s->ucounts.p, sizeof hc, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
  counts[0] = nu; counts[1] = (int64_t)hc[UC_CIRCULAR]; counts[2] = nm; counts[3] = (int64_t)hc[UC_JOINED]; counts[4] = nl;
  counts[5] = (int64_t)hc[UC_LONGEST]; counts[6] = nb;
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) s->last_counts[k] = counts[k];
  s->n_members = nm; s->n_links = nl; s->n_ubases = nb;
  s->n_unitigs = nu;
  return MHAP_OK;
}

}  // namespace

extern "C" int mhap_graph_unitigs(mhap_graph_session* s, int64_t* counts) {
  const char* who = "mhap_graph_unitigs";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  const int rc = need_finish(s, v, who);
  if (rc != MHAP_OK) return rc;
  (void)hipSetDevice(v.device);
  return build_unitigs(s, v, who, nullptr, nullptr, counts);
}

extern "C" void mhap_graph_default_clean_params(mhap_clean_params* p) {
  if (!p) return;
  p->tip_reads = 4; p->bubble_bases = 50000; p->max_rounds = 16;
}

extern "C" int mhap_graph_clean(mhap_graph_session* s, const mhap_clean_params* params, int64_t* counts) {
  const char* who = "mhap_graph_clean";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  mhap_clean_params p;
  mhap_graph_default_clean_params(&p);
  if (params) p = *params;
  if (p.tip_reads < 0 || p.bubble_bases < 0 || p.max_rounds < 1) {
    *v.err = std::string(who) + ": tip_reads and bubble_bases must be >= 0 and max_rounds >= 1";
    return MHAP_E_INVALID;
  }
  int rc = need_finish(s, v, who);
  if (rc != MHAP_OK) return rc;
  (void)hipSetDevice(v.device);
  s->n_unitigs = -1;
  s->cleaned = false;
  const int64_t nr = s->n_reads, nv = 2 * nr, na = s->n_arcs;
  hipError_t e = hipSuccess;
  auto fail = [&](const char* what) { return hip_fail(v, who, what, e); };
  const size_t rb = (size_t)std::max<int64_t>(nr, 1), ab = (size_t)std::max<int64_t>(na, 1);
  if ((e = s->dropped.ensure(rb)) != hipSuccess || (e = s->removed.ensure(ab)) != hipSuccess || (e = s->ccounts.ensure(8 * MHAP_CLEAN_COUNTS)) != hipSuccess ||
      (e = s->o_lo.ensure(4 * 2 * rb)) != hipSuccess || (e = s->o_hi.ensure(4 * 2 * rb)) != hipSuccess || (e = s->o_cand.ensure(2 * rb)) != hipSuccess ||
      (e = s->verdict.ensure(rb)) != hipSuccess) return fail("hipMalloc of the clean state");
  // every call starts again from the uncleaned graph
  if ((e = hipMemsetAsync(s->dropped.p, 0, rb, v.stream)) != hipSuccess || (e = hipMemsetAsync(s->removed.p, 0, ab, v.stream)) != hipSuccess ||
      (e = hipMemsetAsync(s->ccounts.p, 0, 8 * MHAP_CLEAN_COUNTS, v.stream)) != hipSuccess) return fail("memset");
  unsigned long long hc[MHAP_CLEAN_COUNTS] = {0};
  int64_t rounds = 0;
  if (nv > 0) {
    // a round's tables at their largest: a unitig and a member per read, a link per arc
    if ((rc = unitigs_tables(s, v, who, nr, nr, na)) != MHAP_OK) return rc;
    uint8_t* dropped = s->dropped.as<uint8_t>();
    uint8_t* removed = s->removed.as<uint8_t>();
    unsigned long long* d_cc = s->ccounts.as<unsigned long long>();
    const dim3 gx(blocks256(nv)), gr(blocks256(nr)), b256(256);
    unsigned long long before = 0;
    while (rounds < p.max_rounds) {
      if ((rc = unitigs_front(s, v, who, dropped, removed)) != MHAP_OK || (rc = unitigs_back(s, v, who, na > 0)) != MHAP_OK) return rc;
      const UTables U{s->unum.as<int64_t>() + nv, s->mstart.as<int64_t>() + nv, s->lstart.as<int64_t>() + na, s->u_start.as<int64_t>(),
                      s->u_len.as<int64_t>(), s->u_circ.as<uint8_t>(), s->m_vertex.as<int32_t>(), s->links.as<int32_t>()};
      hipLaunchKernelGGL(origin_kernel, gx, b256, 0, v.stream, U, s->fstart.as<int64_t>(), s->o_lo.as<int32_t>(), s->o_hi.as<int32_t>());
      hipLaunchKernelGGL(degree_kernel, gx, b256, 0, v.stream, U, s->o_lo.as<int32_t>(), s->o_hi.as<int32_t>(), p.tip_reads, s->o_cand.as<uint8_t>());
      hipLaunchKernelGGL(tip_kernel, gr, b256, 0, v.stream, U, s->o_lo.as<int32_t>(), s->o_hi.as<int32_t>(), s->o_cand.as<uint8_t>(),
                         s->verdict.as<uint8_t>(), d_cc);
      hipLaunchKernelGGL(bubble_kernel, gr, b256, 0, v.stream, U, s->o_lo.as<int32_t>(), s->o_hi.as<int32_t>(), p.bubble_bases, s->verdict.as<uint8_t>(), d_cc);
      hipLaunchKernelGGL(drop_kernel, gr, b256, 0, v.stream, U, s->verdict.as<uint8_t>(), dropped, d_cc);
      if (na > 0) hipLaunchKernelGGL(removed_kernel, dim3(blocks256(na)), b256, 0, v.stream, na, s->rows.as<int32_t>(), dropped, removed, d_cc);
      if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
      // the one wait of a round: did it remove anything
      if ((e = hipMemcpyAsync(hc, d_cc, sizeof hc, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
      if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("kernel");
      rounds++;
      if (hc[CC_TIPS] + hc[CC_BUBBLES] == before) break;
      before = hc[CC_TIPS] + hc[CC_BUBBLES];
    }
  } else rounds = 1;
  int64_t uc[MHAP_UNITIG_COUNTS];
  if ((rc = build_unitigs(s, v, who, s->dropped.as<uint8_t>(), s->removed.as<uint8_t>(), uc)) != MHAP_OK) return rc;
  for (int k = 0; k < MHAP_CLEAN_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[CC_ROUNDS] = rounds;
  s->cleaned = true;
  return MHAP_OK;
}

extern "C" int mhap_graph_copy_dropped(mhap_graph_session* s, uint8_t* per_read) {
  const char* who = "mhap_graph_copy_dropped";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!s->cleaned) { *v.err = std::string(who) + ": no mhap_graph_clean has completed since the last mhap_graph_finish"; return MHAP_E_INVALID; }
  if (s->n_reads == 0) return MHAP_OK;
  if (!per_read) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return s->download(who, per_read, s->dropped.p, (size_t)s->n_reads);
}

extern "C" int mhap_graph_copy_removed(mhap_graph_session* s, uint8_t* per_arc) {
  const char* who = "mhap_graph_copy_removed";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!s->cleaned) { *v.err = std::string(who) + ": no mhap_graph_clean has completed since the last mhap_graph_finish"; return MHAP_E_INVALID; }
  if (s->n_arcs == 0) return MHAP_OK;
  if (!per_arc) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return s->download(who, per_arc, s->removed.p, (size_t)s->n_arcs);
}

namespace {

// the session of a copy or spell call: its unitigs must be those of the last finish
int need_unitigs(mhap_graph_session* s, const char* who) {
  if (s->n_unitigs >= 0) return MHAP_OK;
  *handle_view(s->h).err = std::string(who) + ": no mhap_graph_unitigs has completed since the last mhap_graph_finish";
  return MHAP_E_INVALID;
}

int null_arg(mhap_graph_session* s, const char* who) {
  *handle_view(s->h).err = std::string(who) + ": null argument";
  return MHAP_E_INVALID;
}

}  // namespace

extern "C" int mhap_graph_unitigs_info(const mhap_graph_session* s, int64_t* n_unitigs, int64_t* n_members, int64_t* n_links, int64_t* n_bases) {
  if (!s) return MHAP_E_INVALID;
  if (n_unitigs) *n_unitigs = s->n_unitigs;
  if (n_members) *n_members = s->n_unitigs < 0 ? 0 : s->n_members;
  if (n_links) *n_links = s->n_unitigs < 0 ? 0 : s->n_links;
  if (n_bases) *n_bases = s->n_unitigs < 0 ? 0 : s->n_ubases;
  return MHAP_OK;
}

extern "C" int mhap_graph_unitigs_counts(mhap_graph_session* s, int64_t* counts) {
  const char* who = "mhap_graph_unitigs_counts";
  if (!s) return MHAP_E_INVALID;
  const int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (!counts) return null_arg(s, who);
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) counts[k] = s->last_counts[k];
  return MHAP_OK;
}

extern "C" int mhap_graph_copy_unitigs(mhap_graph_session* s, int64_t* unitig_start, int64_t* unitig_len, uint8_t* circular) {
  const char* who = "mhap_graph_copy_unitigs";
  if (!s) return MHAP_E_INVALID;
  int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (!unitig_start) return null_arg(s, who);
  unitig_start[s->n_unitigs] = s->n_members;
  if (s->n_unitigs == 0) return MHAP_OK;
  if (!unitig_len || !circular) return null_arg(s, who);
  if ((rc = s->download(who, unitig_start, s->u_start.p, 8 * (size_t)s->n_unitigs)) != MHAP_OK) return rc;
  if ((rc = s->download(who, unitig_len, s->u_len.p, 8 * (size_t)s->n_unitigs)) != MHAP_OK) return rc;
  return s->download(who, circular, s->u_circ.p, (size_t)s->n_unitigs);
}

extern "C" int mhap_graph_copy_layout(mhap_graph_session* s, int32_t* vertex, int64_t* offset, int32_t* span) {
  const char* who = "mhap_graph_copy_layout";
  if (!s) return MHAP_E_INVALID;
  int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (s->n_members == 0) return MHAP_OK;
  if (!vertex || !offset || !span) return null_arg(s, who);
  if ((rc = s->download(who, vertex, s->m_vertex.p, 4 * (size_t)s->n_members)) != MHAP_OK) return rc;
  if ((rc = s->download(who, offset, s->m_offset.p, 8 * (size_t)s->n_members)) != MHAP_OK) return rc;
  return s->download(who, span, s->m_span.p, 4 * (size_t)s->n_members);
}

extern "C" int mhap_graph_copy_links(mhap_graph_session* s, int32_t* rows) {
  const char* who = "mhap_graph_copy_links";
  if (!s) return MHAP_E_INVALID;
  const int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (s->n_links == 0) return MHAP_OK;
  if (!rows) return null_arg(s, who);
  return s->download(who, rows, s->links.p, 24 * (size_t)s->n_links);
}

extern "C" int mhap_graph_spell_device(mhap_graph_session* s, const uint8_t* d_bases, int64_t n_bases, const int64_t* offsets, uint8_t* out) {
  const char* who = "mhap_graph_spell";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (n_bases < 0 || (s->n_reads > 0 && !offsets)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  for (int64_t r = 0; r < s->n_reads; r++)
    if (offsets[r] < 0 || offsets[r] > n_bases || (int64_t)s->lengths[(size_t)r] > n_bases - offsets[r]) {
      *v.err = std::string(who) + ": read " + std::to_string(r) + " is [" + std::to_string(offsets[r]) + ", " +
               std::to_string(offsets[r] + s->lengths[(size_t)r]) + ") of " + std::to_string(n_bases) + " bases";
      return MHAP_E_INVALID;
    }
  if (s->n_ubases == 0) return MHAP_OK;
  if (!d_bases || !out) return null_arg(s, who);
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = s->d_roff.ensure(8 * (size_t)s->n_reads)) != hipSuccess || (e = s->spelled.ensure((size_t)s->n_ubases)) != hipSuccess)
    return hip_fail(v, who, "hipMalloc", e);
  if ((e = hipMemcpyAsync(s->d_roff.p, offsets, 8 * (size_t)s->n_reads, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  const int64_t tiles = (s->n_ubases + SPELL_CHUNK - 1) / SPELL_CHUNK;
  if (tiles > INT32_MAX) { (void)hipStreamSynchronize(v.stream); *v.err = std::string(who) + ": more than 2^31 - 1 tiles of output"; return MHAP_E_INVALID; }
  hipLaunchKernelGGL(spell_kernel, dim3((unsigned)tiles), dim3(SPELL_T), 0, v.stream, d_bases, n_bases, s->d_roff.as<int64_t>(), s->d_lengths.as<int32_t>(),
                     s->n_members, s->m_vertex.as<int32_t>(), s->m_span.as<int32_t>(), s->m_dst.as<int64_t>(), s->n_ubases, s->spelled.as<uint8_t>());
  if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
  if ((e = hipMemcpyAsync(out, s->spelled.p, (size_t)s->n_ubases, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) {
    (void)hipStreamSynchronize(v.stream);
    return hip_fail(v, who, "download", e);
  }
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  return MHAP_OK;
}

extern "C" int mhap_graph_spell(mhap_graph_session* s, const uint8_t* bases, int64_t n_bases, const int64_t* offsets, uint8_t* out) {
  const char* who = "mhap_graph_spell";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_unitigs(s, who);
  if (rc != MHAP_OK) return rc;
  if (n_bases < 0 || (n_bases > 0 && !bases)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = s->d_bases.ensure((size_t)std::max<int64_t>(n_bases, 1))) != hipSuccess) return hip_fail(v, who, "hipMalloc of the bases", e);
  if (n_bases > 0) {   // (waited for: the caller's bytes are free when the call returns, whatever it returns)
    if ((e = hipMemcpyAsync(s->d_bases.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, v.stream)) != hipSuccess ||
        (e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  }
  return mhap_graph_spell_device(s, s->d_bases.as<uint8_t>(), n_bases, offsets, out);
}

extern "C" void mhap_graph_free(mhap_graph_session* s) {
  if (!s) return;
  HandleView v = handle_view(s->h);
  (void)hipSetDevice(v.device);
  if (!s->pending.empty()) (void)hipStreamSynchronize(v.stream);   // an upload may still be reading its source
  s->reap(true);
  s->release();
  delete s;
}

// what the unitig consensus (consensus_kernels.hip) reads of a graph session besides its public calls
mhap::GraphView mhap::graph_view(const mhap_graph_session* s) {
  return GraphView{s->h, s->P, s->n_reads, s->ids.data(), s->lengths.data(), s->unitig_gen, s->n_unitigs};
}
bool mhap::graph_pack_records(const mhap_graph_session* s, const char* who, const mhap_record* recs, int64_t n, std::vector<GItem>& out, std::string& err) {
  out.resize((size_t)n);
  for (int64_t q = 0; q < n; q++) {   // (the lookup alone: a record's aligned ends index nothing here)
    int32_t idx[2];
    if (!s->find_reads(who, q, recs[q], idx, err)) return false;
    out[(size_t)q] = pack_item(idx, recs[q]);
  }
  return true;
}

extern "C" int mhap_format_gfa_link(const int32_t* row7, const int64_t* read_ids, char* out, size_t cap) {
  if (!row7 || !read_ids || (!out && cap > 0)) return -1;
  return snprintf(out, cap, "L\t%lld\t%c\t%lld\t%c\t%dM", (long long)read_ids[row7[0] >> 1], (row7[0] & 1) ? '-' : '+',
                  (long long)read_ids[row7[1] >> 1], (row7[1] & 1) ? '-' : '+', row7[3]);
}

extern "C" int mhap_format_gfa_unitig_link(const int32_t* row6, char* out, size_t cap) {
  if (!row6 || (!out && cap > 0)) return -1;
  return snprintf(out, cap, "L\tutg%06dl\t%c\tutg%06dl\t%c\t%dM", row6[0] + 1, row6[1] ? '-' : '+', row6[2] + 1, row6[3] ? '-' : '+', row6[4]);
}
