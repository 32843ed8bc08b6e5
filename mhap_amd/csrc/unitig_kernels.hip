// unitig_kernels.hip — what is made of a finished string graph (graph_kernels.hip), over the session of graph_session.hpp: its
// unitigs (mhap_graph_unitigs / _unitigs_info / _unitigs_counts / _copy_unitigs / _copy_layout / _copy_links), their spelling
// (mhap_graph_spell / _spell_device) and the cleaning of the graph in rounds (mhap_graph_clean / _copy_dropped / _copy_removed).
// Each of the two parts has the list of its kernels in front of them.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "graph_session.hpp"

namespace mhap {
namespace {

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

// A unitig build in two halves, queued without a wait, over the vertices and arcs the masks leave (both null: the uncleaned graph).
// Front: everything up to the four numbering scans, whose last entries are the sizes.  Back: the tables in their places; they must
// hold the sizes of this build (mhap_graph_unitigs reads the sizes in between, a cleaning round allocates for the largest possible).
int unitigs_front(mhap_graph_session* s, const HandleView& v, const char* who, const uint8_t* dropped, const uint8_t* removed) {
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  const GraphArcs& a = s->arc;
  UnitigBuild& b = s->ub;
  const char* vt = "hipMalloc of the vertex tables";
  Steps q{hipSuccess, v.stream};
  q.ensure_all(vt, (size_t)nv, b.fout, b.cand, b.carc, b.next, b.prev, b.span, b.P[0], b.P[1], b.R[0], b.R[1], b.Q[0], b.Q[1], b.M[0], b.M[1],
               b.tail, b.cnt, b.kept, b.O[0], b.O[1], b.ulen, b.cyc);
  q.ensure_all(vt, (size_t)(nv + 1), b.unum, b.mstart, b.bstart);
  q.ensure(b.ucounts, UC_DEVICE, vt);
  q.ensure(b.islink, (size_t)std::max<int64_t>(na, 1), vt); q.ensure(b.lstart, (size_t)(na + 1), vt);
  q.fill(b.prev.get(), 0xFF, 4 * (size_t)nv); q.fill(b.tail.get(), 0xFF, 4 * (size_t)nv);
  q.zero(b.cnt, (size_t)nv); q.zero(b.ulen, (size_t)nv); q.zero(b.ucounts, UC_DEVICE);
  if (!q.ok()) return q.fail(v, who);
  const int32_t* lengths = (const int32_t*)s->d_lengths.p;
  const dim3 gv(blocks256(nv)), b256(256), one(1), b1024(1024);
  const bool masks = dropped != nullptr;   // (both or neither)
  hipLaunchKernelGGL(masks ? outdeg_kernel<true> : outdeg_kernel<false>, gv, b256, 0, v.stream, nv, a.fstart.get(), a.V.get(), a.rows.get(), removed,
                     b.fout.get(), b.cand.get(), b.carc.get());
  hipLaunchKernelGGL(next_kernel, gv, b256, 0, v.stream, nv, b.fout.get(), b.cand.get(), b.carc.get(), a.LEN.get(), lengths, b.next.get(),
                     b.prev.get(), b.span.get(), b.ucounts.get());
  // the rounds: 2^rounds >= the vertices in play, which no chain and no cycle exceeds; nothing waits between them
  const int64_t in_play = std::max<int64_t>(2, 2 * (s->n_reads - s->n_contained));
  int rounds = 1;
  while (((int64_t)1 << rounds) < in_play) rounds++;
  int cur = 0;
  auto rank_rounds = [&]() {
    for (int r = 0; r < rounds; r++, cur ^= 1)
      hipLaunchKernelGGL(rank_round_kernel, gv, b256, 0, v.stream, nv, b.P[cur].get(), b.R[cur].get(), b.O[cur].get(), b.P[cur ^ 1].get(),
                         b.R[cur ^ 1].get(), b.O[cur ^ 1].get());
  };
  hipLaunchKernelGGL(masks ? rank_init_kernel<true> : rank_init_kernel<false>, gv, b256, 0, v.stream, nv, s->ad.contained.get(), dropped, b.prev.get(),
                     b.span.get(), b.P[0].get(), b.R[0].get(), b.O[0].get());
  rank_rounds();
  hipLaunchKernelGGL(cyc_init_kernel, gv, b256, 0, v.stream, nv, b.P[cur].get(), b.prev.get(), b.cyc.get(), b.Q[0].get(), b.M[0].get());
  int mc = 0;
  for (int r = 0; r < rounds; r++, mc ^= 1)
    hipLaunchKernelGGL(min_round_kernel, gv, b256, 0, v.stream, nv, b.cyc.get(), b.Q[mc].get(), b.M[mc].get(), b.Q[mc ^ 1].get(), b.M[mc ^ 1].get());
  const int32_t* M = b.M[mc].get();
  hipLaunchKernelGGL(cut_init_kernel, gv, b256, 0, v.stream, nv, b.cyc.get(), M, b.prev.get(), b.span.get(), b.P[cur].get(), b.R[cur].get(),
                     b.O[cur].get());
  rank_rounds();
  s->u_cur = cur;   // where the ranks ended: the back half reads them
  hipLaunchKernelGGL(tails_kernel, gv, b256, 0, v.stream, nv, b.P[cur].get(), b.R[cur].get(), b.O[cur].get(), b.next.get(), b.span.get(), b.cyc.get(),
                     M, b.tail.get(), b.cnt.get(), b.ulen.get());
  hipLaunchKernelGGL(select_kernel, gv, b256, 0, v.stream, nv, b.P[cur].get(), b.cyc.get(), M, b.tail.get(), b.kept.get(), b.cnt.get(), b.ulen.get(),
                     b.ucounts.get());
  hipLaunchKernelGGL(scan_kernel<int32_t>, one, b1024, 0, v.stream, b.kept.get(), nv, b.unum.get());
  hipLaunchKernelGGL(scan_kernel<int32_t>, one, b1024, 0, v.stream, b.cnt.get(), nv, b.mstart.get());
  hipLaunchKernelGGL(scan_kernel<int64_t>, one, b1024, 0, v.stream, b.ulen.get(), nv, b.bstart.get());
  if (na > 0) hipLaunchKernelGGL(masks ? linkflag_kernel<true> : linkflag_kernel<false>, dim3(blocks256(na)), b256, 0, v.stream, na, a.rows.get(), removed,
                                 b.next.get(), b.islink.get());
  hipLaunchKernelGGL(scan_kernel<int32_t>, one, b1024, 0, v.stream, b.islink.get(), na, b.lstart.get());
  q.launched();
  return q.ok() ? MHAP_OK : q.fail(v, who);
}

// the tables for nu unitigs, nm members and nl links
int unitigs_tables(mhap_graph_session* s, const HandleView& v, const char* who, int64_t nu, int64_t nm, int64_t nl) {
  UnitigTables& t = s->ut;
  const char* w = "hipMalloc of the unitigs";
  Steps q{hipSuccess, v.stream};
  q.ensure_all(w, (size_t)std::max<int64_t>(nu, 1), t.u_start, t.u_len, t.u_circ);
  q.ensure_all(w, (size_t)std::max<int64_t>(nm, 1), t.m_vertex, t.m_offset, t.m_span, t.m_dst);
  q.ensure(t.links, 6 * (size_t)std::max<int64_t>(nl, 1), w);
  return q.ok() ? MHAP_OK : q.fail(v, who);
}

int unitigs_back(mhap_graph_session* s, const HandleView& v, const char* who, bool links) {
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  const UnitigBuild& b = s->ub;
  const UnitigTables& t = s->ut;
  const dim3 gv(blocks256(nv)), b256(256);
  const int cur = s->u_cur;
  hipLaunchKernelGGL(unitig_scatter_kernel, gv, b256, 0, v.stream, nv, b.kept.get(), b.unum.get(), b.mstart.get(), b.ulen.get(), b.cyc.get(),
                     t.u_start.get(), t.u_len.get(), t.u_circ.get());
  hipLaunchKernelGGL(member_scatter_kernel, gv, b256, 0, v.stream, nv, b.P[cur].get(), b.R[cur].get(), b.O[cur].get(), b.span.get(), b.kept.get(),
                     b.mstart.get(), b.bstart.get(), t.m_vertex.get(), t.m_offset.get(), t.m_span.get(), t.m_dst.get());
  if (links) hipLaunchKernelGGL(link_scatter_kernel, dim3(blocks256(na)), b256, 0, v.stream, na, s->arc.rows.get(), b.islink.get(), b.lstart.get(),
                                b.P[cur].get(), b.kept.get(), b.unum.get(), t.links.get());
  Steps q{hipSuccess, v.stream};
  q.launched();
  return q.ok() ? MHAP_OK : q.fail(v, who);
}

// The unitigs the copy and spell calls serve, built anew over what the masks leave; counts: MHAP_UNITIG_COUNTS.
int build_unitigs(mhap_graph_session* s, const HandleView& v, const char* who, const uint8_t* dropped, const uint8_t* removed, int64_t* counts) {
  s->n_unitigs = -1;
  s->unitig_gen++;
  const int64_t nv = 2 * s->n_reads, na = s->n_arcs;
  const UnitigBuild& b = s->ub;
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) counts[k] = s->last_counts[k] = 0;
  if (nv == 0) { s->n_unitigs = s->n_members = s->n_links = s->n_ubases = 0; return MHAP_OK; }
  int rc = unitigs_front(s, v, who, dropped, removed);
  if (rc != MHAP_OK) return rc;
  int64_t nu = 0, nm = 0, nb = 0, nl = 0;
  Steps q{hipSuccess, v.stream};
  q.fetch({{&nu, b.unum.get() + nv, 8}, {&nm, b.mstart.get() + nv, 8}, {&nb, b.bstart.get() + nv, 8}, {&nl, b.lstart.get() + na, 8}});
  if (!q.ok()) return q.fail(v, who);
  if ((rc = unitigs_tables(s, v, who, nu, nm, nl)) != MHAP_OK || (rc = unitigs_back(s, v, who, nl > 0)) != MHAP_OK) return rc;
  u64 hc[UC_DEVICE];
  q.fetch({{hc, b.ucounts.get(), sizeof hc}});
  if (!q.ok()) return q.fail(v, who);
  counts[0] = nu; counts[1] = (int64_t)hc[UC_CIRCULAR]; counts[2] = nm; counts[3] = (int64_t)hc[UC_JOINED]; counts[4] = nl;
  counts[5] = (int64_t)hc[UC_LONGEST]; counts[6] = nb;
  for (int k = 0; k < MHAP_UNITIG_COUNTS; k++) s->last_counts[k] = counts[k];
  s->n_members = nm; s->n_links = nl; s->n_ubases = nb;
  s->n_unitigs = nu;
  return MHAP_OK;
}

}  // namespace
}  // namespace mhap

using namespace mhap;

extern "C" int mhap_graph_unitigs(mhap_graph_session* s, int64_t* counts) {
  const char* who = "mhap_graph_unitigs";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) return s->null_arg(who);
  if (const int rc = s->need(who, NEED_FINISH); rc != MHAP_OK) return rc;
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
  if (!counts) return s->null_arg(who);
  mhap_clean_params p;
  mhap_graph_default_clean_params(&p);
  if (params) p = *params;
  if (p.tip_reads < 0 || p.bubble_bases < 0 || p.max_rounds < 1) {
    *v.err = std::string(who) + ": tip_reads and bubble_bases must be >= 0 and max_rounds >= 1";
    return MHAP_E_INVALID;
  }
  int rc = s->need(who, NEED_FINISH);
  if (rc != MHAP_OK) return rc;
  (void)hipSetDevice(v.device);
  s->n_unitigs = -1;
  s->cleaned = false;
  const int64_t nr = s->n_reads, nv = 2 * nr, na = s->n_arcs;
  const size_t rn = (size_t)std::max<int64_t>(nr, 1), an = (size_t)std::max<int64_t>(na, 1);
  CleanState& c = s->cl;
  const char* w = "hipMalloc of the clean state";
  Steps q{hipSuccess, v.stream};
  q.ensure_all(w, rn, c.dropped, c.verdict);
  q.ensure_all(w, 2 * rn, c.o_lo, c.o_hi, c.o_cand);
  q.ensure(c.removed, an, w); q.ensure(c.ccounts, MHAP_CLEAN_COUNTS, w);
  q.zero(c.dropped, rn); q.zero(c.removed, an); q.zero(c.ccounts, MHAP_CLEAN_COUNTS);   // every call starts again from the uncleaned graph
  if (!q.ok()) return q.fail(v, who);
  u64 hc[MHAP_CLEAN_COUNTS] = {0};
  int64_t rounds = 0;
  if (nv > 0) {
    // a round's tables at their largest: a unitig and a member per read, a link per arc
    if ((rc = unitigs_tables(s, v, who, nr, nr, na)) != MHAP_OK) return rc;
    const UnitigBuild& b = s->ub;
    const UnitigTables& t = s->ut;
    const dim3 gx(blocks256(nv)), gr(blocks256(nr)), b256(256);
    u64 before = 0;
    while (rounds < p.max_rounds) {
      if ((rc = unitigs_front(s, v, who, c.dropped.get(), c.removed.get())) != MHAP_OK || (rc = unitigs_back(s, v, who, na > 0)) != MHAP_OK) return rc;
      const UTables U{b.unum.get() + nv, b.mstart.get() + nv, b.lstart.get() + na, t.u_start.get(), t.u_len.get(), t.u_circ.get(), t.m_vertex.get(),
                      t.links.get()};
      hipLaunchKernelGGL(origin_kernel, gx, b256, 0, v.stream, U, s->arc.fstart.get(), c.o_lo.get(), c.o_hi.get());
      hipLaunchKernelGGL(degree_kernel, gx, b256, 0, v.stream, U, c.o_lo.get(), c.o_hi.get(), p.tip_reads, c.o_cand.get());
      hipLaunchKernelGGL(tip_kernel, gr, b256, 0, v.stream, U, c.o_lo.get(), c.o_hi.get(), c.o_cand.get(), c.verdict.get(), c.ccounts.get());
      hipLaunchKernelGGL(bubble_kernel, gr, b256, 0, v.stream, U, c.o_lo.get(), c.o_hi.get(), p.bubble_bases, c.verdict.get(), c.ccounts.get());
      hipLaunchKernelGGL(drop_kernel, gr, b256, 0, v.stream, U, c.verdict.get(), c.dropped.get(), c.ccounts.get());
      if (na > 0) hipLaunchKernelGGL(removed_kernel, dim3(blocks256(na)), b256, 0, v.stream, na, s->arc.rows.get(), c.dropped.get(), c.removed.get(),
                                     c.ccounts.get());
      q.launched();
      q.fetch({{hc, c.ccounts.get(), sizeof hc}});   // the one wait of a round: did it remove anything
      if (!q.ok()) return q.fail(v, who);
      rounds++;
      if (hc[CC_TIPS] + hc[CC_BUBBLES] == before) break;
      before = hc[CC_TIPS] + hc[CC_BUBBLES];
    }
  } else rounds = 1;
  int64_t uc[MHAP_UNITIG_COUNTS];
  if ((rc = build_unitigs(s, v, who, c.dropped.get(), c.removed.get(), uc)) != MHAP_OK) return rc;
  for (int k = 0; k < MHAP_CLEAN_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[CC_ROUNDS] = rounds;
  s->cleaned = true;
  return MHAP_OK;
}

extern "C" int mhap_graph_copy_dropped(mhap_graph_session* s, uint8_t* per_read) {
  if (!s) return MHAP_E_INVALID;
  return s->copy_out("mhap_graph_copy_dropped", NEED_CLEAN, s->n_reads, !per_read, {{per_read, s->cl.dropped.get(), (size_t)s->n_reads}});
}

extern "C" int mhap_graph_copy_removed(mhap_graph_session* s, uint8_t* per_arc) {
  if (!s) return MHAP_E_INVALID;
  return s->copy_out("mhap_graph_copy_removed", NEED_CLEAN, s->n_arcs, !per_arc, {{per_arc, s->cl.removed.get(), (size_t)s->n_arcs}});
}

extern "C" int mhap_graph_unitigs_info(const mhap_graph_session* s, int64_t* n_unitigs, int64_t* n_members, int64_t* n_links, int64_t* n_bases) {
  if (!s) return MHAP_E_INVALID;
  if (n_unitigs) *n_unitigs = s->n_unitigs;
  if (n_members) *n_members = s->n_unitigs < 0 ? 0 : s->n_members;
  if (n_links) *n_links = s->n_unitigs < 0 ? 0 : s->n_links;
  if (n_bases) *n_bases = s->n_unitigs < 0 ? 0 : s->n_ubases;
  return MHAP_OK;
}

extern "C" int mhap_graph_unitigs_counts(mhap_graph_session* s, int64_t* counts) {
  if (!s) return MHAP_E_INVALID;
  const int rc = s->copy_out("mhap_graph_unitigs_counts", NEED_UNITIGS, MHAP_UNITIG_COUNTS, !counts, {});   // (they are on the host)
  for (int k = 0; rc == MHAP_OK && k < MHAP_UNITIG_COUNTS; k++) counts[k] = s->last_counts[k];
  return rc;
}

extern "C" int mhap_graph_copy_unitigs(mhap_graph_session* s, int64_t* unitig_start, int64_t* unitig_len, uint8_t* circular) {
  const char* who = "mhap_graph_copy_unitigs";
  if (!s) return MHAP_E_INVALID;
  if (const int rc = s->need(who, NEED_UNITIGS); rc != MHAP_OK) return rc;
  if (!unitig_start) return s->null_arg(who);
  unitig_start[s->n_unitigs] = s->n_members;   // (before the other pointers are looked at: with no unitig it is all there is)
  const size_t n = (size_t)s->n_unitigs;
  return s->copy_out(who, NEED_UNITIGS, s->n_unitigs, !unitig_len || !circular,
                  {{unitig_start, s->ut.u_start.get(), 8 * n}, {unitig_len, s->ut.u_len.get(), 8 * n}, {circular, s->ut.u_circ.get(), n}});
}

extern "C" int mhap_graph_copy_layout(mhap_graph_session* s, int32_t* vertex, int64_t* offset, int32_t* span) {
  if (!s) return MHAP_E_INVALID;
  const size_t n = (size_t)s->n_members;
  return s->copy_out("mhap_graph_copy_layout", NEED_UNITIGS, s->n_members, !vertex || !offset || !span,
                  {{vertex, s->ut.m_vertex.get(), 4 * n}, {offset, s->ut.m_offset.get(), 8 * n}, {span, s->ut.m_span.get(), 4 * n}});
}

extern "C" int mhap_graph_copy_links(mhap_graph_session* s, int32_t* rows) {
  if (!s) return MHAP_E_INVALID;
  return s->copy_out("mhap_graph_copy_links", NEED_UNITIGS, s->n_links, !rows, {{rows, s->ut.links.get(), 24 * (size_t)s->n_links}});
}

extern "C" int mhap_graph_spell_device(mhap_graph_session* s, const uint8_t* d_bases, int64_t n_bases, const int64_t* offsets, uint8_t* out) {
  const char* who = "mhap_graph_spell";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (const int rc = s->need(who, NEED_UNITIGS); rc != MHAP_OK) return rc;
  if (n_bases < 0 || (s->n_reads > 0 && !offsets)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  for (int64_t r = 0; r < s->n_reads; r++)
    if (offsets[r] < 0 || offsets[r] > n_bases || (int64_t)s->lengths[(size_t)r] > n_bases - offsets[r]) {
      *v.err = std::string(who) + ": read " + std::to_string(r) + " is [" + std::to_string(offsets[r]) + ", " +
               std::to_string(offsets[r] + s->lengths[(size_t)r]) + ") of " + std::to_string(n_bases) + " bases";
      return MHAP_E_INVALID;
    }
  if (s->n_ubases == 0) return MHAP_OK;
  if (!d_bases || !out) return s->null_arg(who);
  (void)hipSetDevice(v.device);
  SpellStage& sp = s->sp;
  Steps q{hipSuccess, v.stream};
  q.ensure(sp.roff, (size_t)s->n_reads); q.ensure(sp.spelled, (size_t)s->n_ubases);
  q.upload(sp.roff.get(), offsets, 8 * (size_t)s->n_reads);
  if (!q.ok()) return q.fail(v, who);
  const int64_t tiles = (s->n_ubases + SPELL_CHUNK - 1) / SPELL_CHUNK;
  if (tiles > INT32_MAX) { (void)hipStreamSynchronize(v.stream); *v.err = std::string(who) + ": more than 2^31 - 1 tiles of output"; return MHAP_E_INVALID; }
  hipLaunchKernelGGL(spell_kernel, dim3((unsigned)tiles), dim3(SPELL_T), 0, v.stream, d_bases, n_bases, sp.roff.get(), (const int32_t*)s->d_lengths.p,
                     s->n_members, s->ut.m_vertex.get(), s->ut.m_span.get(), s->ut.m_dst.get(), s->n_ubases, sp.spelled.get());
  q.launched();
  q.fetch({{out, sp.spelled.get(), (size_t)s->n_ubases}});
  if (!q.ok()) { (void)hipStreamSynchronize(v.stream); return q.fail(v, who); }   // (the upload may still read `offsets`)
  return MHAP_OK;
}

extern "C" int mhap_graph_spell(mhap_graph_session* s, const uint8_t* bases, int64_t n_bases, const int64_t* offsets, uint8_t* out) {
  const char* who = "mhap_graph_spell";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (const int rc = s->need(who, NEED_UNITIGS); rc != MHAP_OK) return rc;
  if (n_bases < 0 || (n_bases > 0 && !bases)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  Steps q{hipSuccess, v.stream};
  q.ensure(s->sp.bases, (size_t)std::max<int64_t>(n_bases, 1), "hipMalloc of the bases");
  if (n_bases > 0) {   // (waited for: the caller's bytes are free when the call returns, whatever it returns)
    q.upload(s->sp.bases.get(), bases, (size_t)n_bases);
    if (q.ok()) q.step("upload", hipStreamSynchronize(v.stream));
  }
  if (!q.ok()) return q.fail(v, who);
  return mhap_graph_spell_device(s, s->sp.bases.get(), n_bases, offsets, out);
}
