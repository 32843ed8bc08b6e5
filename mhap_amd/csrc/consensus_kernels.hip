// consensus_kernels.hip — the consensus of the served unitigs (mhap_consensus_begin / _add / _run / _copy* / _quality / _votes / _free): every read
// is placed on a unitig, aligned to the draft in a band round its place, votes as view A of the correction contract, and every draft
// position takes the majority.  The contract is the "unitig consensus" section of include/mhap_hip.h; tests/unitig_consensus_ref.py
// restates it.  The class rule is graph_class.hpp's (classify_kernel's), the column walk, its vote kernel, the scan of emitted lengths
// and the decision vote_common.hpp's (the correction's), the aligner mhap_align_pairs_banded_paths, unchanged.
//
// add: the host finds every record's reads as mhap_graph_add does and appends the packed records (32 bytes, GItem) to one device array.
// run, in order, all on the handle's stream:
//   member_kernel    one lane per member: the read's vertex, unitig and offset (an exact placement)
//   place_kernel<1>  one lane per record: the class, which of the two reads is the member M, the frame turned into M's unitig
//                    orientation, the candidate p; atomicMax per read X of (xe - xs) << 32 | (2^31 - 1 - vertex of M)
//   place_kernel<2>  the same lanes: a record whose key is the read's maximum does atomicMin of (p + 2^61) << 1 | sX
//   plan_kernel      one lane per read: the row of the placement table (p reduced modulo the length on a circular unitig) and the
//                    pair row {a_off, a_len, b_off, b_len, b_rc, diag, band} over the array "reads, then drafts"; an unplaced read and
//                    an empty window get an empty pair
//   guard_kernel     one lane per read: +1 on every tile of MHAP_CONSENSUS_TILE draft positions its window meets; the host refuses the
//                    run when a tile is above the cap, before any vote
//   (the aligner)    the pair rows go down, through mhap_align_pairs_banded_paths over the host copy of reads and drafts, and the runs
//                    come up again, 4 bytes each, with one VoteItem per aligned pair: view A, target the unitig, i0 = w0 + read_begin
//   vote_kernel      vote_common.hpp's, <true, Weigh>: one wave per aligned pair over vote_walk, into a table of 12 planes per unitig
//                    (48 bytes per draft base)
//   ccall_kernel     one workgroup per tile, 256 positions at a time: decide() per thread, a workgroup scan of the emitted lengths; the
//                    first launch leaves every tile's length and four counts, the host prefix-sums the lengths, the second launch writes
//                    the bytes and the position map.  The junction after t belongs to t's tile; t < L - 1 is the unitig's L.
// quality, on request after a run:
//   cqual_kernel     one workgroup per tile: decide() and decide_quality() per position, the bytes' places from the position map
// A session begun with qualities ("quality-weighted votes") runs the same kernels over weighted_vote.hpp's policies: the reads' bytes
// vote with QualityWeight, and ccall_kernel and cqual_kernel count a draft byte with NeutralWeight.
// Integer atomic rates behind the vote layout are not measured here either (correct_kernels.hip).
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "graph_class.hpp"
#include "mhap_internal.hpp"
#include "vote_common.hpp"
#include "vote_table.hpp"
#include "weighted_vote.hpp"

namespace mhap {
namespace {

constexpr int CT = MHAP_CONSENSUS_TILE;
constexpr int64_t P_BIAS = (int64_t)1 << 61;   // added to a candidate p before it is compared as unsigned
constexpr uint32_t V_TOP = 0x7FFFFFFFu;        // key 1 holds V_TOP - vertex, so that the smallest vertex is the greatest key
enum { HOW_MEMBER = 0, HOW_RECORD = 1, HOW_UNPLACED = 2 };
enum { CC_MEMBERS = 0, CC_BY_RECORD, CC_UNPLACED, CC_ALIGNED, CC_NO_ALIGNMENT, CC_BASES_IN, CC_BASES_OUT, CC_SUB, CC_DEL, CC_INS, CC_LOW };

__device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ inline int64_t floor_half(int64_t x) { return (x - (x < 0 ? 1 : 0)) / 2; }
__device__ inline int64_t floor_mod(int64_t x, int64_t m) { const int64_t r = x % m; return r < 0 ? r + m : r; }

// the last k with start[k] <= x, start ascending with start[0] <= x
__device__ inline int64_t last_at_or_before(const int64_t* __restrict__ start, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (start[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void member_kernel(int64_t nm, int64_t nu, const int64_t* __restrict__ u_start, const int32_t* __restrict__ m_vertex,
                                                     const int64_t* __restrict__ m_offset, int32_t* __restrict__ mem_vertex,
                                                     int32_t* __restrict__ mem_unitig, int64_t* __restrict__ mem_off) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= nm) return;
  const int32_t v = m_vertex[m];
  const int32_t r = v >> 1;   // (a read is a member of one unitig, on one strand: one writer)
  mem_vertex[r] = v;
  mem_unitig[r] = (int32_t)last_at_or_before(u_start, nu, m);
  mem_off[r] = m_offset[m];
}

template <int PASS>
__global__ __launch_bounds__(256) void place_kernel(const int4* __restrict__ items, int64_t n, const int32_t* __restrict__ lengths, GParams P,
                                                    const int32_t* __restrict__ mem_vertex, const int64_t* __restrict__ mem_off,
                                                    unsigned long long* __restrict__ key1, unsigned long long* __restrict__ key2) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
  const int32_t A = w0.x, B = w0.y >> 1, o = w0.y & 1;
  GGeom g;
  const int c = graph_class(A, B, o, w0.z, w0.w, w1.x, w1.y, __hiloint2double(w1.w, w1.z), lengths[A], lengths[B], P, g);
  if (c == G_NONE || c == G_INTERNAL) return;
  const bool a_member = mem_vertex[A] >= 0, b_member = mem_vertex[B] >= 0;
  if (a_member == b_member) return;   // two members place nobody, and neither do two non-members
  const int32_t M = a_member ? A : B, X = a_member ? B : A, vm = mem_vertex[M];
  // the aligner's frame: A forward over [qs, qe), B with strand o over [ts, te); turned round when M's strand there is not its unitig's
  int64_t as = g.qs, ae = g.qe, bs = g.ts, be = g.te;
  int sa = 0, sb = o;
  if ((a_member ? sa : sb) != (vm & 1)) {
    const int64_t as2 = g.ql - ae, ae2 = g.ql - as, bs2 = g.tl - be, be2 = g.tl - bs;
    as = as2; ae = ae2; bs = bs2; be = be2;
    sa ^= 1; sb ^= 1;
  }
  const int64_t ms = a_member ? as : bs, me = a_member ? ae : be, xs = a_member ? bs : as, xe = a_member ? be : ae;
  const int sx = a_member ? sb : sa;
  if (xe - xs < 1) return;   // (an alignment has at least one column)
  const int64_t p = floor_half(2 * mem_off[M] + ms + me - xs - xe);
  const unsigned long long k1 = (unsigned long long)(xe - xs) << 32 | (unsigned long long)(V_TOP - (uint32_t)vm);
  if (PASS == 1) atomicMax(key1 + X, k1);
  else if (key1[X] == k1) atomicMin(key2 + X, (unsigned long long)(p + P_BIAS) << 1 | (unsigned long long)sx);
}

__global__ __launch_bounds__(256) void plan_kernel(int64_t nr, const int32_t* __restrict__ lengths, const int64_t* __restrict__ roff,
                                                   const int32_t* __restrict__ mem_vertex, const int32_t* __restrict__ mem_unitig,
                                                   const int64_t* __restrict__ mem_off, const unsigned long long* __restrict__ key1,
                                                   const unsigned long long* __restrict__ key2, const int64_t* __restrict__ u_len,
                                                   const uint8_t* __restrict__ u_circ, const int64_t* __restrict__ ubase, int64_t n_bases,
                                                   int32_t band_given, double max_shift, int64_t* __restrict__ place, int64_t* __restrict__ pairs) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nr) return;
  int64_t k = -1, strand = 0, p = 0, how = HOW_UNPLACED;
  const int32_t v = mem_vertex[r];
  if (v >= 0) { k = mem_unitig[r]; strand = v & 1; p = mem_off[r]; how = HOW_MEMBER; }
  else if (key1[r] != 0) {
    const uint32_t vm = V_TOP - (uint32_t)(key1[r] & 0xFFFFFFFFull);
    const unsigned long long k2 = key2[r];
    k = mem_unitig[vm >> 1]; strand = (int64_t)(k2 & 1ull); p = (int64_t)(k2 >> 1) - P_BIAS; how = HOW_RECORD;
    if (u_circ[k]) p = floor_mod(p, u_len[k]);
  }
  int64_t* row = place + 5 * r;
  row[0] = k; row[1] = strand; row[2] = p; row[3] = how; row[4] = 0;
  int64_t* pr = pairs + 7 * r;
  const int64_t len = lengths[r];
  const int64_t band = band_given > 0 ? band_given : max64(1, (int64_t)(int)((double)len * max_shift));
  int64_t a_off = 0, a_len = 0, b_off = 0, b_len = 0, diag = 0;
  if (how != HOW_UNPLACED) {
    const int64_t w0 = max64(0, p - band), w1 = min64(u_len[k], p + len + band);
    if (w1 > w0) { a_off = n_bases + ubase[k] + w0; a_len = w1 - w0; b_off = roff[r]; b_len = len; diag = w0 - p; }
  }
  pr[0] = a_off; pr[1] = a_len; pr[2] = b_off; pr[3] = b_len; pr[4] = a_len > 0 ? strand : 0; pr[5] = diag; pr[6] = band;
}

__global__ __launch_bounds__(256) void guard_kernel(int64_t nr, const int64_t* __restrict__ place, const int64_t* __restrict__ pairs,
                                                    const int64_t* __restrict__ ubase, const int64_t* __restrict__ utile, int64_t n_bases,
                                                    int64_t n_tiles, uint32_t* __restrict__ tile_reads) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= nr) return;
  const int64_t k = place[5 * r], a_len = pairs[7 * r + 1];
  if (k < 0 || a_len <= 0) return;
  const int64_t w0 = pairs[7 * r] - n_bases - ubase[k];
  for (int64_t j = w0 / CT; j <= (w0 + a_len - 1) / CT; j++)
    if (utile[k] + j < n_tiles) atomicAdd(tile_reads + utile[k] + j, 1u);
}

// tile_off == nullptr: count only (tile_len, tile_counts); else write the bytes at tile_off[tile] and the position map.
// Weigh: what a draft byte weighs — UnitWeight, or in a weighted session ("quality-weighted votes" in include/mhap_hip.h) the
// NeutralWeight, because a draft byte has no single quality.
template <class Weigh>
__global__ __launch_bounds__(CK_T) void ccall_kernel(const uint8_t* __restrict__ draft, int64_t nu, const int64_t* __restrict__ u_len,
                                                     const int64_t* __restrict__ ubase, const int64_t* __restrict__ utile,
                                                     const uint32_t* __restrict__ table, int min_cov, int32_t* __restrict__ tile_len,
                                                     int32_t* __restrict__ tile_counts, const int64_t* __restrict__ tile_off,
                                                     const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ out, int64_t* __restrict__ posmap) {
  const Weigh own_weight{};
  __shared__ int acc[4];   // n_sub, n_del, n_ins, n_low
  const int64_t tile = blockIdx.x;
  const int64_t k = last_at_or_before(utile, nu, tile);   // (every unitig has at least one tile)
  const int64_t L = u_len[k], t_begin = (tile - utile[k]) * CT, t_end = min64(L, t_begin + CT);
  const uint8_t* own = draft + ubase[k];
  const uint32_t* w = table + (int64_t)CK_WORDS * ubase[k];
  const int tid = threadIdx.x;
  if (tid < 4) acc[tid] = 0;
  int64_t written = 0;
  int my[4] = {0, 0, 0, 0};
  for (int64_t t0 = t_begin; t0 < t_end; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    if (t < t_end) D = decide<Weigh::neutral>(w, L, t, own[t], own_weight(ubase[k] + t), min_cov);
    my[0] += D.sub; my[1] += D.del; my[2] += D.ins; my[3] += D.low;
    const EmitScan sc = scan_emitted(D.n);
    if (tile_off && t < t_end) {
      const int64_t at = tile_off[tile] + written + sc.before + (sc.incl - D.n);
      posmap[ubase[k] + t] = at - out_offsets[k];
      for (int u = 0; u < D.n; u++) out[at + u] = D.bytes[u];
    }
    written += sc.tile;
  }
  __syncthreads();
  for (int u = 0; u < 4; u++) if (my[u]) atomicAdd(&acc[u], my[u]);
  __syncthreads();
  if (tid == 0 && !tile_off) {
    tile_len[tile] = (int32_t)written;
    for (int u = 0; u < 4; u++) tile_counts[4 * tile + u] = acc[u];
  }
}

// The quality pass of mhap_consensus_quality, over the table, the offsets and the position map of a completed run: one workgroup per
// tile as in ccall_kernel, decide() and decide_quality() per position.  A kernel of its own, so that ccall_kernel carries no quality;
// it needs no scan, because the run's position map already says where a position's bytes lie.  One writer per quality byte; the
// workgroup's histogram lives in LDS and leaves by one 64-bit atomic per non-empty bin.
template <class Weigh>
__global__ __launch_bounds__(CK_T) void cqual_kernel(const uint8_t* __restrict__ draft, int64_t nu, const int64_t* __restrict__ u_len,
                                                     const int64_t* __restrict__ ubase, const int64_t* __restrict__ utile,
                                                     const uint32_t* __restrict__ table, int min_cov, int per_vote, int cap,
                                                     const int64_t* __restrict__ out_offsets, const int64_t* __restrict__ posmap,
                                                     uint8_t* __restrict__ quals, unsigned long long* __restrict__ hist) {
  __shared__ unsigned long long bins[QUAL_BINS];
  constexpr int U = Weigh::neutral;
  const Weigh own_weight{};
  const int64_t tile = blockIdx.x;
  const int64_t k = last_at_or_before(utile, nu, tile);
  const int64_t L = u_len[k], t_begin = (tile - utile[k]) * CT, t_end = min64(L, t_begin + CT);
  const uint8_t* own = draft + ubase[k];
  const uint32_t* w = table + (int64_t)CK_WORDS * ubase[k];
  const int64_t o_end = out_offsets[k + 1];
  const int tid = threadIdx.x;
  if (tid < QUAL_BINS) bins[tid] = 0ull;
  __syncthreads();
  for (int64_t t = t_begin + tid; t < t_end; t += CK_T) {
    const int own_w = own_weight(ubase[k] + t);
    const Decision D = decide<U>(w, L, t, own[t], own_w, min_cov);
    uint8_t q[1 + CK_KI] = {0, 0, 0, 0, 0};
    decide_quality<U>(w, L, t, own[t], own_w, D, per_vote, cap, q);
    const int64_t at = out_offsets[k] + posmap[ubase[k] + t];
    for (int u = 0; u < D.n; u++)
      if (at + u < o_end) {   // (the map is that of this table and this min_cov: always)
        quals[at + u] = q[u];
        atomicAdd(&bins[q[u]], 1ull);
      }
  }
  __syncthreads();
  if (tid < QUAL_BINS && bins[tid]) atomicAdd(hist + tid, bins[tid]);
}

// the cap on reads per tile: 65 535, lowered by MHAP_CONSENSUS_TILE_CAP (tests), read at each run
uint32_t tile_cap() {
  if (const char* e = getenv("MHAP_CONSENSUS_TILE_CAP")) {
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end != e && *end == '\0' && v >= 1 && v < (long)CK_CAP) return (uint32_t)v;
  }
  return CK_CAP;
}

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_consensus_session {
  mhap_graph_session* g = nullptr;
  mhap_handle* h = nullptr;
  uint64_t gen = 0;                                       // the graph's unitig generation at begin
  int32_t band = 0, min_cov = 4;
  int64_t n_reads = 0, n_bases = 0, n_items = 0;
  std::vector<int64_t> offsets;
  std::vector<uint8_t> host_bases;                        // the reads, then (from a run on) the drafts: what the aligner is given
  bool weighted = false;                                  // begun with qualities: the w* kernels, WK_CAP reads per tile
  Weights W{0, 0};
  // the last run; n_unitigs < 0: none has completed
  int64_t n_unitigs = -1, n_draft = 0, out_bytes = 0;
  double seconds[4] = {0, 0, 0, 0};                       // the host's wall time of the last run: placement, alignment, vote, call
  std::vector<int64_t> u_len, ubase, out_offsets, stats, place;
  DevBuf bases, roff, items, rlen, mem_vertex, mem_unitig, mem_off, key1, key2, d_place, d_pairs, d_ustart, d_ulen, d_ucirc, d_ubase,
      d_utile, m_vertex, m_offset, tile_reads, table, vitems, ops, tile_len, tile_counts, tile_off, d_outoff, out, posmap, quals, hist, in_quals;
  void release() {
    for (DevBuf* b : {&bases, &roff, &items, &rlen, &mem_vertex, &mem_unitig, &mem_off, &key1, &key2, &d_place, &d_pairs, &d_ustart, &d_ulen,
                       &d_ucirc, &d_ubase, &d_utile, &m_vertex, &m_offset, &tile_reads, &table, &vitems, &ops, &tile_len, &tile_counts, &tile_off,
                       &d_outoff, &out, &posmap, &quals, &hist, &in_quals}) b->release();
  }
};

namespace {

// the session of any call after begin: its graph must still serve the unitigs it served at begin
int still_valid(mhap_consensus_session* s, const HandleView& v, const char* who) {
  if (graph_view(s->g).unitig_gen == s->gen) return MHAP_OK;
  *v.err = std::string(who) + ": the graph session has run mhap_graph_finish, mhap_graph_unitigs or mhap_graph_clean since mhap_consensus_begin";
  return MHAP_E_INVALID;
}

int need_run(mhap_consensus_session* s, const HandleView& v, const char* who) {
  const int rc = still_valid(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (s->n_unitigs >= 0) return MHAP_OK;
  *v.err = std::string(who) + ": no mhap_consensus_run has completed";
  return MHAP_E_INVALID;
}

}  // namespace

extern "C" void mhap_consensus_default_params(mhap_consensus_params* p) {
  if (!p) return;
  p->band = 0; p->min_cov = 4;
}

// the begin behind mhap_consensus_begin (qualities == nullptr) and mhap_consensus_begin_weighted
static int consensus_begin(const char* who, mhap_graph_session* g, const uint8_t* bases, const uint8_t* qualities, int64_t n_bases,
                           const int64_t* offsets, const mhap_consensus_params* params, const mhap_weight_params* weights,
                           mhap_consensus_session** session) {
  if (session) *session = nullptr;
  if (!g) return MHAP_E_INVALID;
  const GraphView gv = graph_view(g);
  HandleView v = handle_view(gv.h);
  if (!session || n_bases < 0 || (n_bases > 0 && !bases) || (gv.n_reads > 0 && !offsets)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  mhap_consensus_params p;
  mhap_consensus_default_params(&p);
  if (params) p = *params;
  if (p.band < 0 || p.min_cov < 1) { *v.err = std::string(who) + ": band must be >= 0 and min_cov >= 1"; return MHAP_E_INVALID; }
  for (int64_t r = 0; r < gv.n_reads; r++)
    if (offsets[r] < 0 || gv.lengths[r] > n_bases - offsets[r]) {
      *v.err = std::string(who) + ": read " + std::to_string(r) + " lies outside the " + std::to_string(n_bases) + " bases";
      return MHAP_E_INVALID;
    }
  mhap_weight_params wp;
  mhap_weight_default_params(&wp);
  if (qualities && weights) wp = *weights;
  if (qualities && !weight_params_ok(wp.q_lo, wp.q_hi, who, *v.err)) return MHAP_E_INVALID;
  mhap_consensus_session* s = new mhap_consensus_session();
  s->g = g; s->h = gv.h; s->gen = gv.unitig_gen; s->band = p.band; s->min_cov = p.min_cov;
  s->weighted = qualities != nullptr; s->W = Weights{wp.q_lo, wp.q_hi};
  s->n_reads = gv.n_reads; s->n_bases = n_bases;
  s->offsets.assign(offsets, offsets + gv.n_reads);
  s->host_bases.assign(bases, bases + n_bases);
  (void)hipSetDevice(v.device);
  const size_t rb = (size_t)std::max<int64_t>(gv.n_reads, 1);
  hipError_t e = s->roff.ensure(8 * rb);
  if (e == hipSuccess && gv.n_reads > 0) e = hipMemcpyAsync(s->roff.p, s->offsets.data(), 8 * (size_t)gv.n_reads, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess && s->weighted) e = s->in_quals.ensure((size_t)std::max<int64_t>(n_bases, 1));
  if (e == hipSuccess && s->weighted && n_bases > 0) e = hipMemcpyAsync(s->in_quals.p, qualities, (size_t)n_bases, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
  if (e != hipSuccess) { s->release(); delete s; return hip_fail(v, who, "the table of reads", e); }
  *session = s;
  return MHAP_OK;
}

extern "C" int mhap_consensus_begin(mhap_graph_session* g, const uint8_t* bases, int64_t n_bases, const int64_t* offsets,
                                    const mhap_consensus_params* params, mhap_consensus_session** session) {
  return consensus_begin("mhap_consensus_begin", g, bases, nullptr, n_bases, offsets, params, nullptr, session);
}

extern "C" int mhap_consensus_begin_weighted(mhap_graph_session* g, const uint8_t* bases, const uint8_t* qualities, int64_t n_bases,
                                             const int64_t* offsets, const mhap_consensus_params* params, const mhap_weight_params* weights,
                                             mhap_consensus_session** session) {
  return consensus_begin(qualities ? "mhap_consensus_begin_weighted" : "mhap_consensus_begin", g, bases, qualities, n_bases, offsets, params, weights,
                         session);
}

extern "C" int mhap_consensus_add(mhap_consensus_session* s, const mhap_record* recs, int64_t n) {
  const char* who = "mhap_consensus_add";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = still_valid(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (n < 0 || (n > 0 && !recs)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (s->n_items + n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  std::vector<GItem> items;
  if (!graph_pack_records(s->g, who, recs, n, items, *v.err)) return MHAP_E_INVALID;
  (void)hipSetDevice(v.device);
  hipError_t e = s->items.ensure(sizeof(GItem) * (size_t)(s->n_items + n), true, v.stream);
  if (e != hipSuccess) return hip_fail(v, who, "hipMalloc of the records (32 bytes each)", e);
  e = hipMemcpyAsync(s->items.as<GItem>() + s->n_items, items.data(), sizeof(GItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);   // (the packed records go when the call returns)
  if (e != hipSuccess) return hip_fail(v, who, "upload", e);
  s->n_items += n;
  return MHAP_OK;
}

extern "C" int mhap_consensus_run(mhap_consensus_session* s, int64_t* counts) {
  const char* who = "mhap_consensus_run";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = still_valid(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  const GraphView gv = graph_view(s->g);
  if (gv.n_unitigs < 0) { *v.err = std::string(who) + ": the graph session serves no unitigs (mhap_graph_unitigs or mhap_graph_clean first)"; return MHAP_E_INVALID; }
  s->n_unitigs = -1;
  for (int k = 0; k < MHAP_CONSENSUS_COUNTS; k++) counts[k] = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = now();
  auto lap = [&](int stage) { const double t = now(); s->seconds[stage] = t - t_mark; t_mark = t; };   // (every stage ends behind a wait for the stream)
  int64_t nu = 0, nm = 0, nd = 0;
  (void)mhap_graph_unitigs_info(s->g, &nu, &nm, nullptr, &nd);
  const int64_t nr = s->n_reads;
  // the served unitigs and their draft, through the graph session's own calls
  std::vector<int64_t> u_start((size_t)nu + 1), u_len((size_t)nu), m_offset((size_t)nm);
  std::vector<uint8_t> u_circ((size_t)nu);
  std::vector<int32_t> m_vertex((size_t)nm), m_span((size_t)nm);
  if ((rc = mhap_graph_copy_unitigs(s->g, u_start.data(), u_len.data(), u_circ.data())) != MHAP_OK) return rc;
  if ((rc = mhap_graph_copy_layout(s->g, m_vertex.data(), m_offset.data(), m_span.data())) != MHAP_OK) return rc;
  std::vector<int64_t> ubase((size_t)nu + 1, 0), utile((size_t)nu + 1, 0);
  for (int64_t k = 0; k < nu; k++) {
    if (u_len[(size_t)k] >= ((int64_t)1 << 31)) {
      *v.err = std::string(who) + ": unitig " + std::to_string(k) + " has " + std::to_string(u_len[(size_t)k]) + " bases, 2^31 or more";
      return MHAP_E_INVALID;
    }
    ubase[(size_t)k + 1] = ubase[(size_t)k] + u_len[(size_t)k];
    utile[(size_t)k + 1] = utile[(size_t)k] + (u_len[(size_t)k] + CT - 1) / CT;
  }
  const int64_t n_tiles = utile[(size_t)nu];
  if (n_tiles > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 tiles"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e = hipSuccess;
  auto fail = [&](const char* what) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, what, e); };
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    if (e == hipSuccess) e = b.ensure(std::max<size_t>(bytes, 8));
    if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, v.stream);
  };
  s->host_bases.resize((size_t)(s->n_bases + nd));
  if ((e = s->bases.ensure((size_t)std::max<int64_t>(s->n_bases + nd, 1))) != hipSuccess) return fail("hipMalloc of the reads and the drafts");
  if (s->n_bases > 0 && (e = hipMemcpyAsync(s->bases.p, s->host_bases.data(), (size_t)s->n_bases, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail("upload");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("upload");
  if ((rc = mhap_graph_spell_device(s->g, s->bases.as<uint8_t>(), s->n_bases, s->offsets.data(), s->host_bases.data() + s->n_bases)) != MHAP_OK) return rc;
  if (nd > 0 && (e = hipMemcpyAsync(s->bases.as<uint8_t>() + s->n_bases, s->host_bases.data() + s->n_bases, (size_t)nd, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail("upload");
  up(s->d_ustart, u_start.data(), 8 * (size_t)(nu + 1));
  up(s->d_ulen, u_len.data(), 8 * (size_t)nu);
  up(s->d_ucirc, u_circ.data(), (size_t)nu);
  up(s->d_ubase, ubase.data(), 8 * (size_t)(nu + 1));
  up(s->d_utile, utile.data(), 8 * (size_t)(nu + 1));
  up(s->m_vertex, m_vertex.data(), 4 * (size_t)nm);
  up(s->m_offset, m_offset.data(), 8 * (size_t)nm);
  const size_t rb = (size_t)std::max<int64_t>(nr, 1), tb = (size_t)std::max<int64_t>(n_tiles, 1), db = (size_t)std::max<int64_t>(nd, 1);
  for (DevBuf* b : {&s->mem_off, &s->key1, &s->key2}) if (e == hipSuccess) e = b->ensure(8 * rb);
  for (DevBuf* b : {&s->mem_vertex, &s->mem_unitig}) if (e == hipSuccess) e = b->ensure(4 * rb);
  if (e == hipSuccess) e = s->d_place.ensure(40 * rb);
  if (e == hipSuccess) e = s->d_pairs.ensure(56 * rb);
  if (e == hipSuccess) e = s->tile_reads.ensure(4 * tb);
  if (e == hipSuccess) e = s->tile_len.ensure(4 * tb);
  if (e == hipSuccess) e = s->tile_counts.ensure(16 * tb);
  if (e == hipSuccess) e = s->tile_off.ensure(8 * tb);
  if (e == hipSuccess) e = s->d_outoff.ensure(8 * ((size_t)nu + 1));
  if (e == hipSuccess) e = s->posmap.ensure(8 * db);
  if (e == hipSuccess) e = s->table.ensure(4 * (size_t)CK_WORDS * db);
  if (e == hipSuccess) e = hipMemsetAsync(s->mem_vertex.p, 0xFF, 4 * rb, v.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->mem_unitig.p, 0xFF, 4 * rb, v.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->key1.p, 0, 8 * rb, v.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->key2.p, 0xFF, 8 * rb, v.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s->tile_reads.p, 0, 4 * tb, v.stream);
  if (e != hipSuccess) return fail("the tables of a run (132 bytes per read, 57 per draft base, 32 per tile)");
  const GParams P = gv.P;
  if (nm > 0) hipLaunchKernelGGL(member_kernel, dim3(blocks256(nm)), dim3(256), 0, v.stream, nm, nu, s->d_ustart.as<int64_t>(), s->m_vertex.as<int32_t>(),
                                 s->m_offset.as<int64_t>(), s->mem_vertex.as<int32_t>(), s->mem_unitig.as<int32_t>(), s->mem_off.as<int64_t>());
  if ((e = s->rlen.ensure(4 * rb)) != hipSuccess) return fail("hipMalloc");
  if (nr > 0 && (e = hipMemcpyAsync(s->rlen.p, gv.lengths, 4 * (size_t)nr, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return fail("upload");
  const int32_t* d_lengths = s->rlen.as<int32_t>();
  if (s->n_items > 0) {
    hipLaunchKernelGGL(place_kernel<1>, dim3(blocks256(s->n_items)), dim3(256), 0, v.stream, s->items.as<int4>(), s->n_items, d_lengths, P,
                       s->mem_vertex.as<int32_t>(), s->mem_off.as<int64_t>(), s->key1.as<unsigned long long>(), s->key2.as<unsigned long long>());
    hipLaunchKernelGGL(place_kernel<2>, dim3(blocks256(s->n_items)), dim3(256), 0, v.stream, s->items.as<int4>(), s->n_items, d_lengths, P,
                       s->mem_vertex.as<int32_t>(), s->mem_off.as<int64_t>(), s->key1.as<unsigned long long>(), s->key2.as<unsigned long long>());
  }
  std::vector<int64_t> place((size_t)nr * 5), pairs((size_t)nr * 7);
  std::vector<uint32_t> tile_reads((size_t)n_tiles);
  if (nr > 0) {
    hipLaunchKernelGGL(plan_kernel, dim3(blocks256(nr)), dim3(256), 0, v.stream, nr, d_lengths, s->roff.as<int64_t>(), s->mem_vertex.as<int32_t>(),
                       s->mem_unitig.as<int32_t>(), s->mem_off.as<int64_t>(), s->key1.as<unsigned long long>(), s->key2.as<unsigned long long>(),
                       s->d_ulen.as<int64_t>(), s->d_ucirc.as<uint8_t>(), s->d_ubase.as<int64_t>(), s->n_bases, s->band, v.max_shift,
                       s->d_place.as<int64_t>(), s->d_pairs.as<int64_t>());
    hipLaunchKernelGGL(guard_kernel, dim3(blocks256(nr)), dim3(256), 0, v.stream, nr, s->d_place.as<int64_t>(), s->d_pairs.as<int64_t>(),
                       s->d_ubase.as<int64_t>(), s->d_utile.as<int64_t>(), s->n_bases, n_tiles, s->tile_reads.as<uint32_t>());
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
    if ((e = hipMemcpyAsync(place.data(), s->d_place.p, 40 * (size_t)nr, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(pairs.data(), s->d_pairs.p, 56 * (size_t)nr, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  }
  if (n_tiles > 0 && (e = hipMemcpyAsync(tile_reads.data(), s->tile_reads.p, 4 * (size_t)n_tiles, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("the placement kernels");
  const uint32_t cap = s->weighted ? std::min<uint32_t>(tile_cap(), WK_CAP) : tile_cap();   // (a view adds up to 3 to a counter)
  for (int64_t k = 0; k < nu; k++)
    for (int64_t j = utile[(size_t)k]; j < utile[(size_t)k + 1]; j++)
      if (tile_reads[(size_t)j] > cap) {
        *v.err = std::string(who) + ": unitig " + std::to_string(k) + " tile " + std::to_string(j - utile[(size_t)k]) + " is met by " +
                 std::to_string(tile_reads[(size_t)j]) + " reads, more than " + std::to_string(cap);
        return MHAP_E_INVALID;
      }
  lap(0);
  // align every placed read to its window of the draft
  std::vector<int32_t> results((size_t)nr * 7);
  mhap_align_paths* paths = nullptr;
  if (nr > 0 && (rc = mhap_align_pairs_banded_paths(s->h, s->host_bases.data(), s->n_bases + nd, pairs.data(), nr, results.data(), &paths)) != MHAP_OK) return rc;
  lap(1);
  std::vector<VoteItem> vitems;
  for (int64_t r = 0; r < nr; r++) {
    int64_t* row = place.data() + 5 * r;
    if (row[3] == HOW_UNPLACED) { counts[CC_UNPLACED]++; continue; }
    counts[row[3] == HOW_MEMBER ? CC_MEMBERS : CC_BY_RECORD]++;
    const int64_t o0 = paths->offsets[(size_t)r], o1 = paths->offsets[(size_t)r + 1];
    if (o1 == o0) { counts[CC_NO_ALIGNMENT]++; continue; }
    counts[CC_ALIGNED]++;
    row[4] = 1;
    const int64_t k = row[0], w0 = pairs[(size_t)(7 * r)] - s->n_bases - ubase[(size_t)k];
    VoteItem it{};
    it.a_off = 0; it.b_off = s->offsets[(size_t)r];
    it.v_words = (int64_t)CK_WORDS * ubase[(size_t)k];
    it.ops_off = o0; it.alen = (int32_t)u_len[(size_t)k]; it.blen = gv.lengths[r];
    it.i0 = (int32_t)(w0 + results[(size_t)(7 * r + 1)]); it.j0 = results[(size_t)(7 * r + 3)];
    it.n_ops = (int32_t)(o1 - o0); it.view = 0; it.rc = (int32_t)row[1];
    vitems.push_back(it);
  }
  if (nd > 0 && (e = hipMemsetAsync(s->table.p, 0, 4 * (size_t)CK_WORDS * (size_t)nd, v.stream)) != hipSuccess) { mhap_align_paths_free(paths); return fail("memset"); }
  if (!vitems.empty()) {
    if (vitems.size() > (size_t)INT32_MAX) { mhap_align_paths_free(paths); *v.err = std::string(who) + ": more than 2^31 - 1 aligned reads"; return MHAP_E_INVALID; }
    up(s->ops, paths->ops.data(), 4 * paths->ops.size());
    up(s->vitems, vitems.data(), sizeof(VoteItem) * vitems.size());
    if (e == hipSuccess) {
      const dim3 grid((unsigned)vitems.size()), wave(64);
      if (s->weighted)
        hipLaunchKernelGGL((vote_kernel<true, QualityWeight>), grid, wave, 0, v.stream, s->bases.as<uint8_t>(), s->vitems.as<VoteItem>(),
                           s->ops.as<uint32_t>(), s->table.as<uint32_t>(), QualityWeight{s->in_quals.as<uint8_t>(), s->W});
      else
        hipLaunchKernelGGL((vote_kernel<true, UnitWeight>), grid, wave, 0, v.stream, s->bases.as<uint8_t>(), s->vitems.as<VoteItem>(),
                           s->ops.as<uint32_t>(), s->table.as<uint32_t>(), UnitWeight());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(v.stream);   // (the runs and the items are the host's until here)
  }
  if (paths) mhap_align_paths_free(paths);
  if (e != hipSuccess) return fail("the vote");
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("the vote");
  lap(2);
  // the call: lengths per tile, their prefix sums, the bytes
  std::vector<int32_t> tile_len((size_t)n_tiles), tile_counts((size_t)n_tiles * 4);
  std::vector<int64_t> tile_off((size_t)n_tiles), out_offsets((size_t)nu + 1, 0), stats((size_t)nu * 6, 0);
  const uint8_t* draft = s->bases.as<uint8_t>() + s->n_bases;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(s->weighted ? ccall_kernel<NeutralWeight> : ccall_kernel<UnitWeight>, dim3((unsigned)n_tiles), dim3(CK_T), 0, v.stream, draft, nu, s->d_ulen.as<int64_t>(), s->d_ubase.as<int64_t>(),
                       s->d_utile.as<int64_t>(), s->table.as<uint32_t>(), (int)s->min_cov, s->tile_len.as<int32_t>(), s->tile_counts.as<int32_t>(),
                       (const int64_t*)nullptr, (const int64_t*)nullptr, (uint8_t*)nullptr, (int64_t*)nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
    if ((e = hipMemcpyAsync(tile_len.data(), s->tile_len.p, 4 * (size_t)n_tiles, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(tile_counts.data(), s->tile_counts.p, 16 * (size_t)n_tiles, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return fail("download");
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("the call");
  }
  int64_t at = 0;
  for (int64_t k = 0; k < nu; k++) {
    int64_t* st = stats.data() + 6 * k;
    out_offsets[(size_t)k] = at;
    st[0] = u_len[(size_t)k];
    for (int64_t j = utile[(size_t)k]; j < utile[(size_t)k + 1]; j++) {
      tile_off[(size_t)j] = at;
      at += tile_len[(size_t)j];
      for (int u = 0; u < 4; u++) st[2 + u] += tile_counts[(size_t)(4 * j + u)];
    }
    st[1] = at - out_offsets[(size_t)k];
    counts[CC_BASES_IN] += st[0]; counts[CC_BASES_OUT] += st[1];
    counts[CC_SUB] += st[2]; counts[CC_DEL] += st[3]; counts[CC_INS] += st[4]; counts[CC_LOW] += st[5];
  }
  out_offsets[(size_t)nu] = at;
  if ((e = s->out.ensure((size_t)std::max<int64_t>(at, 1))) != hipSuccess) return fail("hipMalloc of the consensus bytes");
  if (n_tiles > 0) {
    up(s->tile_off, tile_off.data(), 8 * (size_t)n_tiles);
    up(s->d_outoff, out_offsets.data(), 8 * (size_t)(nu + 1));
    if (e != hipSuccess) return fail("upload");
    hipLaunchKernelGGL(s->weighted ? ccall_kernel<NeutralWeight> : ccall_kernel<UnitWeight>, dim3((unsigned)n_tiles), dim3(CK_T), 0, v.stream, draft, nu, s->d_ulen.as<int64_t>(), s->d_ubase.as<int64_t>(),
                       s->d_utile.as<int64_t>(), s->table.as<uint32_t>(), (int)s->min_cov, s->tile_len.as<int32_t>(), s->tile_counts.as<int32_t>(),
                       s->tile_off.as<int64_t>(), s->d_outoff.as<int64_t>(), s->out.as<uint8_t>(), s->posmap.as<int64_t>());
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch");
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return fail("the call");
  }
  s->u_len = std::move(u_len); s->ubase = std::move(ubase); s->out_offsets = std::move(out_offsets); s->stats = std::move(stats);
  s->place = std::move(place);
  s->n_draft = nd; s->out_bytes = at; s->n_unitigs = nu;
  lap(3);
  return MHAP_OK;
}

extern "C" int mhap_consensus_info(mhap_consensus_session* s, int64_t* n_unitigs, int64_t* n_reads, int64_t* n_draft, int64_t* n_out) {
  if (!s) return MHAP_E_INVALID;
  const bool ok = s->n_unitigs >= 0 && graph_view(s->g).unitig_gen == s->gen;
  if (n_unitigs) *n_unitigs = ok ? s->n_unitigs : -1;
  if (n_reads) *n_reads = s->n_reads;
  if (n_draft) *n_draft = ok ? s->n_draft : 0;
  if (n_out) *n_out = ok ? s->out_bytes : 0;
  return MHAP_OK;
}

extern "C" int mhap_consensus_copy(mhap_consensus_session* s, uint8_t* bytes, int64_t* out_offsets, int64_t* stats) {
  const char* who = "mhap_consensus_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!out_offsets || (s->n_unitigs > 0 && !stats) || (s->out_bytes > 0 && !bytes)) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  std::copy(s->out_offsets.begin(), s->out_offsets.end(), out_offsets);
  std::copy(s->stats.begin(), s->stats.end(), stats);
  if (s->out_bytes == 0) return MHAP_OK;
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = hipMemcpyAsync(bytes, s->out.p, (size_t)s->out_bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  return MHAP_OK;
}

extern "C" int mhap_consensus_copy_placements(mhap_consensus_session* s, int64_t* rows) {
  const char* who = "mhap_consensus_copy_placements";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (s->n_reads > 0 && !rows) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  std::copy(s->place.begin(), s->place.end(), rows);
  return MHAP_OK;
}

extern "C" int mhap_consensus_copy_map(mhap_consensus_session* s, int64_t* map) {
  const char* who = "mhap_consensus_copy_map";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (s->n_draft == 0) return MHAP_OK;
  if (!map) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = hipMemcpyAsync(map, s->posmap.p, 8 * (size_t)s->n_draft, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  return MHAP_OK;
}

extern "C" int mhap_consensus_quality(mhap_consensus_session* s, const mhap_quality_params* params, uint8_t* quals, int64_t* hist) {
  const char* who = "mhap_consensus_quality";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  mhap_quality_params p;
  mhap_quality_default_params(&p);
  if (params) p = *params;
  if (!quality_params_ok(p.per_vote, p.cap, who, *v.err)) return MHAP_E_INVALID;
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (hist) for (int b = 0; b < QUAL_BINS; b++) hist[b] = 0;
  if (s->out_bytes == 0) return MHAP_OK;
  if (!quals) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  int64_t n_tiles = 0;
  for (int64_t k = 0; k < s->n_unitigs; k++) n_tiles += (s->u_len[(size_t)k] + CT - 1) / CT;
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = s->quals.ensure((size_t)s->out_bytes)) != hipSuccess || (e = s->hist.ensure(8 * QUAL_BINS)) != hipSuccess) return hip_fail(v, who, "hipMalloc of the quality bytes", e);
  if ((e = hipMemsetAsync(s->hist.p, 0, 8 * QUAL_BINS, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  hipLaunchKernelGGL(s->weighted ? cqual_kernel<NeutralWeight> : cqual_kernel<UnitWeight>, dim3((unsigned)n_tiles), dim3(CK_T), 0, v.stream, s->bases.as<uint8_t>() + s->n_bases, s->n_unitigs,
                     s->d_ulen.as<int64_t>(), s->d_ubase.as<int64_t>(), s->d_utile.as<int64_t>(), s->table.as<uint32_t>(), (int)s->min_cov,
                     (int)p.per_vote, (int)p.cap, s->d_outoff.as<int64_t>(), s->posmap.as<int64_t>(), s->quals.as<uint8_t>(),
                     s->hist.as<unsigned long long>());
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  if ((e = hipMemcpyAsync(quals, s->quals.p, (size_t)s->out_bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if (hist && (e = hipMemcpyAsync(hist, s->hist.p, 8 * QUAL_BINS, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  return MHAP_OK;
}

extern "C" int mhap_consensus_times(mhap_consensus_session* s, double* seconds) {
  const char* who = "mhap_consensus_times";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!seconds) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  for (int k = 0; k < 4; k++) seconds[k] = s->seconds[k];
  return MHAP_OK;
}

extern "C" int mhap_consensus_votes(mhap_consensus_session* s, int64_t unitig, uint16_t* counters) {
  const char* who = "mhap_consensus_votes";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = need_run(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (unitig < 0 || unitig >= s->n_unitigs) { *v.err = std::string(who) + ": unitig " + std::to_string(unitig) + " is not among the " + std::to_string(s->n_unitigs) + " unitigs"; return MHAP_E_INVALID; }
  const int64_t len = s->u_len[(size_t)unitig];
  if (len == 0) return MHAP_OK;
  if (!counters) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return copy_votes(v, who, s->table.as<uint32_t>(), (int64_t)CK_WORDS * s->ubase[(size_t)unitig], len, CK_WORDS, counters);
}

extern "C" void mhap_consensus_free(mhap_consensus_session* s) {
  if (!s) return;
  (void)hipSetDevice(handle_view(s->h).device);
  s->release();
  delete s;
}
