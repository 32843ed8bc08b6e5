// correct_kernels.hip — read correction: a pile-up vote over every read from the realigned overlaps' paths and a majority call per
// position (mhap_correct_begin / _add / _add_views / _finish / _copy / _quality / _votes / _free).  The contract — the two views of a record, the 22 counters,
// the 65 535-view cap and the call — is the prose of include/mhap_hip.h ("read correction"); tests/consensus_ref.py restates it.
//
// The vote table.  24 counters of 16 bits per base, two to a word: 12 words per base, kept as 12 planes per read — word p of position t
// of a read of length L that starts at table position v is table[12 v + p L + t] — so that the lanes of a wave, which take consecutive
// columns of a path and with them consecutive target positions, add to consecutive words of a plane.  Counter c (the order of
// mhap_correct_votes) is the low (c even) or high (c odd) half of word c / 2:
//   word 0 base A | C    word 1 base G | T    word 2 del | span    words 3 + 2 k, 4 + 2 k ins[k] A | C, G | T    word 11 spare
// A vote is atomicAdd(word, 1) or atomicAdd(word, 1 << 16); the host's cap on accepted views per target keeps every half below 2^16,
// so no add carries into its neighbour.  Position-major words (one 48-byte row per base) would put a wave's adds 48 bytes apart.
// Integer atomic rates on this chip are not measured; the layout follows from the shape the float-atomic measurements prefer.
//
// vote_kernel: one wave per accepted (record, view); the walk itself is vote_common.hpp's vote_walk, which the unitig consensus
// shares.  The runs go through 64 at a time: lane l takes run l of the chunk, the lanes
// scan the run lengths (rows consumed, columns consumed, columns of the path) to get every run's first (i, j) and first path column,
// and leave them in LDS; then the chunk's path columns are dealt to the lanes 64 at a time, each lane finding its run by a binary
// search over the 64 starts.  An Ins group's t and k come from its run's start (and its length, in the reversed view), never from a
// neighbouring lane.  The reversed view of a to_rc record is not walked backwards: votes are sums, so only what depends on the
// order is turned round — t -> blen - 1 - t, the complement, the end of the view at which no span is counted, the side of an Ins
// group its target position lies on and the direction k counts in.
//
// call_kernel: one workgroup per read, 256 positions at a time: every thread decides its position (0 to 5 bytes), the workgroup scans
// the emitted lengths, and in the second of two launches writes the bytes.  The first launch leaves the six counts per read; the reads'
// output offsets are the prefix sums of their len_out, made on the host, which returns them anyway.
//
// qcall_kernel (mhap_correct_quality): the call's scan once more over the table and the offsets of a completed finish, with the base
// qualities of vote_common.hpp's decide_quality behind every decision and a histogram of them ("base qualities" in include/mhap_hip.h).
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"
#include "read_table.hpp"
#include "vote_common.hpp"
#include "weighted_vote.hpp"

namespace mhap {
namespace {

__global__ __launch_bounds__(64) void vote_kernel(const uint8_t* __restrict__ bases, const VoteItem* __restrict__ items,
                                                  const uint32_t* __restrict__ ops, uint32_t* __restrict__ table) {
  const VoteItem it = items[blockIdx.x];
  vote_walk(bases, it, ops, table);
}

// reads: per read {offset in bases, first table position}; lengths; out_offsets == nullptr: count only (stats), else write the bytes
__global__ __launch_bounds__(CK_T) void call_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off,
                                                    const int64_t* __restrict__ read_pos, const int32_t* __restrict__ lengths,
                                                    const uint32_t* __restrict__ table, int min_cov, const int64_t* __restrict__ out_offsets,
                                                    uint8_t* __restrict__ out, int32_t* __restrict__ stats) {
  __shared__ int wave_sum[CK_T / 64];
  __shared__ int acc[5];   // len_out, n_sub, n_del, n_ins, n_low
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const uint8_t* own = bases + read_off[r];
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 5) acc[tid] = 0;
  int64_t written = 0;   // bytes emitted by the tiles before this one
  int my[5] = {0, 0, 0, 0, 0};
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    if (t < len) D = decide(w, len, t, own[t], min_cov);
    my[0] += D.n; my[1] += D.sub; my[2] += D.del; my[3] += D.ins; my[4] += D.low;
    int incl = D.n;   // inclusive scan of the emitted lengths over the workgroup
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    __syncthreads();   // wave_sum of the previous tile has been read
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, tile = 0;
    for (int u = 0; u < CK_T / 64; u++) { if (u < wave) before += wave_sum[u]; tile += wave_sum[u]; }
    if (out_offsets) {
      uint8_t* o = out + out_offsets[r] + written + before + (incl - D.n);
      for (int u = 0; u < D.n; u++) o[u] = D.bytes[u];
    }
    written += tile;
  }
  __syncthreads();
  for (int u = 0; u < 5; u++) if (my[u]) atomicAdd(&acc[u], my[u]);
  __syncthreads();
  if (tid == 0 && !out_offsets) {
    int32_t* s = stats + 6 * r;
    s[0] = (int32_t)len; s[1] = acc[0]; s[2] = acc[1]; s[3] = acc[2]; s[4] = acc[3]; s[5] = acc[4];
  }
}

// The quality pass of mhap_correct_quality: call_kernel's scan again, over the table and the offsets of a completed finish, with
// decide_quality() behind every decide().  A kernel of its own, so that call_kernel stays the code it is.  One writer per quality byte;
// the workgroup's histogram lives in LDS and leaves by one 64-bit atomic per non-empty bin.
__global__ __launch_bounds__(CK_T) void qcall_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off,
                                                     const int64_t* __restrict__ read_pos, const int32_t* __restrict__ lengths,
                                                     const uint32_t* __restrict__ table, int min_cov, int per_vote, int cap,
                                                     const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ quals,
                                                     unsigned long long* __restrict__ hist) {
  __shared__ int wave_sum[CK_T / 64];
  __shared__ unsigned long long bins[QUAL_BINS];
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const uint8_t* own = bases + read_off[r];
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int64_t o_begin = out_offsets[r], o_end = out_offsets[r + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < QUAL_BINS) bins[tid] = 0ull;
  int64_t written = 0;
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    uint8_t q[1 + CK_KI] = {0, 0, 0, 0, 0};
    if (t < len) {
      D = decide(w, len, t, own[t], min_cov);
      decide_quality(w, len, t, own[t], D, per_vote, cap, q);
    }
    int incl = D.n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    __syncthreads();   // wave_sum of the previous tile has been read (and, the first time, the bins are zero)
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, tile = 0;
    for (int u = 0; u < CK_T / 64; u++) { if (u < wave) before += wave_sum[u]; tile += wave_sum[u]; }
    const int64_t at = o_begin + written + before + (incl - D.n);
    for (int u = 0; u < D.n; u++)
      if (at + u < o_end) {   // (the offsets are those of this table and this min_cov: always)
        quals[at + u] = q[u];
        atomicAdd(&bins[q[u]], 1ull);
      }
    written += tile;
  }
  __syncthreads();
  if (tid < QUAL_BINS && bins[tid]) atomicAdd(hist + tid, bins[tid]);
}

// The three kernels of a weighted session ("quality-weighted votes" in include/mhap_hip.h): the schedules of vote_kernel, call_kernel
// and qcall_kernel over weighted_vote.hpp's walk, decision and qualities.  quals: one Phred byte per base, parallel to bases; the own
// byte's weight is read next to the own byte.
__global__ __launch_bounds__(64) void wvote_kernel(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, Weights W,
                                                   const VoteItem* __restrict__ items, const uint32_t* __restrict__ ops,
                                                   uint32_t* __restrict__ table) {
  const VoteItem it = items[blockIdx.x];
  vote_walk_weighted(bases, quals, W, it, ops, table);
}

__global__ __launch_bounds__(CK_T) void wcall_kernel(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, Weights W,
                                                     const int64_t* __restrict__ read_off, const int64_t* __restrict__ read_pos,
                                                     const int32_t* __restrict__ lengths, const uint32_t* __restrict__ table, int min_cov,
                                                     const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ out,
                                                     int32_t* __restrict__ stats) {
  __shared__ int wave_sum[CK_T / 64];
  __shared__ int acc[5];   // len_out, n_sub, n_del, n_ins, n_low
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const uint8_t* own = bases + read_off[r];
  const uint8_t* own_q = quals + read_off[r];
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 5) acc[tid] = 0;
  int64_t written = 0;
  int my[5] = {0, 0, 0, 0, 0};
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    if (t < len) D = decide_weighted(w, len, t, own[t], weight_of(own_q[t], W), min_cov);
    my[0] += D.n; my[1] += D.sub; my[2] += D.del; my[3] += D.ins; my[4] += D.low;
    int incl = D.n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    __syncthreads();   // wave_sum of the previous tile has been read
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, tile = 0;
    for (int u = 0; u < CK_T / 64; u++) { if (u < wave) before += wave_sum[u]; tile += wave_sum[u]; }
    if (out_offsets) {
      uint8_t* o = out + out_offsets[r] + written + before + (incl - D.n);
      for (int u = 0; u < D.n; u++) o[u] = D.bytes[u];
    }
    written += tile;
  }
  __syncthreads();
  for (int u = 0; u < 5; u++) if (my[u]) atomicAdd(&acc[u], my[u]);
  __syncthreads();
  if (tid == 0 && !out_offsets) {
    int32_t* s = stats + 6 * r;
    s[0] = (int32_t)len; s[1] = acc[0]; s[2] = acc[1]; s[3] = acc[2]; s[4] = acc[3]; s[5] = acc[4];
  }
}

__global__ __launch_bounds__(CK_T) void wqcall_kernel(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ in_quals, Weights W,
                                                      const int64_t* __restrict__ read_off, const int64_t* __restrict__ read_pos,
                                                      const int32_t* __restrict__ lengths, const uint32_t* __restrict__ table, int min_cov,
                                                      int per_vote, int cap, const int64_t* __restrict__ out_offsets,
                                                      uint8_t* __restrict__ quals, unsigned long long* __restrict__ hist) {
  __shared__ int wave_sum[CK_T / 64];
  __shared__ unsigned long long bins[QUAL_BINS];
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const uint8_t* own = bases + read_off[r];
  const uint8_t* own_q = in_quals + read_off[r];
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int64_t o_begin = out_offsets[r], o_end = out_offsets[r + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < QUAL_BINS) bins[tid] = 0ull;
  int64_t written = 0;
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    uint8_t q[1 + CK_KI] = {0, 0, 0, 0, 0};
    if (t < len) {
      const int own_w = weight_of(own_q[t], W);
      D = decide_weighted(w, len, t, own[t], own_w, min_cov);
      decide_quality_weighted(w, len, t, own[t], own_w, D, per_vote, cap, q);
    }
    int incl = D.n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    __syncthreads();   // wave_sum of the previous tile has been read (and, the first time, the bins are zero)
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, tile = 0;
    for (int u = 0; u < CK_T / 64; u++) { if (u < wave) before += wave_sum[u]; tile += wave_sum[u]; }
    const int64_t at = o_begin + written + before + (incl - D.n);
    for (int u = 0; u < D.n; u++)
      if (at + u < o_end) {   // (the offsets are those of this table and this min_cov: always)
        quals[at + u] = q[u];
        atomicAdd(&bins[q[u]], 1ull);
      }
    written += tile;
  }
  __syncthreads();
  if (tid < QUAL_BINS && bins[tid]) atomicAdd(hist + tid, bins[tid]);
}

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_correct_session {
  mhap_handle* h = nullptr;
  int64_t n_reads = 0, n_bases = 0, n_pos = 0;          // n_pos: bases of the reads = positions of the table
  std::vector<int64_t> offsets, pos;                    // read r: its bytes in the bases, its first table position
  std::vector<int32_t> lengths;
  std::unordered_map<int64_t, int64_t> by_id;
  std::vector<uint32_t> views;                          // accepted views per target
  int64_t skipped = 0, out_bytes = -1;                  // out_bytes < 0: no finish yet
  int32_t min_cov = 0;                                  // of the last completed finish
  bool voted_since = false;                             // votes were cast after that finish: its offsets are not the table's any more
  bool weighted = false;                                // begun with qualities: the w* kernels, WK_CAP views per target
  Weights W{0, 0};
  DevBuf bases, in_quals, table, read_off, read_pos, read_len, items, ops, out_off, out, stats, quals, hist;
  void release() {
    in_quals.release();
    bases.release(); table.release(); read_off.release(); read_pos.release(); read_len.release(); items.release(); ops.release();
    out_off.release(); out.release(); stats.release(); quals.release(); hist.release();
  }
};

extern "C" void mhap_weight_default_params(mhap_weight_params* p) {
  if (!p) return;
  p->q_lo = 7; p->q_hi = 20;   // the fewest wrong bytes on the restatement (EXPERIMENTS.md, "Quality-weighted votes")
}

// the begin behind mhap_correct_begin (qualities == nullptr) and mhap_correct_begin_weighted
static int correct_begin(const char* who, mhap_handle* h, const uint8_t* bases, const uint8_t* qualities, int64_t n_bases,
                         const int64_t* read_ids, const int64_t* offsets, const int32_t* lengths, int64_t n_reads,
                         const mhap_weight_params* weights, mhap_correct_session** session) {
  if (session) *session = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!session || n_bases < 0 || n_reads < 0 || (n_bases > 0 && !bases) || (n_reads > 0 && (!read_ids || !offsets || !lengths))) {
    *v.err = std::string(who) + ": null or negative argument";
    return MHAP_E_INVALID;
  }
  for (int64_t i = 0; i < n_reads; i++)
    if (offsets[i] < 0 || lengths[i] < 0 || offsets[i] > n_bases - lengths[i]) {
      *v.err = std::string(who) + ": read " + std::to_string(i) + " lies outside the " + std::to_string(n_bases) + " bases";
      return MHAP_E_INVALID;
    }
  mhap_weight_params wp;
  mhap_weight_default_params(&wp);
  if (qualities && weights) wp = *weights;
  if (qualities && !weight_params_ok(wp.q_lo, wp.q_hi, who, *v.err)) return MHAP_E_INVALID;
  mhap_correct_session* s = new mhap_correct_session();
  s->h = h; s->n_reads = n_reads; s->n_bases = n_bases;
  s->weighted = qualities != nullptr; s->W = Weights{wp.q_lo, wp.q_hi};
  s->offsets.assign(offsets, offsets + n_reads);
  s->lengths.assign(lengths, lengths + n_reads);
  s->pos.resize((size_t)n_reads);
  s->views.assign((size_t)n_reads, 0u);
  s->by_id.reserve((size_t)n_reads * 2);
  for (int64_t i = 0; i < n_reads; i++) {
    s->by_id.emplace(read_ids[i], i);   // (the first read of an id wins, as in mhap_realign_plan)
    s->pos[(size_t)i] = s->n_pos;
    s->n_pos += lengths[i];
  }
  (void)hipSetDevice(v.device);
  hipError_t e = hipSuccess;
  const size_t table_bytes = (size_t)std::max<int64_t>(s->n_pos, 1) * CK_WORDS * 4, rb = (size_t)std::max<int64_t>(n_reads, 1);
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    if (e == hipSuccess) e = b.ensure(std::max<size_t>(bytes, 1));
    if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, v.stream);
  };
  up(s->bases, bases, (size_t)n_bases);
  if (s->weighted) up(s->in_quals, qualities, (size_t)n_bases);
  up(s->read_off, s->offsets.data(), 8 * (size_t)n_reads);
  up(s->read_pos, s->pos.data(), 8 * (size_t)n_reads);
  up(s->read_len, s->lengths.data(), 4 * (size_t)n_reads);
  if (e == hipSuccess) e = s->stats.ensure(24 * rb);
  if (e == hipSuccess) e = s->out_off.ensure(8 * (rb + 1));
  if (e == hipSuccess) e = s->table.ensure(table_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(s->table.p, 0, table_bytes, v.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
  if (e != hipSuccess) {
    s->release();
    delete s;
    return hip_fail(v, who, "the vote table (48 bytes per base) and the bases", e);
  }
  *session = s;
  return MHAP_OK;
}

extern "C" int mhap_correct_begin(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                                  const int32_t* lengths, int64_t n_reads, mhap_correct_session** session) {
  return correct_begin("mhap_correct_begin", h, bases, nullptr, n_bases, read_ids, offsets, lengths, n_reads, nullptr, session);
}

extern "C" int mhap_correct_begin_weighted(mhap_handle* h, const uint8_t* bases, const uint8_t* qualities, int64_t n_bases,
                                           const int64_t* read_ids, const int64_t* offsets, const int32_t* lengths, int64_t n_reads,
                                           const mhap_weight_params* weights, mhap_correct_session** session) {
  return correct_begin(qualities ? "mhap_correct_begin_weighted" : "mhap_correct_begin", h, bases, qualities, n_bases, read_ids, offsets, lengths,
                       n_reads, weights, session);
}

// the add behind mhap_correct_add (views == nullptr: both views of every record) and mhap_correct_add_views
static int correct_add(const char* who, mhap_correct_session* s, const mhap_record* recs, int64_t n, const mhap_align_paths* paths,
                       const uint8_t* views) {
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (n < 0 || !paths || (n > 0 && !recs)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if ((int64_t)paths->offsets.size() - 1 != n) {
    *v.err = std::string(who) + ": the paths are those of " + std::to_string((int64_t)paths->offsets.size() - 1) + " records, not of " + std::to_string(n);
    return MHAP_E_INVALID;
  }
  auto bad = [&](int64_t q, const std::string& what) {
    *v.err = std::string(who) + ": record " + std::to_string(q) + " " + what;
    return MHAP_E_INVALID;
  };
  std::vector<VoteItem> items;
  std::vector<std::pair<int64_t, int>> accepted;   // (target read, views) to take back when a later record is refused
  int64_t skipped = 0;
  auto undo = [&]() { for (auto& a : accepted) s->views[(size_t)a.first] -= (uint32_t)a.second; };
  for (int64_t q = 0; q < n; q++) {
    const mhap_record& r = recs[q];
    const int64_t o0 = paths->offsets[(size_t)q], o1 = paths->offsets[(size_t)q + 1];
    if (o1 == o0 || r.from_id == r.to_id) continue;
    int64_t idx[2];
    if (!find_record_reads(s->by_id, s->lengths.data(), who, q, r, idx, *v.err)) { undo(); return MHAP_E_INVALID; }
    const bool rc = r.to_rc != 0;
    int64_t i0, j0;
    std::string what;
    if (!path_spells_record(r, paths->ops, o0, o1, i0, j0, what)) { undo(); return bad(q, what); }
    for (int view = 0; view < 2; view++) {
      const int64_t target = idx[view];
      if (views && !(views[q] & (1u << view))) continue;   // not selected: no vote, no place under the cap, not a skipped view
      if (s->views[(size_t)target] >= (s->weighted ? WK_CAP : CK_CAP)) { skipped++; continue; }
      s->views[(size_t)target] += 1;
      accepted.emplace_back(target, 1);
      VoteItem it{};
      it.a_off = s->offsets[(size_t)idx[0]]; it.b_off = s->offsets[(size_t)idx[1]];
      it.v_words = (int64_t)CK_WORDS * s->pos[(size_t)target];
      it.ops_off = o0; it.alen = r.alen; it.blen = r.blen; it.i0 = (int32_t)i0; it.j0 = (int32_t)j0;
      it.n_ops = (int32_t)(o1 - o0); it.view = view; it.rc = rc ? 1 : 0;
      items.push_back(it);
    }
  }
  s->skipped += skipped;
  if (items.empty()) return MHAP_OK;
  s->voted_since = true;
  (void)hipSetDevice(v.device);
  hipError_t e;
  // a grid of at most 2^20 views at a time: the items of one launch are 64 MB
  constexpr size_t CHUNK = (size_t)1 << 20;
  if ((e = s->ops.ensure(4 * paths->ops.size())) != hipSuccess) return hip_fail(v, who, "hipMalloc of the runs", e);
  if ((e = s->items.ensure(sizeof(VoteItem) * std::min(items.size(), CHUNK))) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  if ((e = hipMemcpyAsync(s->ops.p, paths->ops.data(), 4 * paths->ops.size(), hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  for (size_t g0 = 0; g0 < items.size(); g0 += CHUNK) {
    const size_t c = std::min(CHUNK, items.size() - g0);
    if ((e = hipMemcpyAsync(s->items.p, items.data() + g0, sizeof(VoteItem) * c, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
    if (s->weighted)
      hipLaunchKernelGGL(wvote_kernel, dim3((unsigned)c), dim3(64), 0, v.stream, s->bases.as<uint8_t>(), s->in_quals.as<uint8_t>(), s->W,
                         s->items.as<VoteItem>(), s->ops.as<uint32_t>(), s->table.as<uint32_t>());
    else
      hipLaunchKernelGGL(vote_kernel, dim3((unsigned)c), dim3(64), 0, v.stream, s->bases.as<uint8_t>(), s->items.as<VoteItem>(),
                         s->ops.as<uint32_t>(), s->table.as<uint32_t>());
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);   // (items is reused by the next chunk)
  }
  return MHAP_OK;
}

extern "C" int mhap_correct_add(mhap_correct_session* s, const mhap_record* recs, int64_t n, const mhap_align_paths* paths) {
  return correct_add("mhap_correct_add", s, recs, n, paths, nullptr);
}

extern "C" int mhap_correct_add_views(mhap_correct_session* s, const mhap_record* recs, int64_t n, const mhap_align_paths* paths,
                                      const uint8_t* views) {
  return correct_add("mhap_correct_add_views", s, recs, n, paths, views);
}

extern "C" int mhap_correct_finish(mhap_correct_session* s, int32_t min_cov, int64_t* out_offsets, int32_t* stats, int64_t* skipped_views) {
  const char* who = "mhap_correct_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!out_offsets || (s->n_reads > 0 && !stats)) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  if (min_cov < 1) { *v.err = std::string(who) + ": min_cov must be at least 1 (" + std::to_string(min_cov) + ")"; return MHAP_E_INVALID; }
  if (skipped_views) *skipped_views = s->skipped;
  s->out_bytes = -1;
  out_offsets[0] = 0;
  if (s->n_reads == 0) { s->out_bytes = 0; s->min_cov = min_cov; s->voted_since = false; return MHAP_OK; }
  if (s->n_reads > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 reads"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  const dim3 grid((unsigned)s->n_reads), block(CK_T);
  // both launches of the call: the lengths and counts first (out_off == nullptr), then the bytes
  auto launch_call = [&](const int64_t* out_off, uint8_t* out) {
    if (s->weighted)
      hipLaunchKernelGGL(wcall_kernel, grid, block, 0, v.stream, s->bases.as<uint8_t>(), s->in_quals.as<uint8_t>(), s->W, s->read_off.as<int64_t>(),
                         s->read_pos.as<int64_t>(), s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)min_cov, out_off, out,
                         s->stats.as<int32_t>());
    else
      hipLaunchKernelGGL(call_kernel, grid, block, 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(), s->read_pos.as<int64_t>(),
                         s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)min_cov, out_off, out, s->stats.as<int32_t>());
  };
  launch_call(nullptr, nullptr);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  if ((e = hipMemcpyAsync(stats, s->stats.p, 24 * (size_t)s->n_reads, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  for (int64_t r = 0; r < s->n_reads; r++) out_offsets[r + 1] = out_offsets[r] + stats[6 * r + 1];
  const int64_t total = out_offsets[s->n_reads];
  if ((e = s->out.ensure((size_t)std::max<int64_t>(total, 1))) != hipSuccess) return hip_fail(v, who, "hipMalloc of the corrected bytes", e);
  if ((e = hipMemcpyAsync(s->out_off.p, out_offsets, 8 * (size_t)(s->n_reads + 1), hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
  launch_call(s->out_off.as<int64_t>(), s->out.as<uint8_t>());
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  s->out_bytes = total; s->min_cov = min_cov; s->voted_since = false;
  return MHAP_OK;
}

extern "C" int mhap_correct_copy(mhap_correct_session* s, uint8_t* bytes) {
  const char* who = "mhap_correct_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->out_bytes < 0) { *v.err = std::string(who) + ": no mhap_correct_finish has completed"; return MHAP_E_INVALID; }
  if (s->out_bytes == 0) return MHAP_OK;
  if (!bytes) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = hipMemcpyAsync(bytes, s->out.p, (size_t)s->out_bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  return MHAP_OK;
}

extern "C" void mhap_quality_default_params(mhap_quality_params* p) {
  if (!p) return;
  p->per_vote = 15; p->cap = 60;   // the slope is the measured one (EXPERIMENTS.md, "Base qualities"), the cap a convention
}

extern "C" int mhap_correct_quality(mhap_correct_session* s, const mhap_quality_params* params, uint8_t* quals, int64_t* hist) {
  const char* who = "mhap_correct_quality";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  mhap_quality_params p;
  mhap_quality_default_params(&p);
  if (params) p = *params;
  if (!quality_params_ok(p.per_vote, p.cap, who, *v.err)) return MHAP_E_INVALID;
  if (s->out_bytes < 0) { *v.err = std::string(who) + ": no mhap_correct_finish has completed"; return MHAP_E_INVALID; }
  if (s->voted_since) { *v.err = std::string(who) + ": records were added since the last mhap_correct_finish"; return MHAP_E_INVALID; }
  if (hist) for (int b = 0; b < QUAL_BINS; b++) hist[b] = 0;
  if (s->out_bytes == 0) return MHAP_OK;
  if (!quals) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = s->quals.ensure((size_t)s->out_bytes)) != hipSuccess || (e = s->hist.ensure(8 * QUAL_BINS)) != hipSuccess) return hip_fail(v, who, "hipMalloc of the quality bytes", e);
  if ((e = hipMemsetAsync(s->hist.p, 0, 8 * QUAL_BINS, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if (s->weighted)
    hipLaunchKernelGGL(wqcall_kernel, dim3((unsigned)s->n_reads), dim3(CK_T), 0, v.stream, s->bases.as<uint8_t>(), s->in_quals.as<uint8_t>(), s->W,
                       s->read_off.as<int64_t>(), s->read_pos.as<int64_t>(), s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)s->min_cov,
                       (int)p.per_vote, (int)p.cap, s->out_off.as<int64_t>(), s->quals.as<uint8_t>(), s->hist.as<unsigned long long>());
  else
    hipLaunchKernelGGL(qcall_kernel, dim3((unsigned)s->n_reads), dim3(CK_T), 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(),
                       s->read_pos.as<int64_t>(), s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)s->min_cov, (int)p.per_vote, (int)p.cap,
                       s->out_off.as<int64_t>(), s->quals.as<uint8_t>(), s->hist.as<unsigned long long>());
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  if ((e = hipMemcpyAsync(quals, s->quals.p, (size_t)s->out_bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if (hist && (e = hipMemcpyAsync(hist, s->hist.p, 8 * QUAL_BINS, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  return MHAP_OK;
}

extern "C" int mhap_correct_votes(mhap_correct_session* s, int64_t read_index, uint16_t* counters) {
  const char* who = "mhap_correct_votes";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (read_index < 0 || read_index >= s->n_reads) { *v.err = std::string(who) + ": read " + std::to_string(read_index) + " is not among the " + std::to_string(s->n_reads) + " reads"; return MHAP_E_INVALID; }
  const int64_t len = s->lengths[(size_t)read_index];
  if (len == 0) return MHAP_OK;
  if (!counters) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  std::vector<uint32_t> w((size_t)len * CK_WORDS);
  hipError_t e;
  if ((e = hipMemcpyAsync(w.data(), s->table.as<uint32_t>() + (int64_t)CK_WORDS * s->pos[(size_t)read_index], w.size() * 4, hipMemcpyDeviceToHost,
                          v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  for (int64_t t = 0; t < len; t++)
    for (int p = 0; p < CK_WORDS; p++) {
      const uint32_t x = w[(size_t)(p * len + t)];
      counters[24 * t + 2 * p] = (uint16_t)(x & 0xFFFFu);
      counters[24 * t + 2 * p + 1] = (uint16_t)(x >> 16);
    }
  return MHAP_OK;
}

extern "C" void mhap_correct_free(mhap_correct_session* s) {
  if (!s) return;
  s->release();
  delete s;
}
