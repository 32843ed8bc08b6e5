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
// vote_kernel<true, Weigh> (vote_common.hpp): one wave per accepted (record, view) over vote_walk, which the unitig consensus and the
// variant sites share.  The runs go through 64 at a time: lane l takes run l of the chunk, the lanes
// scan the run lengths (rows consumed, columns consumed, columns of the path) to get every run's first (i, j) and first path column,
// and leave them in LDS; then the chunk's path columns are dealt to the lanes 64 at a time, each lane finding its run by a binary
// search over the 64 starts.  An Ins group's t and k come from its run's start (and its length, in the reversed view), never from a
// neighbouring lane.  The reversed view of a to_rc record is not walked backwards: votes are sums, so only what depends on the
// order is turned round — t -> blen - 1 - t, the complement, the end of the view at which no span is counted, the side of an Ins
// group its target position lies on and the direction k counts in.
//
// call_kernel<Weigh>: one workgroup per read, 256 positions at a time: every thread decides its position (0 to 5 bytes), the workgroup
// scans the emitted lengths (vote_common.hpp's scan_emitted), and in the second of two launches writes the bytes.  The first launch
// leaves the six counts per read; the reads' output offsets are the prefix sums of their len_out, made on the host, which returns them
// anyway.
//
// qcall_kernel<Weigh> (mhap_correct_quality): the call's scan once more over the table and the offsets of a completed finish, with the base
// qualities of vote_common.hpp's decide_quality behind every decision and a histogram of them ("base qualities" in include/mhap_hip.h).
//
// Weigh is UnitWeight, or QualityWeight in a session begun with qualities ("quality-weighted votes"): the same three kernels, the own
// byte's weight read next to the own byte.  The host side of the table (the reads, the checks, the items of an add under the cap, the
// chunked launch, the counters of a read) is vote_table.hpp's VoteTable, which the session sits on.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"
#include "vote_common.hpp"
#include "vote_table.hpp"
#include "weighted_vote.hpp"

namespace mhap {
namespace {

// reads: per read {offset in bases, first table position}; lengths; out_offsets == nullptr: count only (stats), else write the bytes.
// own_weight(at): the weight of the own byte stored at `at` of the bases — UnitWeight, or in a weighted session the QualityWeight
// over the qualities parallel to the bases ("quality-weighted votes" in include/mhap_hip.h).
template <class Weigh>
__global__ __launch_bounds__(CK_T) void call_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off,
                                                    const int64_t* __restrict__ read_pos, const int32_t* __restrict__ lengths,
                                                    const uint32_t* __restrict__ table, int min_cov, const int64_t* __restrict__ out_offsets,
                                                    uint8_t* __restrict__ out, int32_t* __restrict__ stats, Weigh own_weight) {
  __shared__ int acc[5];   // len_out, n_sub, n_del, n_ins, n_low
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const int64_t first = read_off[r];
  const uint8_t* own = bases + first;
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int tid = threadIdx.x;
  if (tid < 5) acc[tid] = 0;
  int64_t written = 0;   // bytes emitted by the tiles before this one
  int my[5] = {0, 0, 0, 0, 0};
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    if (t < len) D = decide<Weigh::neutral>(w, len, t, own[t], own_weight(first + t), min_cov);
    my[0] += D.n; my[1] += D.sub; my[2] += D.del; my[3] += D.ins; my[4] += D.low;
    const EmitScan sc = scan_emitted(D.n);
    if (out_offsets) {
      uint8_t* o = out + out_offsets[r] + written + sc.before + (sc.incl - D.n);
      for (int u = 0; u < D.n; u++) o[u] = D.bytes[u];
    }
    written += sc.tile;
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
// decide_quality() behind every decide().  A kernel of its own, so that call_kernel carries no quality.  One writer per quality byte;
// the workgroup's histogram lives in LDS and leaves by one 64-bit atomic per non-empty bin.
template <class Weigh>
__global__ __launch_bounds__(CK_T) void qcall_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off,
                                                     const int64_t* __restrict__ read_pos, const int32_t* __restrict__ lengths,
                                                     const uint32_t* __restrict__ table, int min_cov, int per_vote, int cap,
                                                     const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ quals,
                                                     unsigned long long* __restrict__ hist, Weigh own_weight) {
  __shared__ unsigned long long bins[QUAL_BINS];
  constexpr int U = Weigh::neutral;
  const int64_t r = blockIdx.x;
  const int64_t len = lengths[r];
  const int64_t first = read_off[r];
  const uint8_t* own = bases + first;
  const uint32_t* w = table + (int64_t)CK_WORDS * read_pos[r];
  const int64_t o_begin = out_offsets[r], o_end = out_offsets[r + 1];
  const int tid = threadIdx.x;
  if (tid < QUAL_BINS) bins[tid] = 0ull;
  int64_t written = 0;
  for (int64_t t0 = 0; t0 < len; t0 += CK_T) {
    const int64_t t = t0 + tid;
    Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
    uint8_t q[1 + CK_KI] = {0, 0, 0, 0, 0};
    if (t < len) {
      const int own_w = own_weight(first + t);
      D = decide<U>(w, len, t, own[t], own_w, min_cov);
      decide_quality<U>(w, len, t, own[t], own_w, D, per_vote, cap, q);
    }
    const EmitScan sc = scan_emitted(D.n);   // (behind its first barrier the bins are zero)
    const int64_t at = o_begin + written + sc.before + (sc.incl - D.n);
    for (int u = 0; u < D.n; u++)
      if (at + u < o_end) {   // (the offsets are those of this table and this min_cov: always)
        quals[at + u] = q[u];
        atomicAdd(&bins[q[u]], 1ull);
      }
    written += sc.tile;
  }
  __syncthreads();
  if (tid < QUAL_BINS && bins[tid]) atomicAdd(hist + tid, bins[tid]);
}

}  // namespace
}  // namespace mhap

using namespace mhap;

// the vote table and the reads are VoteTable's; the session's own: the qualities and their weights, the call and the quality pass
struct mhap_correct_session : VoteTable {
  int64_t out_bytes = -1;                               // < 0: no finish yet
  int32_t min_cov = 0;                                  // of the last completed finish
  bool voted_since = false;                             // votes were cast after that finish: its offsets are not the table's any more
  bool weighted = false;                                // begun with qualities: the QualityWeight kernels, WK_CAP views per target
  Weights W{0, 0};
  DevBuf in_quals, out_off, out, stats, quals, hist;
  QualityWeight weigh() const { return QualityWeight{in_quals.as<uint8_t>(), W}; }
  void release() {
    release_table();
    for (DevBuf* b : {&in_quals, &out_off, &out, &stats, &quals, &hist}) b->release();
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
  if (!VoteTable::args_ok(v, who, session, bases, n_bases, read_ids, offsets, lengths, n_reads)) return MHAP_E_INVALID;
  if (!VoteTable::reads_inside(v, who, n_bases, offsets, lengths, n_reads)) return MHAP_E_INVALID;
  mhap_weight_params wp;
  mhap_weight_default_params(&wp);
  if (qualities && weights) wp = *weights;
  if (qualities && !weight_params_ok(wp.q_lo, wp.q_hi, who, *v.err)) return MHAP_E_INVALID;
  mhap_correct_session* s = new mhap_correct_session();
  s->weighted = qualities != nullptr; s->W = Weights{wp.q_lo, wp.q_hi};
  (void)hipSetDevice(v.device);
  hipError_t e = s->begin_table(v, h, CK_WORDS, bases, n_bases, read_ids, offsets, lengths, n_reads);
  const size_t rb = (size_t)std::max<int64_t>(n_reads, 1);
  if (s->weighted) VoteTable::upload(v, e, s->in_quals, qualities, (size_t)n_bases);
  if (e == hipSuccess) e = s->stats.ensure(24 * rb);
  if (e == hipSuccess) e = s->out_off.ensure(8 * (rb + 1));
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
  int rc = check_call(v, who, recs, n, paths, true);
  if (rc != MHAP_OK) return rc;
  std::vector<VoteItem> items;
  if ((rc = s->build_items(v, who, recs, n, paths, views, s->weighted ? WK_CAP : CK_CAP, items)) != MHAP_OK) return rc;
  if (items.empty()) return MHAP_OK;
  s->voted_since = true;
  return s->cast_votes(v, who, paths, items, [&](unsigned c) {
    const dim3 grid(c), wave(64);
    if (s->weighted)
      hipLaunchKernelGGL((vote_kernel<true, QualityWeight>), grid, wave, 0, v.stream, s->bases.as<uint8_t>(), s->items.as<VoteItem>(),
                         s->ops.as<uint32_t>(), s->table.as<uint32_t>(), s->weigh());
    else
      hipLaunchKernelGGL((vote_kernel<true, UnitWeight>), grid, wave, 0, v.stream, s->bases.as<uint8_t>(), s->items.as<VoteItem>(),
                         s->ops.as<uint32_t>(), s->table.as<uint32_t>(), UnitWeight());
  });
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
      hipLaunchKernelGGL(call_kernel<QualityWeight>, grid, block, 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(), s->read_pos.as<int64_t>(),
                         s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)min_cov, out_off, out, s->stats.as<int32_t>(), s->weigh());
    else
      hipLaunchKernelGGL(call_kernel<UnitWeight>, grid, block, 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(), s->read_pos.as<int64_t>(),
                         s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)min_cov, out_off, out, s->stats.as<int32_t>(), UnitWeight());
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
    hipLaunchKernelGGL(qcall_kernel<QualityWeight>, dim3((unsigned)s->n_reads), dim3(CK_T), 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(),
                       s->read_pos.as<int64_t>(), s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)s->min_cov, (int)p.per_vote, (int)p.cap,
                       s->out_off.as<int64_t>(), s->quals.as<uint8_t>(), s->hist.as<unsigned long long>(), s->weigh());
  else
    hipLaunchKernelGGL(qcall_kernel<UnitWeight>, dim3((unsigned)s->n_reads), dim3(CK_T), 0, v.stream, s->bases.as<uint8_t>(), s->read_off.as<int64_t>(),
                       s->read_pos.as<int64_t>(), s->read_len.as<int32_t>(), s->table.as<uint32_t>(), (int)s->min_cov, (int)p.per_vote, (int)p.cap,
                       s->out_off.as<int64_t>(), s->quals.as<uint8_t>(), s->hist.as<unsigned long long>(), UnitWeight());
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  if ((e = hipMemcpyAsync(quals, s->quals.p, (size_t)s->out_bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if (hist && (e = hipMemcpyAsync(hist, s->hist.p, 8 * QUAL_BINS, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  return MHAP_OK;
}

extern "C" int mhap_correct_votes(mhap_correct_session* s, int64_t read_index, uint16_t* counters) {
  if (!s) return MHAP_E_INVALID;
  return s->read_votes("mhap_correct_votes", read_index, counters);
}

extern "C" void mhap_correct_free(mhap_correct_session* s) {
  if (!s) return;
  s->release();
  delete s;
}
