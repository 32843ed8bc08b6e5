// variant_kernels.hip — variant sites marked from the pile-up votes and the overlaps that cross them set aside (mhap_variant_begin /
// _add / _votes / _finish / _copy / _apply / _free).  The contract — the votes, the site rule, the site list and a record's judgement —
// is the prose of include/mhap_hip.h ("variant sites"); tests/variant_ref.py restates it.
//
// The vote table.  The first three planes of the correction's (correct_kernels.hip): word p of position t of a read of length L that
// starts at table position v is table[3 v + p L + t], word 0 base A | C, word 1 base G | T, word 2 del | span, 16 bits each: 12 bytes
// per base.  The votes are cast by vote_common.hpp's vote_kernel<false, UnitWeight>, one wave per accepted view over vote_walk with
// the insertion slots compiled out; the adds are the correction's 32-bit atomics on 16-bit halves and the host's cap on accepted
// views keeps a half from carrying.  The host side of the table is vote_table.hpp's VoteTable, as the correction's.
//
// site_kernel: one workgroup of 256 per read, longest first, over tiles of MHAP_VARIANT_TILE positions in the order of
// pileup_common.hpp's tiles (load j, lane): three coalesced word loads and the own byte per position, one byte stored.
// site_kernel<false> stores the site bytes and leaves {n_sites, n_deep} per read; scan_kernel turns the n_sites into offsets;
// site_kernel<true> walks the reads that have sites again and writes every site at offsets[r] + (the sites in front of it), which
// pile_scan_tile gives: one writer per row and no atomic decides a place.
//
// judge_kernel: one wave per record over the same walk, votes compiled out: every lane classes its column from two bases and two site
// bytes, the lanes are combined by ballot and popcount and lane 0 writes the four tallies and the keep byte.  The run arrays of the
// walk are its only LDS.
#include <hip/hip_runtime.h>

#include <numeric>
#include <string>
#include <vector>

#include "device_common.hpp"
#include "mhap_internal.hpp"
#include "pileup_common.hpp"
#include "vote_common.hpp"
#include "vote_table.hpp"

namespace mhap {
namespace {

constexpr int VK_WORDS = 3;   // words per position: base A | C, G | T, del | span
static_assert(MHAP_VARIANT_TILE == PILE_T * PILE_LOADS, "a tile of the site kernel is a tile of pile_scan_tile");

// counts: reads, reads with a site, sites, deep positions, bases, accepted views, skipped views
enum { VC_READS = 0, VC_SOME, VC_SITES, VC_DEEP, VC_BASES, VC_ACCEPTED, VC_SKIPPED };
static_assert(VC_SKIPPED + 1 == MHAP_VARIANT_COUNTS, "the counts of the header");

struct VParams { int32_t min_depth, min_minor, min_pct, max_del_pct, min_diff, diff_pct; };

// the check of mhap_variant_begin: the three counts at least 1, the three percentages 0 .. 100
bool variant_params_ok(const mhap_variant_params& p, const char* who, std::string& err) {
  const auto pct = [](int32_t x) { return x >= 0 && x <= 100; };
  if (p.min_depth >= 1 && p.min_minor >= 1 && p.min_diff >= 1 && pct(p.min_pct) && pct(p.max_del_pct) && pct(p.diff_pct)) return true;
  err = std::string(who) + ": min_depth, min_minor and min_diff must be >= 1 and min_pct, max_del_pct and diff_pct 0 .. 100 (" +
        std::to_string(p.min_depth) + ", " + std::to_string(p.min_minor) + ", " + std::to_string(p.min_pct) + ", " + std::to_string(p.max_del_pct) + ", " +
        std::to_string(p.min_diff) + ", " + std::to_string(p.diff_pct) + ")";
  return false;
}

// what the rule says of one position
struct Site { int32_t site, deep, major, minor, c_major, c_minor, depth; };

__device__ inline Site decide_site(const uint32_t* __restrict__ w, int64_t len, int64_t t, uint32_t own, const VParams& P) {
  const uint32_t w0 = w[t], w1 = w[len + t], w2 = w[2 * len + t];
  const int ob = base_code(own);
  const int c[4] = {(int)(w0 & 0xFFFFu) + (ob == 0), (int)(w0 >> 16) + (ob == 1), (int)(w1 & 0xFFFFu) + (ob == 2), (int)(w1 >> 16) + (ob == 3)};
  const int del = (int)(w2 & 0xFFFFu);
  Site S;
  S.depth = c[0] + c[1] + c[2] + c[3] + del;
  S.major = 0; S.c_major = c[0];
#pragma unroll
  for (int b = 1; b < 4; b++) if (c[b] > S.c_major) { S.major = b; S.c_major = c[b]; }
  S.minor = -1; S.c_minor = -1;   // the greatest of the other three, the lower code at a tie
#pragma unroll
  for (int b = 0; b < 4; b++) if (b != S.major && c[b] > S.c_minor) { S.minor = b; S.c_minor = c[b]; }
  S.deep = S.depth >= P.min_depth;
  S.site = ob >= 0 && S.deep && S.c_minor >= P.min_minor && 100 * S.c_minor >= P.min_pct * S.depth && 100 * del <= P.max_del_pct * S.depth;
  return S;
}

struct AddOp { __device__ int32_t operator()(int32_t a, int32_t b) const { return a + b; } };

// FILL false: the site bytes, cnt[r] = n_sites and rows[r] = {n_sites, n_deep}.  FILL true: the rows of the list of the reads that have sites.
template <bool FILL>
__global__ __launch_bounds__(PILE_T) void site_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off,
                                                      const int64_t* __restrict__ read_pos, const int32_t* __restrict__ lengths,
                                                      const int32_t* __restrict__ order, const uint32_t* __restrict__ table, VParams P,
                                                      uint8_t* __restrict__ site, int32_t* __restrict__ cnt, int32_t* __restrict__ rows,
                                                      const int64_t* __restrict__ offsets, int64_t cap, int32_t* __restrict__ list) {
  __shared__ int32_t wl[PILE_LOADS][PILE_WAVES], wn[2][PILE_WAVES];
  const int32_t r = order[blockIdx.x];
  const int64_t len = lengths[r];
  int64_t first = 0;
  if (FILL) {
    first = offsets[r];
    if (offsets[r + 1] == first) return;
  }
  const uint8_t* __restrict__ own = bases + read_off[r];
  const uint32_t* __restrict__ w = table + (int64_t)VK_WORDS * read_pos[r];
  uint8_t* __restrict__ mine = site + read_pos[r];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t before = 0, n_site = 0, n_deep = 0;   // before: the sites of the tiles in front
  for (int64_t t0 = 0; t0 < len; t0 += MHAP_VARIANT_TILE) {
    Site S[PILE_LOADS];
    int32_t v[PILE_LOADS], ex[PILE_LOADS];
#pragma unroll
    for (int j = 0; j < PILE_LOADS; j++) {
      const int64_t t = t0 + j * PILE_T + tid;
      v[j] = 0;
      if (t < len) {
        S[j] = decide_site(w, len, t, own[t], P);
        v[j] = S[j].site;
        if (!FILL) {
          mine[t] = (uint8_t)(S[j].site | (S[j].site ? (S[j].major << 1) | (S[j].minor << 3) : 0));
          n_site += S[j].site; n_deep += S[j].deep;
        }
      }
    }
    if (FILL) {
      pile_scan_tile(v, lane, wave, wl, before, ex, AddOp());
#pragma unroll
      for (int j = 0; j < PILE_LOADS; j++) {
        const int64_t at = first + ex[j];
        if (v[j] && at < cap) {
          int32_t* o = list + 6 * at;
          o[0] = (int32_t)(t0 + j * PILE_T + tid); o[1] = S[j].major; o[2] = S[j].minor; o[3] = S[j].c_major; o[4] = S[j].c_minor; o[5] = S[j].depth;
        }
      }
      __syncthreads();   // wl has been read by everyone who comes here
    }
  }
  if (FILL) return;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) { n_site += __shfl_down(n_site, s); n_deep += __shfl_down(n_deep, s); }
  if (lane == 0) { wn[0][wave] = n_site; wn[1][wave] = n_deep; }
  __syncthreads();
  if (tid != 0) return;
  for (int u = 1; u < PILE_WAVES; u++) { n_site += wn[0][u]; n_deep += wn[1][u]; }
  cnt[r] = n_site;
  rows[2 * (int64_t)r] = n_site; rows[2 * (int64_t)r + 1] = n_deep;
}

// one record to judge: the walk's item (v_words is not used) and the first site byte of its two reads
struct JudgeItem { VoteItem it; int64_t site_a, site_b; };

__global__ __launch_bounds__(64) void judge_kernel(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ site,
                                                   const JudgeItem* __restrict__ items, const uint32_t* __restrict__ ops, VParams P,
                                                   int4* __restrict__ tallies, uint8_t* __restrict__ keep) {
  const JudgeItem J = items[blockIdx.x];
  const bool rc = J.it.rc != 0;
  int informative = 0, agree = 0, disagree = 0;   // (lane 0 is in every step of the walk: its sums are the record's)
  vote_walk<false, false>(bases, J.it, ops, (uint32_t*)nullptr, [&](bool diag, int i, int j) {
    bool inf = false, ag = false, dis = false;
    if (diag) {
      const int jb = rc ? J.it.blen - 1 - j : j;   // read B's own position
      int sa = site[J.site_a + i], sb = site[J.site_b + jb];
      if (rc) sb = (sb & 1) | ((3 - ((sb >> 1) & 3)) << 1) | ((3 - ((sb >> 3) & 3)) << 3);   // the alleles complemented
      const bool ia = sa & 1, ib = sb & 1;
      if (ia || ib) {
        inf = true;
        const int s = ia ? sa : sb, p0 = (s >> 1) & 3, p1 = (s >> 3) & 3;
        const int q0 = (sb >> 1) & 3, q1 = (sb >> 3) & 3;
        const bool one_pair = !(ia && ib) || (p0 == q0 && p1 == q1) || (p0 == q1 && p1 == q0);
        const uint32_t eb = bases[J.it.b_off + jb];
        const int ca = base_code(bases[J.it.a_off + i]), cb = base_code(rc ? rc_char(eb) : eb);
        const bool in = one_pair && (ca == p0 || ca == p1) && (cb == p0 || cb == p1);
        ag = in && ca == cb;
        dis = in && ca != cb;
      }
    }
    informative += __popcll(__ballot(inf)); agree += __popcll(__ballot(ag)); disagree += __popcll(__ballot(dis));
  });
  if (threadIdx.x == 0) {
    tallies[blockIdx.x] = make_int4(informative, agree, disagree, informative - agree - disagree);
    keep[blockIdx.x] = (uint8_t)!(disagree >= P.min_diff && 100 * (int64_t)disagree >= (int64_t)P.diff_pct * (agree + disagree));
  }
}

}  // namespace
}  // namespace mhap

using namespace mhap;

// the vote table and the reads are VoteTable's; the session's own: the order of the site kernel, the sites and the judge's buffers
struct mhap_variant_session : VoteTable {
  static constexpr const char* finish_name = "mhap_variant_finish";
  static constexpr int unfinished_rc = MHAP_E_INVALID;
  std::vector<int32_t> order;                           // the reads longest first
  int64_t accepted = 0, n_sites = 0;
  VParams P{};
  bool finished = false;
  DevBuf d_order, site, cnt, rows, soff, list, jitems, tallies, keep;
  void release() {
    release_table();
    for (DevBuf* b : {&d_order, &site, &cnt, &rows, &soff, &list, &jitems, &tallies, &keep}) b->release();
  }
};

extern "C" void mhap_variant_default_params(mhap_variant_params* p) {
  if (!p) return;
  p->min_depth = 8; p->min_minor = 3; p->min_pct = 25; p->max_del_pct = 25; p->min_diff = 2; p->diff_pct = 50;   // provisional (EXPERIMENTS.md, "Variant filter")
}

extern "C" int mhap_variant_begin(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                                  const int32_t* lengths, int64_t n_reads, const mhap_variant_params* params, mhap_variant_session** session) {
  const char* who = "mhap_variant_begin";
  if (session) *session = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!VoteTable::args_ok(v, who, session, bases, n_bases, read_ids, offsets, lengths, n_reads)) return MHAP_E_INVALID;
  if (n_reads > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 reads"; return MHAP_E_INVALID; }
  if (!VoteTable::reads_inside(v, who, n_bases, offsets, lengths, n_reads)) return MHAP_E_INVALID;
  mhap_variant_params p;
  mhap_variant_default_params(&p);
  if (params) p = *params;
  if (!variant_params_ok(p, who, *v.err)) return MHAP_E_INVALID;
  mhap_variant_session* s = new mhap_variant_session();
  s->P = VParams{p.min_depth, p.min_minor, p.min_pct, p.max_del_pct, p.min_diff, p.diff_pct};
  s->order.resize((size_t)n_reads);   // the long workgroups start early
  std::iota(s->order.begin(), s->order.end(), 0);
  std::stable_sort(s->order.begin(), s->order.end(), [&](int32_t a, int32_t b) { return lengths[a] > lengths[b]; });
  (void)hipSetDevice(v.device);
  hipError_t e = s->begin_table(v, h, VK_WORDS, bases, n_bases, read_ids, offsets, lengths, n_reads);
  const size_t np = (size_t)std::max<int64_t>(s->n_pos, 1), nr = (size_t)std::max<int64_t>(n_reads, 1);
  VoteTable::upload(v, e, s->d_order, s->order.data(), 4 * (size_t)n_reads);
  if (e == hipSuccess) e = s->site.ensure(np);
  if (e == hipSuccess) e = s->cnt.ensure(4 * nr);
  if (e == hipSuccess) e = s->rows.ensure(8 * nr);
  if (e == hipSuccess) e = s->soff.ensure(8 * (nr + 1));
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
  if (e != hipSuccess) {
    s->release();
    delete s;
    return hip_fail(v, who, "the vote table (12 bytes per base), the site bytes and the bases", e);
  }
  *session = s;
  return MHAP_OK;
}

extern "C" int mhap_variant_add(mhap_variant_session* s, const mhap_record* recs, int64_t n, const mhap_align_paths* paths) {
  const char* who = "mhap_variant_add";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = check_call(v, who, recs, n, paths, true);
  if (rc != MHAP_OK) return rc;
  if (s->finished) { *v.err = std::string(who) + ": mhap_variant_finish has completed, and its sites are those of the votes before it"; return MHAP_E_INVALID; }
  std::vector<VoteItem> items;
  if ((rc = s->build_items(v, who, recs, n, paths, nullptr, CK_CAP, items)) != MHAP_OK) return rc;
  s->accepted += (int64_t)items.size();
  if (items.empty()) return MHAP_OK;
  return s->cast_votes(v, who, paths, items, [&](unsigned c) {
    hipLaunchKernelGGL((vote_kernel<false, UnitWeight>), dim3(c), dim3(64), 0, v.stream, s->bases.as<uint8_t>(), s->items.as<VoteItem>(),
                       s->ops.as<uint32_t>(), s->table.as<uint32_t>(), UnitWeight());
  });
}

extern "C" int mhap_variant_votes(mhap_variant_session* s, int64_t read_index, uint16_t* counters) {
  if (!s) return MHAP_E_INVALID;
  return s->read_votes("mhap_variant_votes", read_index, counters);
}

extern "C" int mhap_variant_finish(mhap_variant_session* s, int64_t* counts) {
  const char* who = "mhap_variant_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  s->finished = false;
  s->n_sites = 0;
  std::vector<int32_t> rows(2 * (size_t)s->n_reads);
  if (s->n_reads > 0) {
    hipError_t e;
    const dim3 grid((unsigned)s->n_reads), wg(PILE_T);
    const uint8_t* bases = s->bases.as<uint8_t>();
    const int64_t *off = s->read_off.as<int64_t>(), *pos = s->read_pos.as<int64_t>();
    const int32_t *lens = s->read_len.as<int32_t>(), *order = s->d_order.as<int32_t>();
    hipLaunchKernelGGL(site_kernel<false>, grid, wg, 0, v.stream, bases, off, pos, lens, order, s->table.as<uint32_t>(), s->P, s->site.as<uint8_t>(),
                       s->cnt.as<int32_t>(), s->rows.as<int32_t>(), (const int64_t*)nullptr, (int64_t)0, (int32_t*)nullptr);
    hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->cnt.as<int32_t>(), s->n_reads, s->soff.as<int64_t>());
    if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
    e = hipMemcpyAsync(rows.data(), s->rows.p, 8 * (size_t)s->n_reads, hipMemcpyDeviceToHost, v.stream);
    const hipError_t es = hipStreamSynchronize(v.stream);
    if (e != hipSuccess) return hip_fail(v, who, "download", e);
    if (es != hipSuccess) return hip_fail(v, who, "kernel", es);
    for (int64_t r = 0; r < s->n_reads; r++) s->n_sites += rows[2 * (size_t)r];
    if (s->n_sites > 0) {   // the list is as long as the count says: the second walk fills it
      if ((e = s->list.ensure(24 * (size_t)s->n_sites)) != hipSuccess) return hip_fail(v, who, "hipMalloc of the site list", e);
      hipLaunchKernelGGL(site_kernel<true>, grid, wg, 0, v.stream, bases, off, pos, lens, order, s->table.as<uint32_t>(), s->P, (uint8_t*)nullptr,
                         (int32_t*)nullptr, (int32_t*)nullptr, s->soff.as<int64_t>(), s->n_sites, s->list.as<int32_t>());
      if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
      if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
    }
  }
  for (int k = 0; k < MHAP_VARIANT_COUNTS; k++) counts[k] = 0;
  for (int64_t r = 0; r < s->n_reads; r++) {
    counts[VC_SOME] += rows[2 * (size_t)r] > 0;
    counts[VC_DEEP] += rows[2 * (size_t)r + 1];
  }
  counts[VC_READS] = s->n_reads; counts[VC_SITES] = s->n_sites; counts[VC_BASES] = s->n_pos;
  counts[VC_ACCEPTED] = s->accepted; counts[VC_SKIPPED] = s->skipped;
  s->finished = true;
  return MHAP_OK;
}

extern "C" int mhap_variant_copy(mhap_variant_session* s, int32_t* rows, int64_t* offsets, int32_t* sites) {
  const char* who = "mhap_variant_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = check_finished(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (!offsets || (s->n_reads > 0 && !rows) || (s->n_sites > 0 && !sites)) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  offsets[0] = 0;
  (void)hipSetDevice(v.device);
  hipError_t e = hipSuccess;
  if (s->n_reads > 0) e = hipMemcpyAsync(offsets, s->soff.p, 8 * ((size_t)s->n_reads + 1), hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess && s->n_reads > 0) e = hipMemcpyAsync(rows, s->rows.p, 8 * (size_t)s->n_reads, hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess && s->n_sites > 0) e = hipMemcpyAsync(sites, s->list.p, 24 * (size_t)s->n_sites, hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);
  if (e != hipSuccess || es != hipSuccess) return hip_fail(v, who, "download", e != hipSuccess ? e : es);
  return MHAP_OK;
}

extern "C" int mhap_variant_apply(mhap_variant_session* s, const mhap_record* recs, int64_t n, const mhap_align_paths* paths, uint8_t* keep,
                                  int32_t* tallies) {
  const char* who = "mhap_variant_apply";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = check_finished(s, v, who);
  if (rc != MHAP_OK) return rc;
  if ((rc = check_call(v, who, recs, n, paths, n == 0 || (keep && tallies))) != MHAP_OK) return rc;
  if (n == 0) return MHAP_OK;
  std::vector<JudgeItem> items((size_t)n);
  for (int64_t q = 0; q < n; q++) {
    const mhap_record& r = recs[q];
    int64_t idx[2], i0, j0;
    bool walk;
    if ((rc = s->check_record(v, who, q, r, paths, idx, i0, j0, walk)) != MHAP_OK) return rc;
    JudgeItem J{};   // (a record that takes no part: no runs, no column, four zeros and keep = 1)
    if (walk) {
      J.it = s->item_of(r, paths, q, idx, i0, j0);
      J.site_a = s->pos[(size_t)idx[0]]; J.site_b = s->pos[(size_t)idx[1]];
    }
    items[(size_t)q] = J;
  }
  (void)hipSetDevice(v.device);
  hipError_t e;
  constexpr size_t CHUNK = (size_t)1 << 20;
  const size_t nc = std::min((size_t)n, CHUNK);
  if ((e = s->ops.ensure(std::max<size_t>(4 * paths->ops.size(), 4))) != hipSuccess) return hip_fail(v, who, "hipMalloc of the runs", e);
  if ((e = s->jitems.ensure(sizeof(JudgeItem) * nc)) != hipSuccess || (e = s->tallies.ensure(16 * nc)) != hipSuccess || (e = s->keep.ensure(nc)) != hipSuccess)
    return hip_fail(v, who, "hipMalloc of the records", e);
  if (!paths->ops.empty() && (e = hipMemcpyAsync(s->ops.p, paths->ops.data(), 4 * paths->ops.size(), hipMemcpyHostToDevice, v.stream)) != hipSuccess)
    return hip_fail(v, who, "upload", e);
  for (size_t g0 = 0; g0 < (size_t)n; g0 += CHUNK) {
    const size_t c = std::min(CHUNK, (size_t)n - g0);
    if ((e = hipMemcpyAsync(s->jitems.p, items.data() + g0, sizeof(JudgeItem) * c, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
    hipLaunchKernelGGL(judge_kernel, dim3((unsigned)c), dim3(64), 0, v.stream, s->bases.as<uint8_t>(), s->site.as<uint8_t>(), s->jitems.as<JudgeItem>(),
                       s->ops.as<uint32_t>(), s->P, s->tallies.as<int4>(), s->keep.as<uint8_t>());
    if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
    if ((e = hipMemcpyAsync(tallies + 4 * g0, s->tallies.p, 16 * c, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
        (e = hipMemcpyAsync(keep + g0, s->keep.p, c, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) {
      (void)hipStreamSynchronize(v.stream);
      return hip_fail(v, who, "download", e);
    }
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  }
  return MHAP_OK;
}

extern "C" void mhap_variant_free(mhap_variant_session* s) {
  if (!s) return;
  HandleView v = handle_view(s->h);
  (void)hipSetDevice(v.device);
  (void)hipStreamSynchronize(v.stream);
  s->release();
  delete s;
}
