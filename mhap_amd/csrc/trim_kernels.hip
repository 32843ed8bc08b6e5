// trim_kernels.hip — reads cut to the part that other reads support (mhap_trim_begin / _add / _finish / _copy / _coverage / _apply /
// _clip_record / _refine / _refine_record / _free).  The contract — eligible records, the intervals they contribute, coverage, runs, the clear range, the
// per-read row and a record rewritten onto the trimmed reads — is the prose of include/mhap_hip.h ("read trimming");
// tests/trim_ref.py restates it.  The rules host and device share are trim_common.hpp's.
//
// begin: read r owns lengths[r] + 1 int32 slots of one difference array, at an offset rounded up to four slots (so that a read's
//        slots begin on a 16-byte word); the array is zeroed once.
// The difference array, the add and the tile's coverage scan are pileup_common.hpp's, shared with the repeat marking.
// add:   the host finds every record's two reads (and refuses the call before anything is queued), packs the record into 32 bytes
//        (GItem) and queues one upload and add_kernel, one lane per record: +1 at an interval's begin, -1 at its end, up to four
//        atomicAdd(int32).  Integer adds commute, so the array is a function of the multiset of records.  Nothing waits; the items'
//        device buffer is reused by the next add, which the stream orders behind this one.
// finish: run_kernel, one workgroup of 256 lanes per read, longest reads first.  It walks the read in tiles of MHAP_TRIM_TILE
//        positions: four 16-byte loads per lane, each contiguous across the wave, so a lane holds four groups of four positions and
//        the order of a tile is (load j, lane, k).  A wave scan of the lanes' sums and the 16 (j, wave) totals in LDS turn
//        differences into coverage; cov[p - 1] = cov[p] - diff[p], so a run's first position (in, the one before out) and the
//        position behind its last (out, the one before in) are found without a neighbour.  A second scan of the same shape, a
//        running maximum of the first positions, gives every end its begin.  Carried from tile to tile: the coverage at the tile's
//        end and the begin of the latest run.  A lane keeps the best (length, begin) of the ends it has seen, the runs it has
//        begun and the positions it has counted; they are reduced once per read.  cov[length] = 0, so every run has ended by then.
//        Lane 0 writes the row and the flag byte and adds the read to the counts.
// apply: one lane per packed record with trim_clip; the host puts the six rewritten fields into a copy of the record.
// refine (mhap_trim_refine, in front of the add): one lane per record walks the record's runs once with trim_refine and gives the
//        ends, columns and errors of the best stretch; the runs of a call are uploaded for it and freed behind it.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_common.hpp"
#include "graph_class.hpp"
#include "mhap_internal.hpp"
#include "pileup_common.hpp"
#include "trim_common.hpp"

namespace mhap {
namespace {

// counts: reads, deleted, cut5, cut3, gapped, bases in, bases kept, eligible records
enum { TC_READS = 0, TC_DELETED, TC_CUT5, TC_CUT3, TC_GAPPED, TC_BASES_IN, TC_BASES_KEPT, TC_ELIGIBLE };
static_assert(TC_ELIGIBLE + 1 == MHAP_TRIM_COUNTS, "the counts of the header");
enum { TRIM_T = PILE_T, TRIM_WAVES = PILE_WAVES, TRIM_LOADS = PILE_LOADS };
static_assert(PILE_TILE == MHAP_TRIM_TILE, "a tile is four 16-byte loads per lane");

__global__ __launch_bounds__(TRIM_T) void run_kernel(const int32_t* __restrict__ diff, const int64_t* __restrict__ off,
                                                     const int32_t* __restrict__ lengths, const int32_t* __restrict__ order, TParams P,
                                                     int32_t* __restrict__ rows, uint8_t* __restrict__ flags, u64* __restrict__ counts) {
  __shared__ int32_t ws[TRIM_LOADS][TRIM_WAVES], wm[TRIM_LOADS][TRIM_WAVES], wr[TRIM_WAVES], wc[TRIM_WAVES];
  __shared__ u64 wb[TRIM_WAVES];
  const int32_t r = order[blockIdx.x], len = lengths[r];
  const int64_t groups = ((int64_t)len + 4) >> 2;   // 16-byte words that hold the read's len + 1 slots
  const int4* __restrict__ base = (const int4*)(diff + off[r]);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t carry = 0, open_begin = -1, runs = 0, covered = 0;
  u64 best = 0;   // (length << 32) | (2^32 - 1 - begin): the longest run, the first of equal ones
  for (int64_t g0 = 0; g0 < groups; g0 += TRIM_T * TRIM_LOADS) {
    int4 d[TRIM_LOADS];
    int32_t c0[TRIM_LOADS];
    pile_coverage_tile(base, groups, g0, tid, lane, wave, ws, carry, d, c0);   // (its barrier: wm of the tile before has been read by everyone who comes here)
    // pass 1: coverage, the counts, and the latest first position of a run in each of the lane's groups
    int32_t m[TRIM_LOADS], minc[TRIM_LOADS], mpre[TRIM_LOADS];
#pragma unroll
    for (int j = 0; j < TRIM_LOADS; j++) {
      const int32_t p0 = (int32_t)((g0 + j * TRIM_T + tid) << 2);
      int32_t c = c0[j];
      m[j] = -1;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int32_t before = c;
        c += quad(d[j], k);
        const bool in = c >= P.min_cov, was = before >= P.min_cov;
        covered += in;
        if (in && !was) { runs++; m[j] = p0 + k; }
      }
      minc[j] = m[j];
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
      for (int j = 0; j < TRIM_LOADS; j++) {
        const int32_t u = __shfl_up(minc[j], s);
        if (lane >= s && u > minc[j]) minc[j] = u;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int j = 0; j < TRIM_LOADS; j++) wm[j][wave] = minc[j];
    }
    __syncthreads();   // (ws has been read by everyone who comes here)
    int32_t macc = open_begin;
#pragma unroll
    for (int j = 0; j < TRIM_LOADS; j++) {
#pragma unroll
      for (int w = 0; w < TRIM_WAVES; w++) {
        if (w == wave) mpre[j] = macc;
        if (wm[j][w] > macc) macc = wm[j][w];
      }
    }
    open_begin = macc;
    // pass 2: every position behind a run's last closes the run that began latest
#pragma unroll
    for (int j = 0; j < TRIM_LOADS; j++) {
      const int32_t p0 = (int32_t)((g0 + j * TRIM_T + tid) << 2);
      const int32_t left = __shfl_up(minc[j], 1);
      int32_t cur = lane > 0 && left > mpre[j] ? left : mpre[j];
      int32_t c = c0[j];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int32_t before = c;
        c += quad(d[j], k);
        const bool in = c >= P.min_cov, was = before >= P.min_cov;
        if (in && !was) cur = p0 + k;
        if (!in && was && cur >= 0) {
          const u64 key = ((u64)(uint32_t)(p0 + k - cur) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)cur);
          if (key > best) best = key;
        }
      }
    }
  }
  // the read's best run, runs and covered positions: over the wave, then over the waves
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const u64 b = __shfl_down(best, s);
    if (b > best) best = b;
    runs += __shfl_down(runs, s);
    covered += __shfl_down(covered, s);
  }
  if (lane == 0) { wb[wave] = best; wr[wave] = runs; wc[wave] = covered; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < TRIM_WAVES; w++) {
    if (wb[w] > best) best = wb[w];
    runs += wr[w];
    covered += wc[w];
  }
  int32_t begin = 0, end = 0;
  uint8_t f = TRIM_DELETED;
  if (best != 0) {
    const int32_t s = (int32_t)(0xFFFFFFFFu - (uint32_t)best), e = s + (int32_t)(best >> 32);
    begin = s - P.end_clip; end = e + P.end_clip;
    f = (begin > 0 ? TRIM_CUT5 : 0) | (end < len ? TRIM_CUT3 : 0) | (runs > 1 ? TRIM_GAPPED : 0);
  }
  ((int4*)rows)[r] = make_int4(begin, end, runs, covered);
  flags[r] = f;
  if (f & TRIM_DELETED) atomicAdd(counts + TC_DELETED, (u64)1);
  if (f & TRIM_CUT5) atomicAdd(counts + TC_CUT5, (u64)1);
  if (f & TRIM_CUT3) atomicAdd(counts + TC_CUT3, (u64)1);
  if (f & TRIM_GAPPED) atomicAdd(counts + TC_GAPPED, (u64)1);
  if (end > begin) atomicAdd(counts + TC_BASES_KEPT, (u64)(end - begin));
}

// out: two 16-byte words per record, {a1, a2, b1, b2} and {alen, blen, keep, 0}
__global__ __launch_bounds__(256) void apply_kernel(const int4* __restrict__ items, int64_t n, const int32_t* __restrict__ lengths,
                                                    const int32_t* __restrict__ rows, const uint8_t* __restrict__ flags, TParams P,
                                                    int4* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
  const int32_t A = w0.x, B = w0.y >> 1, o = w0.y & 1;
  TClip c{w0.z, w0.w, lengths[A], w1.x, w1.y, lengths[B]};
  bool keep = trim_eligible(A, B, __hiloint2double(w1.w, w1.z), P) && !(flags[A] & TRIM_DELETED) && !(flags[B] & TRIM_DELETED);
  if (keep) {
    const int4 ra = ((const int4*)rows)[A], rb = ((const int4*)rows)[B];
    keep = trim_clip(w0.z, w0.w, w1.x, w1.y, o, lengths[B], ra.x, ra.y, rb.x, rb.y, c);
  }
  out[2 * q] = make_int4(c.a1, c.a2, c.b1, c.b2);
  out[2 * q + 1] = make_int4(c.alen, c.blen, keep ? 1 : 0, 0);
}

// one lane per record: the record's ends and identity become those of the best sub-path of its path (trim_refine)
struct RItem { int32_t a1, b1, b2, blen, to_rc, pad; int64_t op0, op1; };
static_assert(sizeof(RItem) == 40, "a refine item");
__global__ __launch_bounds__(256) void refine_kernel(const RItem* __restrict__ items, int64_t n, const uint32_t* __restrict__ ops, int32_t penalty,
                                                     int4* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const RItem it = items[q];
  const int64_t ts = it.to_rc ? (int64_t)it.blen - it.b2 - 1 : (int64_t)it.b1;
  TRefined r;
  const bool ok = trim_refine(ops + it.op0, it.op1 - it.op0, it.a1, ts, penalty, r);
  if (!ok) { out[2 * q] = make_int4(0, 0, 0, 0); out[2 * q + 1] = make_int4(0, 0, 0, 0); return; }
  const int32_t b1 = (int32_t)(it.to_rc ? it.blen - r.te : r.ts), b2 = (int32_t)(it.to_rc ? it.blen - r.ts - 1 : r.te - 1);
  out[2 * q] = make_int4((int32_t)r.qs, (int32_t)(r.qe - 1), b1, b2);
  out[2 * q + 1] = make_int4((int32_t)r.columns, (int32_t)r.errors, 1, 0);
}

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_trim_session : Pile {
  static constexpr const char* finish_name = "mhap_trim_finish";
  static constexpr int unfinished_rc = MHAP_E_INVALID;
  TParams P{};
  bool finished = false;
  DevBuf rows, flags, counts, applied;   // counts: MHAP_TRIM_COUNTS x uint64
  void release() {
    release_pile();
    for (DevBuf* b : {&rows, &flags, &counts, &applied}) b->release();
  }
};

namespace {

bool params_ok(const mhap_trim_params& p) { return p.min_cov >= 1 && p.end_clip >= 0 && p.min_span >= 0; }

}  // namespace

extern "C" void mhap_trim_default_params(mhap_trim_params* p) {
  if (!p) return;
  p->min_cov = 3; p->end_clip = 500; p->min_span = 2000; p->min_identity = 0.0;
}

extern "C" int mhap_trim_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_trim_params* params,
                               mhap_trim_session** session) {
  return session_begin("mhap_trim_begin", h, read_ids, lengths, n_reads, params, mhap_trim_default_params, params_ok,
                       "min_cov must be >= 1, end_clip and min_span >= 0", session,
                       [&](mhap_trim_session& s, const mhap_trim_params& p, const HandleView& v) {
    s.P = TParams{p.min_cov, p.end_clip, p.min_span, p.min_identity};
    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1);
    Steps q{s.begin_pile(v, h, read_ids, lengths, n_reads), v.stream};
    q.ensure(s.rows, 16 * nr);
    q.ensure(s.flags, nr);
    q.ensure(s.counts, 8 * MHAP_TRIM_COUNTS);
    q.zero(s.counts, 8 * MHAP_TRIM_COUNTS);
    return q.e;
  });
}

extern "C" int mhap_trim_add(mhap_trim_session* s, const mhap_record* recs, int64_t n) {
  const char* who = "mhap_trim_add";
  if (!s) return MHAP_E_INVALID;
  return s->add_records(who, recs, n, s->P, s->counts.as<u64>() + TC_ELIGIBLE);
}

extern "C" int mhap_trim_finish(mhap_trim_session* s, int64_t* counts) {
  const char* who = "mhap_trim_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  s->finished = false;
  hipError_t e;
  u64* d_counts = s->counts.as<u64>();
  // the counts of this finish; the eligible records are summed over the adds and stay
  if ((e = hipMemsetAsync(d_counts, 0, 8 * TC_ELIGIBLE, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if (s->n_reads > 0) {
    hipLaunchKernelGGL(run_kernel, dim3((unsigned)s->n_reads), dim3(TRIM_T), 0, v.stream, s->diff.as<int32_t>(), s->d_off.as<int64_t>(),
                       s->d_lengths.as<int32_t>(), s->d_order.as<int32_t>(), s->P, s->rows.as<int32_t>(), s->flags.as<uint8_t>(), d_counts);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
  }
  u64 hc[MHAP_TRIM_COUNTS];
  if ((e = hipMemcpyAsync(hc, d_counts, sizeof hc, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
  s->reap(true);   // the stream is empty: every upload has been read
  for (int k = 0; k < MHAP_TRIM_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[TC_READS] = s->n_reads;
  counts[TC_BASES_IN] = s->bases_in;
  s->finished = true;
  return MHAP_OK;
}

extern "C" int mhap_trim_copy(mhap_trim_session* s, int32_t* rows, uint8_t* flags) {
  const char* who = "mhap_trim_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  int rc = check_finished(s, v, who);
  if (rc != MHAP_OK || s->n_reads == 0) return rc;
  if (!rows || !flags) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  rc = s->download(who, rows, s->rows.p, 16 * (size_t)s->n_reads);
  return rc != MHAP_OK ? rc : s->download(who, flags, s->flags.p, (size_t)s->n_reads);
}

extern "C" int mhap_trim_coverage(mhap_trim_session* s, int64_t read_index, int32_t* cov) {
  const char* who = "mhap_trim_coverage";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (read_index < 0 || read_index >= s->n_reads) { *v.err = std::string(who) + ": no such read"; return MHAP_E_INVALID; }
  const int64_t len = s->lengths[(size_t)read_index];
  if (len == 0) return MHAP_OK;
  if (!cov) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  const int rc = s->download(who, cov, s->diff.as<int32_t>() + s->slot_off[(size_t)read_index], 4 * (size_t)len);
  if (rc != MHAP_OK) return rc;
  for (int64_t p = 1; p < len; p++) cov[p] += cov[p - 1];   // the differences as the add kernel left them, summed here
  return MHAP_OK;
}

extern "C" int mhap_trim_apply(mhap_trim_session* s, const mhap_record* in, int64_t n, mhap_record* out, uint8_t* keep) {
  const char* who = "mhap_trim_apply";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  std::vector<GItem> items;
  int rc = apply_begin(s, v, who, in, n, out && keep, items, s->applied, 32 * (size_t)n, "hipMalloc of the records");
  if (rc != MHAP_OK || n == 0) return rc;
  hipLaunchKernelGGL(apply_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, s->items.as<int4>(), n, s->d_lengths.as<int32_t>(),
                     s->rows.as<int32_t>(), s->flags.as<uint8_t>(), s->P, s->applied.as<int4>());
  std::vector<int32_t> got(8 * (size_t)n);
  if ((rc = apply_end(v, who, got.data(), s->applied, 32 * (size_t)n)) != MHAP_OK) return rc;
  for (int64_t q = 0; q < n; q++) {
    const int32_t* g = got.data() + 8 * (size_t)q;
    out[q] = in[q];
    keep[q] = (uint8_t)g[6];
    if (g[6]) { out[q].a1 = g[0]; out[q].a2 = g[1]; out[q].b1 = g[2]; out[q].b2 = g[3]; out[q].alen = g[4]; out[q].blen = g[5]; }
  }
  return MHAP_OK;
}

extern "C" int mhap_trim_clip_record(const mhap_record* in, const int32_t* clearA, const int32_t* clearB, const mhap_trim_params* params,
                                     mhap_record* out) {
  if (!in || !clearA || !clearB || !out) return -1;
  mhap_trim_params p;
  mhap_trim_default_params(&p);
  if (params) p = *params;
  if (!params_ok(p)) return -1;
  const TParams P{p.min_cov, p.end_clip, p.min_span, p.min_identity};
  *out = *in;
  TClip c;
  if (!trim_eligible(in->from_id, in->to_id, in->score, P) ||
      !trim_clip(in->a1, in->a2, in->b1, in->b2, in->to_rc != 0, in->blen, clearA[0], clearA[1], clearB[0], clearB[1], c)) return 0;
  out->a1 = c.a1; out->a2 = c.a2; out->alen = c.alen; out->b1 = c.b1; out->b2 = c.b2; out->blen = c.blen;
  return 1;
}

namespace {

void refined_record(const mhap_record& in, const TRefined& r, mhap_record& out) {
  out = in;
  out.a1 = (int32_t)r.qs; out.a2 = (int32_t)(r.qe - 1);
  out.b1 = (int32_t)(in.to_rc ? in.blen - r.te : r.ts); out.b2 = (int32_t)(in.to_rc ? in.blen - r.ts - 1 : r.te - 1);
  out.score = 1.0 - (double)r.errors / (double)r.columns;
}

}  // namespace

extern "C" int mhap_trim_refine_record(const mhap_record* in, const uint32_t* ops, int64_t n_ops, int32_t penalty, mhap_record* out) {
  if (!in || !out || n_ops < 0 || (n_ops > 0 && !ops) || penalty < 1) return -1;
  *out = *in;
  TRefined r;
  const int64_t ts = in->to_rc ? (int64_t)in->blen - in->b2 - 1 : (int64_t)in->b1;
  if (!trim_refine(ops, n_ops, in->a1, ts, penalty, r)) return 0;
  refined_record(*in, r, *out);
  return 1;
}

extern "C" int mhap_trim_refine(mhap_handle* h, const mhap_record* recs, int64_t n, const mhap_align_paths* paths, int32_t penalty, mhap_record* out) {
  const char* who = "mhap_trim_refine";
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (n < 0 || (n > 0 && (!recs || !out)) || !paths || penalty < 1) { *v.err = std::string(who) + ": null or negative argument, or penalty < 1"; return MHAP_E_INVALID; }
  if ((int64_t)paths->offsets.size() != n + 1) { *v.err = std::string(who) + ": the paths are those of another number of records"; return MHAP_E_INVALID; }
  if (n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records in one call"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  const int64_t n_ops = paths->offsets[(size_t)n];
  std::vector<RItem> items((size_t)n);
  for (int64_t q = 0; q < n; q++) {
    const mhap_record& r = recs[q];
    const int64_t o0 = paths->offsets[(size_t)q], o1 = paths->offsets[(size_t)q + 1];
    if (o0 < 0 || o1 < o0 || o1 > n_ops || o1 > (int64_t)paths->ops.size()) { *v.err = std::string(who) + ": record " + std::to_string(q) + " has runs outside the paths"; return MHAP_E_INVALID; }
    items[(size_t)q] = RItem{r.a1, r.b1, r.b2, r.blen, r.to_rc != 0 ? 1 : 0, 0, o0, o1};
  }
  (void)hipSetDevice(v.device);
  DevBuf d_items, d_ops, d_out;
  hipError_t e = d_items.ensure(sizeof(RItem) * (size_t)n);
  if (e == hipSuccess) e = d_ops.ensure(4 * (size_t)std::max<int64_t>(n_ops, 1));
  if (e == hipSuccess) e = d_out.ensure(32 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_items.p, items.data(), sizeof(RItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess && n_ops > 0) e = hipMemcpyAsync(d_ops.p, paths->ops.data(), 4 * (size_t)n_ops, hipMemcpyHostToDevice, v.stream);
  std::vector<int32_t> got(8 * (size_t)n);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(refine_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, d_items.as<RItem>(), n, d_ops.as<uint32_t>(), penalty, d_out.as<int4>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), d_out.p, 32 * (size_t)n, hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);   // (the uploads read host vectors of this call: waited for whatever happened)
  if (e == hipSuccess) e = es;
  d_items.release(); d_ops.release(); d_out.release();
  if (e != hipSuccess) return hip_fail(v, who, "upload, kernel or download", e);
  for (int64_t q = 0; q < n; q++) {
    const int32_t* g = got.data() + 8 * (size_t)q;
    out[q] = recs[q];
    if (!g[6]) continue;   // no '=' column (a record without an alignment): as it came
    out[q].a1 = g[0]; out[q].a2 = g[1]; out[q].b1 = g[2]; out[q].b2 = g[3];
    out[q].score = 1.0 - (double)g[5] / (double)g[4];
  }
  return MHAP_OK;
}

extern "C" void mhap_trim_free(mhap_trim_session* s) { session_free(s); }
