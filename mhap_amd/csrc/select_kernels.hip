// select_kernels.hip — overlap selection: every read keeps the best_n views with the greatest keys (mhap_select_begin / _add / _finish /
// _copy / _apply / _judge_record / _free).  The contract — eligible records, the two views of a record, the key, the threshold and
// the per-read row — is the prose of include/mhap_hip.h ("overlap selection"); tests/select_ref.py restates it.  The key is
// select_common.hpp's; the table of reads, the record checks and the begin / apply / free of a session are read_table.hpp's, shared
// with the trimming and the repeat marking; no per-base array exists here.
//
// add:    entry_kernel, one lane per record: the record's two entries {read or -1, key} go to the fixed slots 2 (records so far + q)
//         and + 1 in one 16-byte store, and count[read] takes an atomicAdd of 1 per entry.  Nothing waits (but the entries' buffer
//         doubles when it is full, and the copy into the larger one is waited for).
// finish: scan_kernel turns the counts into the segments' offsets; scatter_kernel, one lane per slot, puts every entry's key into its
//         read's segment at a place an atomic cursor hands out (the order inside a segment is arbitrary, and nothing below depends on
//         it); rows_kernel, one lane per read, writes the row of a read with at most best_n entries and puts the others on a work
//         list; select_kernel, workgroups of 256 that take the list's reads in turn, finds the best_n-th greatest key of a segment by
//         a radix select, most significant byte first: 256 bins in LDS per pass, a suffix sum over the bins from the top finds the
//         bin that holds the place, and the next pass looks only at the keys of that bin.  A bin that holds one key ends the search:
//         that key is found in one more walk without bins.  The keys strictly above the threshold are the sum of what lay above the
//         chosen bin in every pass, so `kept` needs no walk of its own.  A segment of at most SEL_LDS_KEYS keys is read from HBM
//         once and stays in LDS; a longer one is streamed once per pass.  Every row has one writer.  The host waits once, for the
//         counts.
// apply:  one lane per packed record: the two keys again and two loads of thr.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "device_common.hpp"
#include "graph_class.hpp"
#include "mhap_internal.hpp"
#include "read_table.hpp"
#include "select_common.hpp"

namespace mhap {
namespace {

// counts: reads, reads with an entry, reads with more than best_n entries, entries, kept entries, eligible records
enum { SC_READS = 0, SC_SOME, SC_OVER, SC_ENTRIES, SC_KEPT, SC_ELIGIBLE };
static_assert(SC_ELIGIBLE + 1 == MHAP_SELECT_COUNTS, "the counts of the header");

enum { SEL_T = 256, SEL_WAVES = SEL_T / 64, SEL_LDS_KEYS = MHAP_SELECT_LDS_KEYS };
static_assert(SEL_T == 256, "one lane per bin");

__device__ inline int64_t wave_sum(int64_t x) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) x += __shfl_down(x, s);
  return x;   // (lane 0's)
}

// entries: the slots of this add, entries[2 q] = view A, entries[2 q + 1] = view B of record q as {read, key}, {-1, 0} for no view
__global__ __launch_bounds__(256) void entry_kernel(const int4* __restrict__ items, int64_t n, int64_t n_reads, SParams P,
                                                    int4* __restrict__ entries, int32_t* __restrict__ count, u64* __restrict__ eligible) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool el = false;
  if (q < n) {
    const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
    const int32_t A = w0.x, B = w0.y >> 1;
    const double score = __hiloint2double(w1.w, w1.z);
    el = select_eligible(A, B, score, P.min_identity);
    // (the host has refused reads outside the table; the bounds are looked at again where the add is)
    const uint32_t ka = el && A >= 0 && A < n_reads ? select_key(w0.z, w0.w, score, P.min_span) : 0u;
    const uint32_t kb = el && B >= 0 && B < n_reads ? select_key(w1.x, w1.y, score, P.min_span) : 0u;
    entries[q] = make_int4(ka ? A : -1, (int32_t)ka, kb ? B : -1, (int32_t)kb);
    if (ka) atomicAdd(count + A, 1);
    if (kb) atomicAdd(count + B, 1);
  }
  const u64 m = __ballot(el);   // one add per wave
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(eligible, (u64)__popcll(m));
}

__global__ __launch_bounds__(256) void scatter_kernel(const int2* __restrict__ entries, int64_t n_slots, int64_t n_reads,
                                                      const int64_t* __restrict__ offsets, int32_t* __restrict__ cursor,
                                                      uint32_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_slots) return;
  const int2 ent = entries[e];
  if (ent.x < 0 || ent.x >= n_reads) return;
  const int64_t at = offsets[ent.x] + atomicAdd(cursor + ent.x, 1);
  if (at < offsets[ent.x + 1]) keys[at] = (uint32_t)ent.y;
}

// the row of every read with at most best_n entries: all of them kept, thr = 1; the others go on the work list, in any order
__global__ __launch_bounds__(256) void rows_kernel(const int32_t* __restrict__ count, int64_t n_reads, const int64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ keys, int32_t best_n, int32_t* __restrict__ rows,
                                                   int32_t* __restrict__ work, int32_t* __restrict__ n_work, u64* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int32_t E = r < n_reads ? count[r] : 0;
  const bool small = r < n_reads && E <= best_n;
  if (small) {
    const int64_t o = offsets[r];
    uint32_t top = 0;
    for (int32_t i = 0; i < E; i++) {
      const uint32_t k = keys[o + i];
      if (k > top) top = k;
    }
    ((int4*)rows)[r] = make_int4(E, E, 1, (int32_t)top);
  } else if (r < n_reads) {
    work[atomicAdd(n_work, 1)] = (int32_t)r;
  }
  const u64 some = __ballot(small && E > 0);
  const int64_t sum = wave_sum(small ? (int64_t)E : 0);
  if ((threadIdx.x & 63) == 0 && some) {
    atomicAdd(counts + SC_SOME, (u64)__popcll(some));
    atomicAdd(counts + SC_ENTRIES, (u64)sum);
    atomicAdd(counts + SC_KEPT, (u64)sum);
  }
}

// One workgroup per listed read at a time (every one has more than best_n entries): thr = its best_n-th greatest key, kept = the
// keys >= thr, top = its greatest key.
__global__ __launch_bounds__(SEL_T) void select_kernel(const uint32_t* __restrict__ keys, const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ work, const int32_t* __restrict__ n_work, int32_t best_n,
                                                       int32_t* __restrict__ rows, u64* __restrict__ counts) {
  __shared__ uint32_t seg[SEL_LDS_KEYS];
  __shared__ uint32_t bins[256], wsum[SEL_WAVES], wtop[SEL_WAVES], pick[4], found;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t listed = *n_work;
  for (int32_t w = blockIdx.x; w < listed; w += gridDim.x) {
    const int32_t r = work[w];
    const int64_t o = offsets[r], E = offsets[r + 1] - o;
    const uint32_t* __restrict__ src = keys + o;
    const bool in_lds = E <= SEL_LDS_KEYS;
    if (in_lds)
      for (int64_t i = tid; i < E; i += SEL_T) seg[i] = src[i];
    uint32_t k = (uint32_t)best_n, prefix = 0, mask = 0, greater = 0, ties = 0, thr = 0, top = 0;
    for (int p = 3; p >= 0; p--) {
      const int shift = 8 * p;
      bins[tid] = 0;
      __syncthreads();   // (and the segment is in LDS)
      for (int64_t i = tid; i < E; i += SEL_T) {
        const uint32_t key = in_lds ? seg[i] : src[i];
        if ((key & mask) == prefix) atomicAdd(&bins[(key >> shift) & 255u], 1u);
        if (p == 3 && key > top) top = key;
      }
      __syncthreads();
      // lane order is bin order from the top: after the scan, incl = the keys of this pass in the bins b .. 255
      const uint32_t b = 255u - (uint32_t)tid, c = bins[b];
      uint32_t incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(incl, d);
        if (lane >= d) incl += u;
      }
      if (lane == 63) wsum[wave] = incl;
      __syncthreads();
      for (int u = 0; u < wave; u++) incl += wsum[u];
      // the pass's keys number at least k, so exactly one bin holds the k-th greatest of them
      if (incl >= k && incl - c < k) { pick[0] = b; pick[1] = k - (incl - c); pick[2] = c; pick[3] = incl - c; }
      __syncthreads();
      prefix |= pick[0] << shift;
      mask |= 255u << shift;
      k = pick[1];
      greater += pick[3];
      ties = pick[2];
      if (p == 0) { thr = prefix; break; }
      if (ties == 1) {   // the bin is decided: its one key is the threshold
        for (int64_t i = tid; i < E; i += SEL_T) {
          const uint32_t key = in_lds ? seg[i] : src[i];
          if ((key & mask) == prefix) found = key;
        }
        __syncthreads();
        thr = found;
        break;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const uint32_t t = __shfl_down(top, s);
      if (t > top) top = t;
    }
    if (lane == 0) wtop[wave] = top;
    __syncthreads();   // (and every lane has read pick and found)
    if (tid == 0) {
      for (int u = 1; u < SEL_WAVES; u++) if (wtop[u] > top) top = wtop[u];
      const uint32_t kept = greater + ties;
      ((int4*)rows)[r] = make_int4((int32_t)E, (int32_t)kept, (int32_t)thr, (int32_t)top);
      atomicAdd(counts + SC_SOME, (u64)1);
      atomicAdd(counts + SC_OVER, (u64)1);
      atomicAdd(counts + SC_ENTRIES, (u64)E);
      atomicAdd(counts + SC_KEPT, (u64)kept);
    }
    __syncthreads();   // (wtop and the segment have been read before the next read's are written)
  }
}

__global__ __launch_bounds__(256) void view_kernel(const int4* __restrict__ items, int64_t n, int64_t n_reads, SParams P,
                                                   const int32_t* __restrict__ rows, uint8_t* __restrict__ views) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const int4 w0 = items[2 * q], w1 = items[2 * q + 1];
  const int32_t A = w0.x, B = w0.y >> 1;
  const double score = __hiloint2double(w1.w, w1.z);
  uint8_t bits = 0;
  if (select_eligible(A, B, score, P.min_identity) && A >= 0 && A < n_reads && B >= 0 && B < n_reads) {
    const uint32_t ka = select_key(w0.z, w0.w, score, P.min_span), kb = select_key(w1.x, w1.y, score, P.min_span);
    if (ka && ka >= (uint32_t)rows[4 * (int64_t)A + 2]) bits |= MHAP_SELECT_A;
    if (kb && kb >= (uint32_t)rows[4 * (int64_t)B + 2]) bits |= MHAP_SELECT_B;
  }
  views[q] = bits;
}

bool params_ok(const mhap_select_params& p) { return p.best_n >= 1 && p.min_span >= 0; }

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_select_session : ReadTable {
  static constexpr const char* finish_name = "mhap_select_finish";
  static constexpr int unfinished_rc = MHAP_E_STATE;
  SParams P{};
  bool finished = false;
  int grid = 1;   // the workgroups of select_kernel
  DevBuf entries, keys, count, offsets, cursor, rows, work, n_work, counts, views;   // counts: MHAP_SELECT_COUNTS x uint64
  void release() {
    release_table();
    for (DevBuf* b : {&entries, &keys, &count, &offsets, &cursor, &rows, &work, &n_work, &counts, &views}) b->release();
  }
};

extern "C" void mhap_select_default_params(mhap_select_params* p) {
  if (!p) return;
  p->best_n = 40; p->min_span = 500; p->min_identity = 0.0;
}

extern "C" int mhap_select_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_select_params* params,
                                 mhap_select_session** session) {
  return session_begin("mhap_select_begin", h, read_ids, lengths, n_reads, params, mhap_select_default_params, params_ok,
                       "best_n must be >= 1 and min_span >= 0", session,
                       [&](mhap_select_session& s, const mhap_select_params& p, const HandleView& v) {
    s.P = SParams{p.best_n, p.min_span, p.min_identity};
    s.grid = std::max(1, v.num_cus) * 4;
    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1);
    Steps q{s.begin_table(v, h, read_ids, lengths, n_reads), v.stream};
    q.ensure(s.count, 4 * nr);
    q.ensure(s.offsets, 8 * (nr + 1));
    q.ensure(s.cursor, 4 * nr);
    q.ensure(s.rows, 16 * nr);
    q.ensure(s.work, 4 * nr);
    q.ensure(s.n_work, 4);
    q.ensure(s.counts, 8 * MHAP_SELECT_COUNTS);
    q.zero(s.counts, 8 * MHAP_SELECT_COUNTS);
    q.zero(s.count, 4 * nr);
    q.zero(s.offsets, 8 * (nr + 1));
    return q.e;
  });
}

extern "C" int mhap_select_add(mhap_select_session* s, const mhap_record* recs, int64_t n) {
  const char* who = "mhap_select_add";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (n > 0 && n > (int64_t)INT32_MAX - s->n_records) { *v.err = std::string(who) + ": more than 2^31 - 1 records in one session"; return MHAP_E_INVALID; }
  ReadTable::Pending p;
  const int rc = s->queue_add(v, who, recs, n, p);
  if (rc != MHAP_OK || !p.ev) return rc;
  const hipError_t e = s->entries.ensure(16 * (size_t)(s->n_records + n), true, v.stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(v.stream);   // (the upload reads p.host)
    (void)hipEventDestroy(p.ev);
    return hip_fail(v, who, "hipMalloc of the entries", e);
  }
  hipLaunchKernelGGL(entry_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, s->items.as<int4>(), n, s->n_reads, s->P,
                     s->entries.as<int4>() + s->n_records, s->count.as<int32_t>(), s->counts.as<u64>() + SC_ELIGIBLE);
  return s->commit_add(v, who, p, n);
}

extern "C" int mhap_select_finish(mhap_select_session* s, int64_t* counts) {
  const char* who = "mhap_select_finish";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (!counts) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  (void)hipSetDevice(v.device);
  s->finished = false;
  hipError_t e;
  u64* d_counts = s->counts.as<u64>();
  const size_t nr = (size_t)std::max<int64_t>(s->n_reads, 1);
  const int64_t n_slots = 2 * s->n_records;
  if ((e = s->keys.ensure(4 * (size_t)std::max<int64_t>(n_slots, 1))) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "hipMalloc of the keys", e); }
  // the counts of this finish; the eligible records are summed over the adds and stay
  if ((e = hipMemsetAsync(d_counts, 0, 8 * SC_ELIGIBLE, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if ((e = hipMemsetAsync(s->cursor.p, 0, 4 * nr, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if ((e = hipMemsetAsync(s->n_work.p, 0, 4, v.stream)) != hipSuccess) return hip_fail(v, who, "memset", e);
  if (s->n_reads > 0) {
    hipLaunchKernelGGL(scan_kernel<int32_t>, dim3(1), dim3(1024), 0, v.stream, s->count.as<int32_t>(), s->n_reads, s->offsets.as<int64_t>());
    if (n_slots > 0)
      hipLaunchKernelGGL(scatter_kernel, dim3(blocks256(n_slots)), dim3(256), 0, v.stream, s->entries.as<int2>(), n_slots, s->n_reads,
                         s->offsets.as<int64_t>(), s->cursor.as<int32_t>(), s->keys.as<uint32_t>());
    hipLaunchKernelGGL(rows_kernel, dim3(blocks256(s->n_reads)), dim3(256), 0, v.stream, s->count.as<int32_t>(), s->n_reads,
                       s->offsets.as<int64_t>(), s->keys.as<uint32_t>(), s->P.best_n, s->rows.as<int32_t>(), s->work.as<int32_t>(),
                       s->n_work.as<int32_t>(), d_counts);
    const unsigned grid = (unsigned)std::min<int64_t>(s->grid, s->n_reads);
    hipLaunchKernelGGL(select_kernel, dim3(grid), dim3(SEL_T), 0, v.stream, s->keys.as<uint32_t>(), s->offsets.as<int64_t>(),
                       s->work.as<int32_t>(), s->n_work.as<int32_t>(), s->P.best_n, s->rows.as<int32_t>(), d_counts);
  }
  if ((e = hipGetLastError()) != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, "launch", e); }
  u64 hc[MHAP_SELECT_COUNTS];
  e = hipMemcpyAsync(hc, d_counts, sizeof hc, hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);   // the one wait of a finish
  if (e != hipSuccess) return hip_fail(v, who, "download", e);
  if (es != hipSuccess) return hip_fail(v, who, "kernel", es);
  s->reap(true);   // the stream is empty: every upload has been read
  for (int k = 0; k < MHAP_SELECT_COUNTS; k++) counts[k] = (int64_t)hc[k];
  counts[SC_READS] = s->n_reads;
  s->finished = true;
  return MHAP_OK;
}

extern "C" int mhap_select_copy(mhap_select_session* s, int32_t* rows) {
  const char* who = "mhap_select_copy";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  const int rc = check_finished(s, v, who);
  if (rc != MHAP_OK || s->n_reads == 0) return rc;
  if (!rows) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return s->download(who, rows, s->rows.p, 16 * (size_t)s->n_reads);
}

extern "C" int mhap_select_apply(mhap_select_session* s, const mhap_record* in, int64_t n, uint8_t* views) {
  const char* who = "mhap_select_apply";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  std::vector<GItem> items;
  const int rc = apply_begin(s, v, who, in, n, views != nullptr, items, s->views, (size_t)n, "hipMalloc of the views");
  if (rc != MHAP_OK || n == 0) return rc;
  hipLaunchKernelGGL(view_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, s->items.as<int4>(), n, s->n_reads, s->P, s->rows.as<int32_t>(),
                     s->views.as<uint8_t>());
  return apply_end(v, who, views, s->views, (size_t)n);   // (a view byte is what the kernel wrote: nothing to unpack)
}

extern "C" int mhap_select_judge_record(const mhap_record* in, const mhap_select_params* params, uint32_t* keys) {
  if (!in || !keys) return -1;
  mhap_select_params p;
  mhap_select_default_params(&p);
  if (params) p = *params;
  if (!params_ok(p)) return -1;
  keys[0] = keys[1] = 0;
  if (!select_eligible(in->from_id, in->to_id, in->score, p.min_identity)) return 0;
  if (in->a1 < 0 || in->a2 < in->a1 || in->a2 >= in->alen || in->b1 < 0 || in->b2 < in->b1 || in->b2 >= in->blen) return -1;
  keys[0] = select_key(in->a1, in->a2, in->score, p.min_span);
  keys[1] = select_key(in->b1, in->b2, in->score, p.min_span);
  return 1;
}

extern "C" void mhap_select_free(mhap_select_session* s) { session_free(s); }
