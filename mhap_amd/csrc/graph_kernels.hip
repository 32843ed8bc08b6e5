// graph_kernels.hip — the string graph of the realigned overlaps (mhap_graph_begin / _add / _finish / _copy_* / _free) and the GFA link
// line.  The contract — the class of a record, the arcs of a dovetail, contained reads, the arc list, the reduction and the final
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
#include <unordered_map>
#include <vector>

#include "mhap_internal.hpp"

namespace mhap {
namespace {

enum { G_NONE = 0, G_INTERNAL, G_A_CONTAINED, G_B_CONTAINED, G_SHORT, G_DOVETAIL, G_CLASSES };
// counts: records, the six classes, contained reads, arcs, reduced, final
enum { GC_RECORDS = 0, GC_CLASS0 = 1, GC_CONTAINED = 7, GC_ARCS = 8, GC_REDUCED = 9, GC_FINAL = 10 };

// a record as it goes up: the two reads' positions in the table (brc = 2 B + to_rc), the aligned ends, the identity
struct GItem { int32_t a, brc, a1, a2, b1, b2; double score; };
struct GArc { int32_t u, v, len, q; };   // two of them over a GItem; u = -1: no arc
static_assert(sizeof(GItem) == 32 && sizeof(GArc) == 16, "an item is two arcs");

struct GParams { int32_t max_hang, permille, min_ovlp, fuzz; double min_identity; };

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
    if (A == B || score == 0.0 || score < P.min_identity) c = G_NONE;
    else {
      const int32_t qs = w0.z, qe = w0.w + 1, ql = lengths[A], tl = lengths[B];
      const int32_t ts = o ? tl - w1.y - 1 : w1.x, te = o ? tl - w1.x : w1.y + 1;
      const int32_t tl5 = ts, tl3 = tl - te, q3 = ql - qe;
      const int32_t ext5 = min(qs, tl5), ext3 = min(q3, tl3);
      const int64_t span = (int64_t)qe - qs, ext = (int64_t)ext5 + ext3;
      if (ext5 > P.max_hang || ext3 > P.max_hang || span * 1000 < (span + ext) * P.permille) c = G_INTERNAL;
      else if (qs <= tl5 && q3 <= tl3) { c = G_A_CONTAINED; atomicOr(contained + A, 1u); }
      else if (qs >= tl5 && q3 >= tl3) { c = G_B_CONTAINED; atomicOr(contained + B, 1u); }
      else if (span + ext < P.min_ovlp || (int64_t)te - ts + ext < P.min_ovlp) c = G_SHORT;
      else {
        c = G_DOVETAIL;
        const int32_t lab = q0 + (int32_t)q;
        if (qs > tl5) { e0 = GArc{2 * A, 2 * B + o, qs - tl5, lab}; e1 = GArc{2 * B + (1 - o), 2 * A + 1, tl3 - q3, lab}; }
        else { e0 = GArc{2 * B + o, 2 * A, tl5 - qs, lab}; e1 = GArc{2 * A + 1, 2 * B + (1 - o), q3 - tl3, lab}; }
      }
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

// start[0 .. n] = the exclusive prefix sums of deg[0 .. n): one workgroup, 1024 values at a time with a carry
__global__ __launch_bounds__(1024) void scan_kernel(const int32_t* __restrict__ deg, int64_t n, int64_t* __restrict__ start) {
  __shared__ int64_t wave_sum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t i0 = 0; i0 < n; i0 += 1024) {
    const int64_t i = i0 + tid;
    const int64_t x = i < n ? deg[i] : 0;
    int64_t incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t u = __shfl_up(incl, d);
      if (lane >= d) incl += u;
    }
    __syncthreads();   // wave_sum of the previous tile has been read
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int64_t before = 0, tile = 0;
    for (int u = 0; u < 16; u++) { if (u < wave) before += wave_sum[u]; tile += wave_sum[u]; }
    if (i < n) start[i] = carry + before + incl - x;
    carry += tile;
  }
  if (tid == 0) start[n] = carry;
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

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_graph_session {
  mhap_handle* h = nullptr;
  GParams P{};
  int64_t n_reads = 0, n_records = 0, n_arcs = -1;        // n_arcs < 0: no finish yet
  std::vector<int64_t> ids;
  std::vector<int32_t> lengths;
  std::unordered_map<int64_t, int32_t> by_id;
  struct Chunk { DevBuf items, cls; int64_t n = 0; };     // items: the add's records, then its arc slots
  std::deque<Chunk> chunks;
  struct Pending { std::vector<GItem> host; hipEvent_t ev = nullptr; };   // packed records an upload may still be reading
  std::deque<Pending> pending;
  DevBuf d_lengths, contained, counts;                    // counts: MHAP_GRAPH_COUNTS x uint64, the classes summed over the adds
  DevBuf deg, fill, start, fstart, tmp, keep, U, V, LEN, Q, bt_v, bt_pos, mark, rows;
  void reap(bool all) {
    while (!pending.empty() && (all || hipEventQuery(pending.front().ev) == hipSuccess)) {
      (void)hipEventDestroy(pending.front().ev);
      pending.pop_front();
    }
    (void)hipGetLastError();   // (an event that has not passed is no error of the call that looked)
  }
  void release() {
    for (auto& c : chunks) { c.items.release(); c.cls.release(); }
    chunks.clear();
    for (DevBuf* b : {&d_lengths, &contained, &counts, &deg, &fill, &start, &fstart, &tmp, &keep, &U, &V, &LEN, &Q, &bt_v, &bt_pos, &mark, &rows}) b->release();
  }
};

namespace {

int hip_fail(const HandleView& v, const char* who, const char* what, hipError_t e) {
  *v.err = std::string(who) + ": " + what + ": " + hipGetErrorString(e);
  return MHAP_E_HIP;
}

unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

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
  s->h = h; s->n_reads = n_reads;
  s->P = GParams{p.max_hang, p.int_frac_permille, p.min_ovlp, p.fuzz, p.min_identity};
  s->ids.assign(read_ids, read_ids + n_reads);
  s->lengths.assign(lengths, lengths + n_reads);
  s->by_id.reserve((size_t)n_reads * 2);
  for (int64_t i = 0; i < n_reads; i++) s->by_id.emplace(read_ids[i], (int32_t)i);   // (the first read of an id wins, as in mhap_realign_plan)
  (void)hipSetDevice(v.device);
  const size_t rb = 4 * (size_t)std::max<int64_t>(n_reads, 1);
  hipError_t e = s->d_lengths.ensure(rb);
  if (e == hipSuccess) e = s->contained.ensure(rb);
  if (e == hipSuccess) e = s->counts.ensure(8 * MHAP_GRAPH_COUNTS);
  if (e == hipSuccess && n_reads > 0) e = hipMemcpyAsync(s->d_lengths.p, s->lengths.data(), 4 * (size_t)n_reads, hipMemcpyHostToDevice, v.stream);
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
  std::vector<GItem> items((size_t)n);
  for (int64_t q = 0; q < n; q++) {
    const mhap_record& r = recs[q];
    int32_t idx[2];
    const int64_t ids[2] = {r.from_id, r.to_id};
    const int32_t lens[2] = {r.alen, r.blen};
    for (int f = 0; f < 2; f++) {
      const auto it = s->by_id.find(ids[f]);
      if (it == s->by_id.end()) {
        *v.err = std::string(who) + ": record " + std::to_string(q) + " names read " + std::to_string(ids[f]) + ", which is not among the reads";
        return MHAP_E_INVALID;
      }
      idx[f] = it->second;
      if (s->lengths[(size_t)idx[f]] != lens[f]) {
        *v.err = std::string(who) + ": record " + std::to_string(q) + " gives read " + std::to_string(ids[f]) + " the length " + std::to_string(lens[f]) +
                 ", the reads say " + std::to_string(s->lengths[(size_t)idx[f]]);
        return MHAP_E_INVALID;
      }
    }
    items[(size_t)q] = GItem{idx[0], 2 * idx[1] + (r.to_rc != 0 ? 1 : 0), r.a1, r.a2, r.b1, r.b2, r.score};
  }
  (void)hipSetDevice(v.device);
  mhap_graph_session::Chunk c;
  mhap_graph_session::Pending p;
  hipError_t e = c.items.ensure(sizeof(GItem) * (size_t)n);
  if (e == hipSuccess) e = c.cls.ensure((size_t)n);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p.ev, hipEventDisableTiming);
  if (e != hipSuccess) { c.items.release(); c.cls.release(); return hip_fail(v, who, "hipMalloc of the records", e); }
  p.host = std::move(items);
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
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, v.stream, s->deg.as<int32_t>(), nv, s->start.as<int64_t>());
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
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, v.stream, s->deg.as<int32_t>(), nv, s->fstart.as<int64_t>());
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
  return MHAP_OK;
}

extern "C" int mhap_graph_info(const mhap_graph_session* s, int64_t* n_reads, int64_t* n_records, int64_t* n_arcs) {
  if (!s) return MHAP_E_INVALID;
  if (n_reads) *n_reads = s->n_reads;
  if (n_records) *n_records = s->n_records;
  if (n_arcs) *n_arcs = s->n_arcs;
  return MHAP_OK;
}

namespace {

int download(mhap_graph_session* s, const char* who, void* dst, const void* src, size_t bytes) {
  HandleView v = handle_view(s->h);
  (void)hipSetDevice(v.device);
  hipError_t e;
  if ((e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  return MHAP_OK;
}

}  // namespace

extern "C" int mhap_graph_copy_arcs(mhap_graph_session* s, int32_t* rows) {
  const char* who = "mhap_graph_copy_arcs";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->n_arcs < 0) { *v.err = std::string(who) + ": no mhap_graph_finish has completed"; return MHAP_E_INVALID; }
  if (s->n_arcs == 0) return MHAP_OK;
  if (!rows) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  return download(s, who, rows, s->rows.p, 28 * (size_t)s->n_arcs);
}

extern "C" int mhap_graph_copy_classes(mhap_graph_session* s, uint8_t* classes) {
  const char* who = "mhap_graph_copy_classes";
  if (!s) return MHAP_E_INVALID;
  HandleView v = handle_view(s->h);
  if (s->n_records == 0) return MHAP_OK;
  if (!classes) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
  int64_t at = 0;
  for (auto& c : s->chunks) {
    const int rc = download(s, who, classes + at, c.cls.p, (size_t)c.n);
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
  const int rc = download(s, who, w.data(), s->contained.p, 4 * w.size());
  if (rc != MHAP_OK) return rc;
  for (int64_t r = 0; r < s->n_reads; r++) flags[r] = w[(size_t)r] ? 1 : 0;
  return MHAP_OK;
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

extern "C" int mhap_format_gfa_link(const int32_t* row7, const int64_t* read_ids, char* out, size_t cap) {
  if (!row7 || !read_ids || (!out && cap > 0)) return -1;
  return snprintf(out, cap, "L\t%lld\t%c\t%lld\t%c\t%dM", (long long)read_ids[row7[0] >> 1], (row7[0] & 1) ? '-' : '+',
                  (long long)read_ids[row7[1] >> 1], (row7[1] & 1) ? '-' : '+', row7[3]);
}
