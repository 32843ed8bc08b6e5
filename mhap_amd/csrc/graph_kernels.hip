// graph_kernels.hip — the string graph of the realigned overlaps (mhap_graph_begin / _add / _finish / _info / _copy_arcs /
// _copy_classes / _copy_read_flags / _free) and the GFA link lines.  Its unitigs, their spelling and the cleaning of the graph are
// unitig_kernels.hip's, over the session both units share (graph_session.hpp).  The contract — the class of a record, the arcs of a
// dovetail, contained reads, the arc list, the reduction and the final arcs — is the prose of include/mhap_hip.h ("string graph");
// tests/string_graph_ref.py restates it.
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

#include "device_common.hpp"
#include "graph_session.hpp"

namespace mhap {
namespace {

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

bool params_ok(const mhap_graph_params& p) {
  return p.max_hang >= 0 && p.int_frac_permille >= 0 && p.int_frac_permille <= 1000 && p.min_ovlp >= 0 && p.fuzz >= 0;
}

}  // namespace
}  // namespace mhap

using namespace mhap;

extern "C" void mhap_graph_default_params(mhap_graph_params* p) {
  if (!p) return;
  p->max_hang = 1000; p->int_frac_permille = 800; p->min_ovlp = 2000; p->fuzz = 1000; p->min_identity = 0.0;
}

extern "C" int mhap_graph_begin(mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const mhap_graph_params* params,
                                mhap_graph_session** session) {
  return session_begin("mhap_graph_begin", h, read_ids, lengths, n_reads, params, mhap_graph_default_params, params_ok,
                       "max_hang, min_ovlp and fuzz must be >= 0 and int_frac_permille in [0, 1000]", session,
                       [&](mhap_graph_session& s, const mhap_graph_params& p, const HandleView& v) {
    s.P = GParams{p.max_hang, p.int_frac_permille, p.min_ovlp, p.fuzz, p.min_identity};
    const size_t nr = (size_t)std::max<int64_t>(n_reads, 1);
    Steps q{s.begin_table(v, h, read_ids, lengths, n_reads), v.stream};
    q.ensure(s.ad.contained, nr);
    q.ensure(s.ad.counts, MHAP_GRAPH_COUNTS);
    q.zero(s.ad.contained, nr);
    q.zero(s.ad.counts, MHAP_GRAPH_COUNTS);
    return q.e;
  });
}

// (nothing here is shared with ReadTable::queue_add / commit_add: a chunk of the add's own that stays, and other messages)
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
  hipError_t e = c.items.ensure(2 * (size_t)n);
  if (e == hipSuccess) e = c.cls.ensure((size_t)n);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&p.ev, hipEventDisableTiming);
  if (e != hipSuccess) { c.release(); return hip_fail(v, who, "hipMalloc of the records", e); }
  e = hipMemcpyAsync(c.items.get(), p.host.data(), sizeof(GItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
  if (e == hipSuccess) {   // (the kernel reads an item as two int4 and writes its two arcs over them)
    hipLaunchKernelGGL(classify_kernel, dim3(blocks256(n)), dim3(256), 0, v.stream, (int4*)c.items.get(), n, (int32_t)s->n_records,
                       (const int32_t*)s->d_lengths.p, s->P, c.cls.get(), s->ad.contained.get(), s->ad.counts.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipEventRecord(p.ev, v.stream);
  if (e != hipSuccess) {   // nothing of this call stays; the upload may be in flight, so it is waited for before its source goes
    (void)hipStreamSynchronize(v.stream);
    (void)hipEventDestroy(p.ev);
    c.release();
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
  if (!counts) return s->null_arg(who);
  (void)hipSetDevice(v.device);
  s->n_arcs = s->n_unitigs = -1;
  s->unitig_gen++;
  s->cleaned = false;   // (a clean starts from zeroed bytes: nothing to zero here)
  const int64_t nv = 2 * s->n_reads;
  GraphArcs& a = s->arc;
  const uint32_t* contained = s->ad.contained.get();
  const int32_t* lengths = (const int32_t*)s->d_lengths.p;
  u64* d_counts = s->ad.counts.get();
  const dim3 b256(256), wave(64), one(1), b1024(1024);
  Steps q{hipSuccess, v.stream};
  // the counts of this finish start from the classes the adds have summed
  q.fill(d_counts + GC_CONTAINED, 0, 8 * (MHAP_GRAPH_COUNTS - GC_CONTAINED));
  q.ensure_all("hipMalloc of the vertex tables", (size_t)(nv + 1), a.deg, a.fill, a.start, a.fstart);
  q.zero(a.deg, (size_t)(nv + 1)); q.zero(a.fill, (size_t)(nv + 1));
  if (!q.ok()) return q.fail(v, who);
  if (s->n_reads > 0) hipLaunchKernelGGL(flags_kernel, dim3(blocks256(s->n_reads)), b256, 0, v.stream, contained, s->n_reads, d_counts);
  for (auto& c : s->chunks)
    hipLaunchKernelGGL(count_kernel, dim3(blocks256(2 * c.n)), b256, 0, v.stream, c.items.get(), 2 * c.n, contained, a.deg.get());
  hipLaunchKernelGGL(scan_kernel<int32_t>, one, b1024, 0, v.stream, a.deg.get(), nv, a.start.get());
  q.launched();
  int64_t n_live = 0, n_arcs = 0;
  q.fetch({{&n_live, a.start.get() + nv, 8}});
  if (!q.ok()) return q.fail(v, who);
  s->reap(true);   // the stream is empty: every upload has been read
  if (n_live > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 arcs"; return MHAP_E_INVALID; }
  q.ensure_all("hipMalloc of the arcs", (size_t)std::max<int64_t>(n_live, 1), a.tmp, a.keep);
  if (!q.ok()) return q.fail(v, who);
  for (auto& c : s->chunks)
    hipLaunchKernelGGL(scatter_kernel, dim3(blocks256(2 * c.n)), b256, 0, v.stream, c.items.get(), 2 * c.n, contained, a.start.get(), a.fill.get(),
                       a.tmp.get());
  if (nv > 0) hipLaunchKernelGGL(dedup_kernel, dim3((unsigned)nv), wave, 0, v.stream, a.tmp.get(), a.start.get(), a.keep.get(),
                                 a.deg.get());   // (deg has been scanned: it now takes the kept arcs per u)
  hipLaunchKernelGGL(scan_kernel<int32_t>, one, b1024, 0, v.stream, a.deg.get(), nv, a.fstart.get());
  q.launched();
  q.fetch({{&n_arcs, a.fstart.get() + nv, 8}});
  const size_t na = (size_t)std::max<int64_t>(n_arcs, 1);
  q.ensure_all("hipMalloc of the arc list", na, a.U, a.V, a.LEN, a.Q, a.bt_v, a.bt_pos, a.mark);
  q.ensure(a.rows, 7 * na, "hipMalloc of the arc list");
  q.zero(a.mark, na);
  if (!q.ok()) return q.fail(v, who);
  if (n_arcs > 0) {
    hipLaunchKernelGGL(place_kernel, dim3((unsigned)nv), wave, 0, v.stream, a.tmp.get(), a.keep.get(), a.start.get(), a.fstart.get(), a.U.get(),
                       a.V.get(), a.LEN.get(), a.Q.get(), a.bt_v.get(), a.bt_pos.get());
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)nv), wave, 0, v.stream, a.fstart.get(), a.V.get(), a.LEN.get(), a.bt_v.get(), a.bt_pos.get(),
                       s->P.fuzz, a.mark.get());
    hipLaunchKernelGGL(finish_kernel, dim3(blocks256(n_arcs)), b256, 0, v.stream, n_arcs, a.fstart.get(), a.U.get(), a.V.get(), a.LEN.get(),
                       a.Q.get(), a.bt_v.get(), a.bt_pos.get(), a.mark.get(), lengths, a.rows.get(), d_counts);
    q.launched();
  }
  u64 hc[MHAP_GRAPH_COUNTS];
  q.fetch({{hc, d_counts, sizeof hc}});
  if (!q.ok()) return q.fail(v, who);
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
  if (!s) return MHAP_E_INVALID;
  return s->copy_out("mhap_graph_copy_arcs", NEED_ARCS, s->n_arcs, !rows, {{rows, s->arc.rows.get(), 28 * (size_t)s->n_arcs}});
}

extern "C" int mhap_graph_copy_classes(mhap_graph_session* s, uint8_t* classes) {   // (needs no finish: an add has classed its records)
  if (!s) return MHAP_E_INVALID;
  std::vector<Copy> copies;
  int64_t at = 0;
  if (classes) for (auto& c : s->chunks) { copies.push_back(Copy{classes + at, c.cls.get(), (size_t)c.n}); at += c.n; }
  return s->copy_out("mhap_graph_copy_classes", NEED_NOTHING, s->n_records, !classes, copies);
}

extern "C" int mhap_graph_copy_read_flags(mhap_graph_session* s, uint8_t* flags) {
  if (!s) return MHAP_E_INVALID;
  std::vector<uint32_t> w((size_t)s->n_reads);
  const int rc = s->copy_out("mhap_graph_copy_read_flags", NEED_NOTHING, s->n_reads, !flags, {{w.data(), s->ad.contained.get(), 4 * w.size()}});
  if (rc != MHAP_OK) return rc;
  for (int64_t r = 0; r < s->n_reads; r++) flags[r] = w[(size_t)r] ? 1 : 0;
  return MHAP_OK;
}

extern "C" void mhap_graph_free(mhap_graph_session* s) { session_free(s); }

// what the unitig consensus (consensus_kernels.hip) reads of a graph session besides its public calls
mhap::GraphView mhap::graph_view(const mhap_graph_session* s) {
  return GraphView{s->h, s->P, s->n_reads, s->ids.data(), s->lengths.data(), s->unitig_gen, s->n_unitigs};
}
bool mhap::graph_pack_records(const mhap_graph_session* s, const char* who, const mhap_record* recs, int64_t n, std::vector<GItem>& out, std::string& err) {
  return s->pack_records(who, recs, n, out, err, false);
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
