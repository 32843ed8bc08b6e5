// read_table.hpp — the host side that every session over a table of reads begins with, written once and without a kernel: the
// table (ids, lengths, the lengths on the device), a record's two reads looked up and checked against it, the record packed as the
// 32-byte item the kernels read, the uploads an add has queued, and the begin / apply / free that "read trimming"
// (trim_kernels.hip), "repeat marking" (repeat_kernels.hip) and "overlap selection" (select_kernels.hip) share.  The string graph's
// session (graph_session.hpp; its calls are in graph_kernels.hip and unitig_kernels.hip) begins, frees and queues its steps through
// the same skeleton, and the unitig consensus looks its reads up through that session; the read
// correction (correct_kernels.hip) and the variant sites (variant_kernels.hip), which keep the bases and a vote table, sit on
// vote_table.hpp's VoteTable and share the lookup.
//
// Two checks of a record, kept apart: find_record_reads (both reads are among the reads, and with the lengths the record gives)
// is every session's; range_ok (the aligned ends lie inside the reads) is applied by the trimming, the repeat marking and the
// selection only, whose kernels index a read by those ends.  The graph and the consensus take such a record.  A record that fails
// both is refused with the lookup's message.
#pragma once
#include <hip/hip_runtime.h>

#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

#include "graph_class.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

typedef unsigned long long u64;

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

// Record q's two reads in a table of ids (by_id: id -> position) and lengths: their positions, or false with the message in err.
template <class Map, class Index>
bool find_record_reads(const Map& by_id, const int32_t* lengths, const char* who, int64_t q, const mhap_record& r, Index (&idx)[2], std::string& err) {
  const int64_t rid[2] = {r.from_id, r.to_id};
  const int32_t lens[2] = {r.alen, r.blen};
  for (int f = 0; f < 2; f++) {
    const auto it = by_id.find(rid[f]);
    if (it == by_id.end()) {
      err = std::string(who) + ": record " + std::to_string(q) + " names read " + std::to_string(rid[f]) + ", which is not among the reads";
      return false;
    }
    idx[f] = it->second;
    if (lengths[idx[f]] != lens[f]) {
      err = std::string(who) + ": record " + std::to_string(q) + " gives read " + std::to_string(rid[f]) + " the length " + std::to_string(lens[f]) +
            ", the reads say " + std::to_string(lengths[idx[f]]);
      return false;
    }
  }
  return true;
}

// the aligned ends of record q lie inside its reads (a record without an alignment, score 0, has none to check)
inline bool range_ok(const char* who, int64_t q, const mhap_record& r, std::string& err) {
  const int64_t rid[2] = {r.from_id, r.to_id};
  const int32_t lens[2] = {r.alen, r.blen}, x1[2] = {r.a1, r.b1}, x2[2] = {r.a2, r.b2};
  for (int f = 0; f < 2; f++)
    if (r.score != 0.0 && (x1[f] < 0 || x2[f] < x1[f] || x2[f] >= lens[f])) {
      err = std::string(who) + ": record " + std::to_string(q) + " aligns " + std::to_string(x1[f]) + " .. " + std::to_string(x2[f]) + " of read " +
            std::to_string(rid[f]) + ", which has " + std::to_string(lens[f]) + " bases";
      return false;
    }
  return true;
}

inline GItem pack_item(const int32_t (&idx)[2], const mhap_record& r) {
  return GItem{idx[0], 2 * idx[1] + (r.to_rc != 0 ? 1 : 0), r.a1, r.a2, r.b1, r.b2, r.score};
}

struct ReadTable {
  mhap_handle* h = nullptr;
  int64_t n_reads = 0, n_records = 0;
  std::vector<int64_t> ids;
  std::vector<int32_t> lengths;
  std::unordered_map<int64_t, int32_t> by_id;
  struct Pending { std::vector<GItem> host; hipEvent_t ev = nullptr; };   // packed records an upload may still be reading
  std::deque<Pending> pending;
  DevBuf d_lengths, items;
  static constexpr bool any_length = false;   // a session that sets it takes every length >= 0 (the graph: nothing indexes a base)

  void reap(bool all) {
    while (!pending.empty() && (all || hipEventQuery(pending.front().ev) == hipSuccess)) {
      (void)hipEventDestroy(pending.front().ev);
      pending.pop_front();
    }
    (void)hipGetLastError();   // (an event that has not passed is no error of the call that looked)
  }
  void release_table() {
    for (DevBuf* b : {&d_lengths, &items}) b->release();
  }

  // the arguments every begin refuses; false with the handle's message set
  static bool table_ok(const HandleView& v, const char* who, const void* session, const int64_t* read_ids, const int32_t* lens, int64_t n,
                       bool any_len = false) {
    if (!session || n < 0 || (n > 0 && (!read_ids || !lens))) { *v.err = std::string(who) + ": null or negative argument"; return false; }
    if (n >= ((int64_t)1 << 30)) { *v.err = std::string(who) + ": 2^30 reads or more"; return false; }
    for (int64_t i = 0; i < n; i++)
      if (lens[i] < 0 || (!any_len && lens[i] > INT32_MAX - 8)) {
        *v.err = std::string(who) + ": read " + std::to_string(i) + (any_len ? " has a negative length" : " has a negative length or one above 2^31 - 9");
        return false;
      }
    return true;
  }

  // the table on the host and the lengths on the device; queued on the handle's stream, not waited for
  hipError_t begin_table(const HandleView& v, mhap_handle* handle, const int64_t* read_ids, const int32_t* lens, int64_t n) {
    h = handle; n_reads = n;
    ids.assign(read_ids, read_ids + n);
    lengths.assign(lens, lens + n);
    by_id.reserve((size_t)n * 2);
    for (int64_t i = 0; i < n; i++) by_id.emplace(read_ids[i], (int32_t)i);   // (the first read of an id wins, as in mhap_realign_plan)
    hipError_t e = d_lengths.ensure(4 * (size_t)std::max<int64_t>(n, 1));
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(d_lengths.p, lengths.data(), 4 * (size_t)n, hipMemcpyHostToDevice, v.stream);
    return e;
  }

  bool find_reads(const char* who, int64_t q, const mhap_record& r, int32_t (&idx)[2], std::string& err) const {
    return find_record_reads(by_id, lengths.data(), who, q, r, idx, err);
  }
  // the records of a call as items for the sessions whose kernels index a read by a record's aligned ends: record by record, the
  // lookup and then range_ok (`ranges` false: the lookup alone, for the graph and the consensus, where a record's aligned ends
  // index nothing); a refused record leaves its message in err
  bool pack_records(const char* who, const mhap_record* recs, int64_t n, std::vector<GItem>& out, std::string& err, bool ranges = true) const {
    out.resize((size_t)n);
    for (int64_t q = 0; q < n; q++) {
      int32_t idx[2];
      if (!find_reads(who, q, recs[q], idx, err) || (ranges && !range_ok(who, q, recs[q], err))) return false;
      out[(size_t)q] = pack_item(idx, recs[q]);
    }
    return true;
  }

  // The front of an add: the records are checked (a refused call queues nothing), packed into p and their upload into `items` is
  // queued.  MHAP_OK with p.ev == nullptr: n == 0, nothing to do.  The caller launches its kernel on the stream and calls commit_add.
  int queue_add(const HandleView& v, const char* who, const mhap_record* recs, int64_t n, Pending& p) {
    if (n < 0 || (n > 0 && !recs)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
    if (n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records in one call"; return MHAP_E_INVALID; }
    reap(false);
    if (n == 0) return MHAP_OK;
    if (!pack_records(who, recs, n, p.host, *v.err)) return MHAP_E_INVALID;
    (void)hipSetDevice(v.device);
    hipError_t e = items.ensure(sizeof(GItem) * (size_t)n);   // (a larger buffer frees the old one, which waits for the device)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p.ev, hipEventDisableTiming);
    if (e != hipSuccess) { p.ev = nullptr; return hip_fail(v, who, "hipMalloc of the records", e); }
    e = hipMemcpyAsync(items.p, p.host.data(), sizeof(GItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
    if (e != hipSuccess) {   // nothing was queued behind the upload: nothing of this call stays
      (void)hipStreamSynchronize(v.stream);
      (void)hipEventDestroy(p.ev);
      p.ev = nullptr;
      return hip_fail(v, who, "upload", e);
    }
    return MHAP_OK;
  }
  // The back of an add, behind the caller's launch: the launch's error is looked at, the event recorded and the records counted.
  int commit_add(const HandleView& v, const char* who, Pending& p, int64_t n) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(p.ev, v.stream);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(v.stream);
      (void)hipEventDestroy(p.ev);
      return hip_fail(v, who, "launch", e);
    }
    pending.push_back(std::move(p));
    n_records += n;
    return MHAP_OK;
  }

  // the packed records of an apply queued into `items`, behind everything an add may still read; `packed` must live until the
  // caller has waited for the stream.  False with rc set.
  bool upload_for_apply(const HandleView& v, const char* who, const mhap_record* in, int64_t n, std::vector<GItem>& packed, int& rc) {
    if (!pack_records(who, in, n, packed, *v.err)) { rc = MHAP_E_INVALID; return false; }
    (void)hipSetDevice(v.device);
    hipError_t e;
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) { rc = hip_fail(v, who, "the stream", e); return false; }   // (an add may still read the items' buffer)
    reap(true);
    if ((e = items.ensure(sizeof(GItem) * (size_t)n)) != hipSuccess) { rc = hip_fail(v, who, "hipMalloc of the records", e); return false; }
    if ((e = hipMemcpyAsync(items.p, packed.data(), sizeof(GItem) * (size_t)n, hipMemcpyHostToDevice, v.stream)) != hipSuccess) {
      rc = hip_fail(v, who, "upload", e);
      return false;
    }
    return true;
  }

  int download(const char* who, void* dst, const void* src, size_t bytes) {
    HandleView v = handle_view(h);
    (void)hipSetDevice(v.device);
    hipError_t e;
    if ((e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
    return MHAP_OK;
  }
};

// ---- the calls of a session S that the trimming, the repeat marking and the selection share -----------------------------------------
// S sits on ReadTable and has: `finished` (a finish has completed), `finish_name` and `unfinished_rc` (the entry point a call before
// it is told of, and the code it gets), and release().

struct Copy { void* dst; const void* src; size_t bytes; };   // one download

// The steps a call queues: nothing runs once a step has failed, and `what` keeps the kind of step that did, as hip_fail names it.
// The caller looks at ok() before it launches kernels, which are no steps; launched() looks at them afterwards.
struct Steps {
  hipError_t e;
  hipStream_t stream;
  const char* what = "";
  bool ok() const { return e == hipSuccess; }
  int fail(const HandleView& v, const char* who) const { return hip_fail(v, who, what, e); }
  void step(const char* w, hipError_t r) { e = r; if (r != hipSuccess) what = w; }   // (behind an ok())
  void ensure(DevBuf& b, size_t bytes, const char* w = "hipMalloc") { if (ok()) step(w, b.ensure(bytes)); }
  template <class T> void ensure(Dev<T>& b, size_t n, const char* w = "hipMalloc") { ensure(b.b, n * sizeof(T), w); }
  template <class... B> void ensure_all(const char* w, size_t n, B&... b) { (ensure(b, n, w), ...); }   // n elements each
  void fill(void* p, int byte, size_t bytes) { if (ok()) step("memset", hipMemsetAsync(p, byte, bytes, stream)); }
  void zero(DevBuf& b, size_t bytes) { fill(b.p, 0, bytes); }
  template <class T> void zero(Dev<T>& b, size_t n) { fill(b.b.p, 0, n * sizeof(T)); }
  void upload(void* dst, const void* src, size_t bytes) { if (ok()) step("upload", hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream)); }
  void launched() { if (ok()) step("launch", hipGetLastError()); }
  // these few values, and the one wait for them
  void fetch(std::initializer_list<Copy> cs) {
    for (const Copy& c : cs) if (ok()) step("download", hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream));
    if (ok()) step("kernel", hipStreamSynchronize(stream));
  }
};

// begin: the arguments (the lengths by S::any_length) and the parameters checked (`rule`: what a refused set of parameters is told), the session made, `setup`
// fills its fields from the parameters and queues the table and the session's own buffers (hipError_t setup(S&, const Params&,
// const HandleView&)), and the one wait.
template <class S, class Params, class Setup>
int session_begin(const char* who, mhap_handle* h, const int64_t* read_ids, const int32_t* lengths, int64_t n_reads, const Params* params,
                  void (*defaults)(Params*), bool (*ok)(const Params&), const char* rule, S** session, Setup setup) {
  if (session) *session = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!ReadTable::table_ok(v, who, session, read_ids, lengths, n_reads, S::any_length)) return MHAP_E_INVALID;
  Params p;
  defaults(&p);
  if (params) p = *params;
  if (!ok(p)) { *v.err = std::string(who) + ": " + rule; return MHAP_E_INVALID; }
  S* s = new S();
  (void)hipSetDevice(v.device);
  hipError_t e = setup(*s, p, v);
  if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
  if (e != hipSuccess) {
    s->release();
    delete s;
    return hip_fail(v, who, "the table of reads", e);
  }
  *session = s;
  return MHAP_OK;
}

// a call that reads what a finish made
template <class S>
int check_finished(const S* s, const HandleView& v, const char* who) {
  if (s->finished) return MHAP_OK;
  *v.err = std::string(who) + ": no " + S::finish_name + " has completed";
  return S::unfinished_rc;
}

// apply, around the caller's kernel.  apply_begin: the state and the arguments checked (args_ok: the caller's pointers), the records
// checked, packed into `packed` and queued into s->items, and `out` made large enough (out_what: what hip_fail names it).  Not
// MHAP_OK, or n == 0: the caller returns the code.  Otherwise it launches on the stream and calls apply_end, which looks at the
// launch, downloads `bytes` of `out` into dst and waits; `packed` lives until then.  A failure with work queued waits for the
// stream before it returns: the upload reads `packed`.
template <class S>
int apply_begin(S* s, const HandleView& v, const char* who, const mhap_record* in, int64_t n, bool args_ok, std::vector<GItem>& packed, DevBuf& out,
                size_t out_bytes, const char* out_what) {
  int rc = check_finished(s, v, who);
  if (rc != MHAP_OK) return rc;
  if (n < 0 || (n > 0 && (!in || !args_ok))) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records in one call"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  if (!s->upload_for_apply(v, who, in, n, packed, rc)) return rc;
  const hipError_t e = out.ensure(out_bytes);
  if (e != hipSuccess) { (void)hipStreamSynchronize(v.stream); return hip_fail(v, who, out_what, e); }
  return MHAP_OK;
}
inline int apply_end(const HandleView& v, const char* who, void* dst, const DevBuf& out, size_t bytes) {
  Steps q{hipSuccess, v.stream};
  q.launched();
  q.fetch({{dst, out.p, bytes}});
  if (!q.ok()) { (void)hipStreamSynchronize(v.stream); return q.fail(v, who); }
  return MHAP_OK;
}

template <class S>
void session_free(S* s) {
  if (!s) return;
  HandleView v = handle_view(s->h);
  (void)hipSetDevice(v.device);
  (void)hipStreamSynchronize(v.stream);
  s->reap(true);
  s->release();
  delete s;
}

}  // namespace
}  // namespace mhap
