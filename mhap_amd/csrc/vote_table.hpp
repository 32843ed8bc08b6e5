// vote_table.hpp — the host side of a pile-up vote table over reads, written once for the sessions that keep one: the read correction
// (correct_kernels.hip, 12 planes per position) and the variant sites (variant_kernels.hip, 3).  The reads' bytes, offsets, table
// positions, lengths, id map and per-target view counts; the checks and uploads of a begin; the records of an add turned into
// VoteItems under the cap on views, with the views of a refused call taken back; the items cast 2^20 at a time by the caller's
// launch; and a target's counters downloaded and unpacked, which the unitig consensus (a table of its own, one target per unitig)
// uses too.  The walk, the item and the kernels are vote_common.hpp's; ReadTable (read_table.hpp) is the table of the sessions
// that keep no bases.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "mhap_internal.hpp"
#include "read_table.hpp"
#include "vote_common.hpp"

namespace mhap {
namespace {

// What every call that takes records with their paths checks before it looks at a record; args_ok: the caller's own pointers.
inline int check_call(const HandleView& v, const char* who, const mhap_record* recs, int64_t n, const mhap_align_paths* paths, bool args_ok) {
  if (n < 0 || !paths || !args_ok || (n > 0 && !recs)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if ((int64_t)paths->offsets.size() - 1 != n) {
    *v.err = std::string(who) + ": the paths are those of " + std::to_string((int64_t)paths->offsets.size() - 1) + " records, not of " + std::to_string(n);
    return MHAP_E_INVALID;
  }
  return MHAP_OK;
}

// `len` positions of `words` planes each, from word `first_word` of a device table, as 2 * words counters per position
inline int copy_votes(const HandleView& v, const char* who, const uint32_t* table, int64_t first_word, int64_t len, int words, uint16_t* counters) {
  (void)hipSetDevice(v.device);
  std::vector<uint32_t> w((size_t)len * words);
  hipError_t e;
  if ((e = hipMemcpyAsync(w.data(), table + first_word, w.size() * 4, hipMemcpyDeviceToHost, v.stream)) != hipSuccess ||
      (e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
  for (int64_t t = 0; t < len; t++)
    for (int p = 0; p < words; p++) {
      const uint32_t x = w[(size_t)(p * len + t)];
      counters[2 * words * t + 2 * p] = (uint16_t)(x & 0xFFFFu);
      counters[2 * words * t + 2 * p + 1] = (uint16_t)(x >> 16);
    }
  return MHAP_OK;
}

struct VoteTable {
  mhap_handle* h = nullptr;
  int words = 0;                                        // planes per position
  int64_t n_reads = 0, n_bases = 0, n_pos = 0;          // n_pos: bases of the reads = positions of the table
  std::vector<int64_t> offsets, pos;                    // read r: its bytes in the bases, its first table position
  std::vector<int32_t> lengths;
  std::unordered_map<int64_t, int64_t> by_id;
  std::vector<uint32_t> views;                          // accepted views per target
  int64_t skipped = 0;                                  // views refused a place under the cap
  DevBuf bases, table, read_off, read_pos, read_len, items, ops;
  void release_table() {
    for (DevBuf* b : {&bases, &table, &read_off, &read_pos, &read_len, &items, &ops}) b->release();
  }

  // the two refusals every begin starts with (a session's own come between them or behind); false with the handle's message set
  static bool args_ok(const HandleView& v, const char* who, const void* session, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids,
                      const int64_t* offsets, const int32_t* lengths, int64_t n_reads) {
    if (session && n_bases >= 0 && n_reads >= 0 && (n_bases == 0 || bases) && (n_reads == 0 || (read_ids && offsets && lengths))) return true;
    *v.err = std::string(who) + ": null or negative argument";
    return false;
  }
  static bool reads_inside(const HandleView& v, const char* who, int64_t n_bases, const int64_t* offsets, const int32_t* lengths, int64_t n_reads) {
    for (int64_t i = 0; i < n_reads; i++)
      if (offsets[i] < 0 || lengths[i] < 0 || offsets[i] > n_bases - lengths[i]) {
        *v.err = std::string(who) + ": read " + std::to_string(i) + " lies outside the " + std::to_string(n_bases) + " bases";
        return false;
      }
    return true;
  }

  // One upload of a begin's queue: nothing runs once a step has failed (e).
  static void upload(const HandleView& v, hipError_t& e, DevBuf& b, const void* src, size_t bytes) {
    if (e == hipSuccess) e = b.ensure(std::max<size_t>(bytes, 1));
    if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, v.stream);
  }

  // the table on the host, the reads on the device and the zeroed planes; queued on the handle's stream, not waited for
  hipError_t begin_table(const HandleView& v, mhap_handle* handle, int n_words, const uint8_t* b, int64_t nb, const int64_t* read_ids,
                         const int64_t* offs, const int32_t* lens, int64_t n) {
    h = handle; words = n_words; n_reads = n; n_bases = nb;
    offsets.assign(offs, offs + n);
    lengths.assign(lens, lens + n);
    pos.resize((size_t)n);
    views.assign((size_t)n, 0u);
    by_id.reserve((size_t)n * 2);
    for (int64_t i = 0; i < n; i++) {
      by_id.emplace(read_ids[i], i);   // (the first read of an id wins, as in mhap_realign_plan)
      pos[(size_t)i] = n_pos;
      n_pos += lens[i];
    }
    hipError_t e = hipSuccess;
    const size_t table_bytes = (size_t)std::max<int64_t>(n_pos, 1) * words * 4;
    upload(v, e, bases, b, (size_t)nb);
    upload(v, e, read_off, offsets.data(), 8 * (size_t)n);
    upload(v, e, read_pos, pos.data(), 8 * (size_t)n);
    upload(v, e, read_len, lengths.data(), 4 * (size_t)n);
    if (e == hipSuccess) e = table.ensure(table_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(table.p, 0, table_bytes, v.stream);
    return e;
  }

  // What add and apply check of record q before they look at its runs: both reads are among the reads with the lengths the record
  // gives, and the runs spell the record.  walk false with MHAP_OK: a record that takes no part.
  int check_record(const HandleView& v, const char* who, int64_t q, const mhap_record& r, const mhap_align_paths* paths, int64_t (&idx)[2],
                   int64_t& i0, int64_t& j0, bool& walk) const {
    const int64_t o0 = paths->offsets[(size_t)q], o1 = paths->offsets[(size_t)q + 1];
    walk = false;
    if (o1 == o0 || r.from_id == r.to_id) return MHAP_OK;
    if (!find_record_reads(by_id, lengths.data(), who, q, r, idx, *v.err)) return MHAP_E_INVALID;
    std::string what;
    if (!path_spells_record(r, paths->ops, o0, o1, i0, j0, what)) {
      *v.err = std::string(who) + ": record " + std::to_string(q) + " " + what;
      return MHAP_E_INVALID;
    }
    walk = true;
    return MHAP_OK;
  }

  // the walk's item of record q over its runs; idx: its two reads (v_words and view are the caller's)
  VoteItem item_of(const mhap_record& r, const mhap_align_paths* paths, int64_t q, const int64_t (&idx)[2], int64_t i0, int64_t j0) const {
    const int64_t o0 = paths->offsets[(size_t)q], o1 = paths->offsets[(size_t)q + 1];
    VoteItem it{};
    it.a_off = offsets[(size_t)idx[0]]; it.b_off = offsets[(size_t)idx[1]];
    it.ops_off = o0; it.alen = r.alen; it.blen = r.blen; it.i0 = (int32_t)i0; it.j0 = (int32_t)j0;
    it.n_ops = (int32_t)(o1 - o0); it.rc = r.to_rc != 0 ? 1 : 0;
    return it;
  }

  // The records of an add as one item per accepted view: view f of record q votes unless mask says otherwise (mask[q] bit f; nullptr:
  // both views) or its target has `cap` views, which counts it as skipped.  A refused record refuses the call: the views accepted
  // before it are taken back, nothing is counted and the code is returned with the message set.
  int build_items(const HandleView& v, const char* who, const mhap_record* recs, int64_t n, const mhap_align_paths* paths, const uint8_t* mask,
                  uint32_t cap, std::vector<VoteItem>& out) {
    std::vector<int64_t> accepted;   // the targets of the accepted views
    int64_t over = 0;
    for (int64_t q = 0; q < n; q++) {
      int64_t idx[2], i0, j0;
      bool walk;
      const int rc = check_record(v, who, q, recs[q], paths, idx, i0, j0, walk);
      if (rc != MHAP_OK) {
        for (int64_t t : accepted) views[(size_t)t] -= 1;
        out.clear();
        return rc;
      }
      if (!walk) continue;
      for (int view = 0; view < 2; view++) {
        const int64_t target = idx[view];
        if (mask && !(mask[q] & (1u << view))) continue;   // not selected: no vote, no place under the cap, not a skipped view
        if (views[(size_t)target] >= cap) { over++; continue; }
        views[(size_t)target] += 1;
        accepted.push_back(target);
        VoteItem it = item_of(recs[q], paths, q, idx, i0, j0);
        it.v_words = (int64_t)words * pos[(size_t)target];
        it.view = view;
        out.push_back(it);
      }
    }
    skipped += over;
    return MHAP_OK;
  }

  // The runs go up and the items are cast, a grid of at most 2^20 views at a time (the items of one launch are 64 MB):
  // launch(c) starts the vote kernel over the c items in `items` on the handle's stream.
  template <class Launch>
  int cast_votes(const HandleView& v, const char* who, const mhap_align_paths* paths, const std::vector<VoteItem>& its, Launch launch) {
    (void)hipSetDevice(v.device);
    hipError_t e;
    constexpr size_t CHUNK = (size_t)1 << 20;
    if ((e = ops.ensure(4 * paths->ops.size())) != hipSuccess) return hip_fail(v, who, "hipMalloc of the runs", e);
    if ((e = items.ensure(sizeof(VoteItem) * std::min(its.size(), CHUNK))) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
    if ((e = hipMemcpyAsync(ops.p, paths->ops.data(), 4 * paths->ops.size(), hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
    for (size_t g0 = 0; g0 < its.size(); g0 += CHUNK) {
      const size_t c = std::min(CHUNK, its.size() - g0);
      if ((e = hipMemcpyAsync(items.p, its.data() + g0, sizeof(VoteItem) * c, hipMemcpyHostToDevice, v.stream)) != hipSuccess) return hip_fail(v, who, "upload", e);
      launch((unsigned)c);
      if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
      if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);   // (items is reused by the next chunk)
    }
    return MHAP_OK;
  }

  // the counters of read `read_index`, 2 * words per position
  int read_votes(const char* who, int64_t read_index, uint16_t* counters) const {
    HandleView v = handle_view(h);
    if (read_index < 0 || read_index >= n_reads) { *v.err = std::string(who) + ": read " + std::to_string(read_index) + " is not among the " + std::to_string(n_reads) + " reads"; return MHAP_E_INVALID; }
    const int64_t len = lengths[(size_t)read_index];
    if (len == 0) return MHAP_OK;
    if (!counters) { *v.err = std::string(who) + ": null argument"; return MHAP_E_INVALID; }
    return copy_votes(v, who, table.as<uint32_t>(), (int64_t)words * pos[(size_t)read_index], len, words, counters);
  }
};

}  // namespace
}  // namespace mhap
