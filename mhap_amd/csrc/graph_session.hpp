// graph_session.hpp — the session of the string graph as its two units see it: graph_kernels.hip (the class rule and the arc list) and
// unitig_kernels.hip (the unitigs, their spelling, the cleaning).  No kernels: the session, its buffers in groups by lifetime, the
// indices of the count vectors, the two structs the kernels of both units read, and the refusals and the copy-out that the
// mhap_graph_copy_* calls share.  The table of reads, a record's lookup, the queued uploads, Steps and begin / free are read_table.hpp's.
#pragma once
#include <type_traits>

#include "read_table.hpp"

namespace mhap {
namespace {

// counts: records, the six classes, contained reads, arcs, reduced, final
enum { GC_RECORDS = 0, GC_CLASS0 = 1, GC_CONTAINED = 7, GC_ARCS = 8, GC_REDUCED = 9, GC_FINAL = 10 };
enum { UC_CIRCULAR = 0, UC_JOINED = 1, UC_LONGEST = 2, UC_DEVICE = 3 };
enum { CC_ROUNDS = 0, CC_TIPS, CC_TIP_READS, CC_BUBBLES, CC_BUBBLE_READS, CC_ARCS };

// (GItem, the record as it goes up, the class codes and the parameters are graph_class.hpp's)
struct GArc { int32_t u, v, len, q; };   // two of them over a GItem; u = -1: no arc
static_assert(sizeof(GArc) == 16, "an item is two arcs");

struct UTables {   // the unitigs of a round where the kernels find them; the sizes stay on the device
  const int64_t *nu, *nm, *nl, *u_start, *u_len;
  const uint8_t* u_circ;
  const int32_t *m_vertex, *links;
};

// The state a call needs: the arc list of a finish; that list with no record added since (an add may have set contained flags the
// list does not know of); a completed clean; served unitigs.
enum GraphNeed { NEED_NOTHING, NEED_ARCS, NEED_FINISH, NEED_CLEAN, NEED_UNITIGS };

// The session's buffers, in groups by lifetime.  A group is a struct of Dev<T> members and nothing else, so that release_group can
// walk it as the DevBufs it is made of: a buffer is named once, with its element type, and none can be missing from a release.
template <class G>
void release_group(G& g) {
  static_assert(std::is_standard_layout<G>::value && sizeof(Dev<char>) == sizeof(DevBuf) && sizeof(G) % sizeof(DevBuf) == 0, "Dev<T> members only");
  DevBuf* b = reinterpret_cast<DevBuf*>(&g);
  for (size_t i = 0; i < sizeof(G) / sizeof(DevBuf); i++) b[i].release();
}

struct GraphAdds {   // what the adds sum, from begin on: a word per read, MHAP_GRAPH_COUNTS counts (the classes)
  Dev<uint32_t> contained; Dev<u64> counts;
  void release() { release_group(*this); }
};
struct GraphArcs {   // the arc list a finish makes
  Dev<int32_t> deg, fill, U, V, LEN, Q, bt_v, bt_pos, mark, rows;
  Dev<int64_t> start, fstart; Dev<GArc> tmp; Dev<uint8_t> keep;
  void release() { release_group(*this); }
};
struct UnitigBuild {   // the scratch and the numbering of a unitig build; P / R / O and Q / M are read from one buffer and written to the other
  Dev<int32_t> fout, cand, carc, next, prev, span, P[2], Q[2], M[2], tail, cnt, kept, islink;
  Dev<uint32_t> R[2]; Dev<u64> O[2], ucounts; Dev<uint8_t> cyc;
  Dev<int64_t> ulen, unum, mstart, bstart, lstart;
  void release() { release_group(*this); }
};
struct UnitigTables {   // the unitigs that the copy and spell calls serve
  Dev<int64_t> u_start, u_len, m_offset, m_dst; Dev<uint8_t> u_circ;
  Dev<int32_t> m_vertex, m_span, links;
  void release() { release_group(*this); }
};
struct CleanState {   // dropped (per read) and removed (per arc) hold from a mhap_graph_clean to the next finish; the rest is a round's
  Dev<uint8_t> dropped, removed, o_cand, verdict; Dev<u64> ccounts; Dev<int32_t> o_lo, o_hi;
  void release() { release_group(*this); }
};
struct SpellStage {   // a spell's read offsets, the bases a host caller brought, and the output before it goes down
  Dev<int64_t> roff; Dev<uint8_t> bases, spelled;
  void release() { release_group(*this); }
};

}  // namespace
}  // namespace mhap

// An add keeps a chunk of its own (the records stay on the device until the session goes), so the table's one `items` buffer, and
// with it queue_add / commit_add, are not used here.
struct mhap_graph_session : mhap::ReadTable {
  static constexpr bool any_length = true;                // lengths up to 2^31 - 1: no kernel of the graph indexes a base by them
  mhap::GParams P{};
  int64_t n_arcs = -1;                                    // n_arcs < 0: no finish yet
  struct Chunk {                                          // one add: its records, which classify_kernel overwrites with two arc slots each
    mhap::Dev<mhap::GArc> items; mhap::Dev<uint8_t> cls; int64_t n = 0;
    void release() { items.release(); cls.release(); }
  };
  std::deque<Chunk> chunks;
  mhap::GraphAdds ad; mhap::GraphArcs arc;
  // unitigs: rebuilt by every mhap_graph_unitigs, invalid (n_unitigs < 0) from the next finish on
  int64_t n_contained = 0, finish_records = 0, n_unitigs = -1, n_members = 0, n_links = 0, n_ubases = 0;
  mhap::UnitigBuild ub; mhap::UnitigTables ut; mhap::SpellStage sp;
  int64_t last_counts[MHAP_UNITIG_COUNTS] = {0};          // the counts of the unitigs now served
  int u_cur = 0;                                          // which of ub.P / R / O the last build's ranks ended in
  bool cleaned = false;                                   // a mhap_graph_clean has completed since the last finish
  uint64_t unitig_gen = 0;                                // bumped whenever the served unitigs go or change: a consensus session's key
  mhap::CleanState cl;
  void release() {
    release_table();
    for (auto& c : chunks) c.release();
    chunks.clear();
    ad.release(); arc.release(); ub.release(); ut.release(); sp.release(); cl.release();
  }

  // ---- what the calls that read a session share: MHAP_OK, or the refusal with the handle's message set
  int refuse(const char* who, const char* why) { *mhap::handle_view(h).err = std::string(who) + why; return MHAP_E_INVALID; }
  int null_arg(const char* who) { return refuse(who, ": null argument"); }
  int need(const char* who, mhap::GraphNeed what) {
    using namespace mhap;
    if ((what == NEED_ARCS || what == NEED_FINISH) && n_arcs < 0) return refuse(who, ": no mhap_graph_finish has completed");
    if (what == NEED_FINISH && n_records != finish_records) return refuse(who, ": records were added after the last mhap_graph_finish");
    if (what == NEED_CLEAN && !cleaned) return refuse(who, ": no mhap_graph_clean has completed since the last mhap_graph_finish");
    if (what == NEED_UNITIGS && n_unitigs < 0) return refuse(who, ": no mhap_graph_unitigs has completed since the last mhap_graph_finish");
    return MHAP_OK;
  }
  // A copy call behind its null-session check, in the order every one of them keeps: the state, nothing to copy (n == 0), a null
  // pointer among the caller's (`null`), the downloads.
  int copy_out(const char* who, mhap::GraphNeed what, int64_t n, bool null, const std::vector<mhap::Copy>& copies) {
    int rc = need(who, what);
    if (rc != MHAP_OK || n == 0) return rc;
    if (null) return null_arg(who);
    for (const mhap::Copy& c : copies)
      if ((rc = download(who, c.dst, c.src, c.bytes)) != MHAP_OK) return rc;
    return MHAP_OK;
  }
};
