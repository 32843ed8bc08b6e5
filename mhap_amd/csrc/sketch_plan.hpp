// sketch_plan.hpp — the host rules of the sketch phase's driver (sketch_staged in mhap_capi.hip): launch groups, one group's descriptor layout,
// length order and the ordered kernel's place around the MinHash launch.  Pure functions: no HIP call, no handle
// (mhap_selftest_sketch_plan / mhap_selftest_ordered_schedule run them without a GPU).
#pragma once
#include <climits>
#include <cstdint>
#include <vector>

#include "capi_switches.hpp"

namespace mhap {

inline int64_t align4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// Bases per launch group: 16 B of scratch per base (weights + class lists of both strands) = 16 GB of the 288 GB at 2^30; fewer, larger
// launches = fewer drain tails of the persistent MinHash waves (a strand takes ~2 ms).
// Round 6: larger launch groups where the HBM is there — a job of more than 1 G bases (configs[3]: 15 G) is cut into groups of up to 4 G bases
// as long as their scratch stays under a quarter of the memory that is free now: 14 -> 4 groups at C4, 1 469 -> 1 437 ms on one box (fewer
// drain tails, fewer launches into an idle GPU).  The groups of one rank of configs[4] at N = 8 (137 GB in use) stay where they were.
// (free_bytes = 0: the free memory is not known; override = MHAP_BATCH_BASES)
inline int64_t launch_group_bases(size_t free_bytes, long long override) {
  if (override > 0) return override;
  return std::max<int64_t>(1LL << 30, std::min<int64_t>(4LL << 30, (int64_t)(free_bytes / 4 / 16)));
}

// entries of a weight workgroup's HBM slab: a power of two with room for 4/3 of the longest strand's k-mers
inline int64_t slab_entries(int max_len, int k) {
  int64_t se = 64;
  while (3 * se < 4LL * std::max(1, max_len - k + 1)) se <<= 1;
  return se;
}

// One launch group's reads laid out in the scratch arrays: every read gets its strides and w_off; a read that is not skipped takes
// 2 x align4(k-mers) weight elements (both strands, adjacent), and 2 x align4 key / 32-bit hash elements as well when is_mat(read) says its hashes
// are materialised (MHAP_RD_MAT is set on it).  out = nullptr: the totals only.
struct GroupLayout {
  int64_t key_elems = 0, h2_elems = 0, w_elems = 0, read_bases = 0;   // read_bases: every read's, skipped ones too
  bool any_mat = false;
  int min_len = INT32_MAX, max_len = 0, max_len_codes = 0;   // of the reads not skipped; max_len_codes: of those hashed from their 2-bit codes
};
template <class IsMat>
GroupLayout layout_group(const ReadDesc* in, int64_t nb, int k, int k2, IsMat is_mat, ReadDesc* out) {
  GroupLayout g;
  for (int64_t i = 0; i < nb; i++) {
    ReadDesc d = in[i];
    const int64_t nk = align4(std::max(0, d.length - k + 1)), nk2 = align4(std::max(0, d.length - k2 + 1));
    g.read_bases += d.length;
    d.key_off = d.h2_off = 0;
    d.w_off = g.w_elems; d.key_stride = (int32_t)nk; d.h2_stride = (int32_t)nk2;
    if (!(d.flags & MHAP_RD_SKIP)) {
      g.min_len = std::min(g.min_len, d.length); g.max_len = std::max(g.max_len, d.length);
      g.w_elems += 2 * nk;
      if (is_mat(d)) {
        d.flags |= MHAP_RD_MAT; g.any_mat = true;
        d.key_off = g.key_elems; d.h2_off = g.h2_elems;
        g.key_elems += 2 * nk; g.h2_elems += 2 * nk2;
      } else g.max_len_codes = std::max(g.max_len_codes, d.length);
    }
    if (out) out[i] = d;
  }
  return g;
}

// The launch groups of n staged reads: at most 2^22 reads each; a group is closed before the read that would pass group_bases, except that a
// group always takes its first read.  The worst-case scratch sizes (allocated once) are the maxima of the groups' layout totals.
struct LaunchGroup { int64_t r0, r1; int max_len; };
struct SketchPlan {
  std::vector<LaunchGroup> groups;
  int64_t max_key = 4, max_h2 = 4, max_w = 4, max_nb = 1;
  int max_len_all = 0;
};
template <class IsMat>
SketchPlan plan_launch_groups(const ReadDesc* descs, int64_t n, int64_t group_bases, int k, int k2, IsMat is_mat) {
  SketchPlan p;
  for (int64_t r0 = 0; r0 < n;) {
    int64_t r1 = r0, tot = 0;
    while (r1 < n && (r1 == r0 || tot + descs[r1].length <= group_bases) && (r1 - r0) < (1 << 22)) { tot += descs[r1].length; r1++; }
    const GroupLayout g = layout_group(descs + r0, r1 - r0, k, k2, is_mat, nullptr);
    p.max_key = std::max(p.max_key, g.key_elems); p.max_h2 = std::max(p.max_h2, g.h2_elems); p.max_w = std::max(p.max_w, g.w_elems);
    p.max_nb = std::max(p.max_nb, r1 - r0); p.max_len_all = std::max(p.max_len_all, g.max_len);
    p.groups.push_back(LaunchGroup{r0, r1, g.max_len});
    r0 = r1;
  }
  return p;
}

// Reads of clearly different lengths are handed out longest first (a stable counting sort on length / 128), so that the persistent
// workgroups do not end on a long read while the rest of the GPU idles.  false = no order: a single read, or 5 min_len >= 4 max_len.
// (a read longer than max_len — none that is sketched — shares the longest reads' bucket)
inline bool length_order(const ReadDesc* descs, int64_t nb, int min_len, int max_len, std::vector<int32_t>& order) {
  if (5LL * min_len >= 4LL * max_len || nb <= 1) return false;
  const int nbk = max_len / 128 + 2;
  auto bucket = [&](int64_t i) { return (size_t)std::max(0, nbk - 1 - descs[i].length / 128); };
  std::vector<int64_t> start((size_t)nbk + 1, 0);
  for (int64_t i = 0; i < nb; i++) start[bucket(i)]++;
  int64_t acc = 0;
  for (int b = 0; b <= nbk; b++) { const int64_t c = start[(size_t)b]; start[(size_t)b] = acc; acc += c; }
  order.resize((size_t)nb);
  for (int64_t i = 0; i < nb; i++) order[(size_t)start[bucket(i)]++] = (int32_t)i;
  return true;
}

// Round 6: PART of the ordered kernel runs between the weight kernel's read-back and the weight-1 MinHash launch, and the weighted strands'
// MinHash launch (its own stream) runs NEXT TO THAT PART instead of next to the weight-1 launch's start.  Measured, not derived (EXPERIMENTS.md,
// round 6, "the MinHash launch's clock"): the weight-1 launch of C2 — 75 ms at the card's power limit — holds whatever clock the power
// management settles on when it starts.  Started into an idle GPU (the read-back is a host round trip) together with the weighted launch it held
// 1 820-2 126 MHz from step to step; started alone, right behind a running, moderately busy kernel, 2 164-2 179 MHz every time
// (MHAP_MINHASH_PROF): 76.2-76.8 -> 72.1-72.4 ms, the C2 step 93.4-94.6 -> 90.5-91.3 ms on one box.  With the weighted launch made to wait for
// the ordered part the gain is gone (76.1-76.3); behind memory fills the clock is 1 800; with an idle gap behind the ordered part 1 850-2 030.
// The rest of the strands' ordered rows are made behind the MinHash launch, next to the index build as before (the build takes about as long as
// 0.45 of the ordered kernel beside it).  Only where a LONG weight-1 launch is the job: a launch group of 0.9 G bases of reads or more (a
// MinHash launch of 60 ms and more: C2 on one GPU, the launch groups of C4) with at most a fifth of the strands weighted.  Shorter launches
// lose by it — one rank's share of an N-GPU C2 job, same box, alternating: N = 2 / 4 / 8 rank step 50.5 -> 50.7 / 26.85 -> 27.6 / 14.8 -> 15.2 ms —
// and a -f run's strands are all weighted (its MinHash launch would run under the ordered part from the start: c5slice 180.3 -> 180.5 / 184.6).
// MHAP_ORDERED_SPLIT = per cent of the strands in the first part (0 = rounds 1-5's order, 100 = all of them); MHAP_ORDERED_NOWAIT=0 makes the
// weighted launch wait for the first part; MHAP_ORDERED_FIRST=1 / 2 = all of it first / and an idle gap behind it (the experiments: round 6,
// EXPERIMENTS.md "the MinHash launch's clock"); MHAP_W1_PREFILL=n = n fills of the queue buffer in front of the MinHash launch (it is enqueued
// behind running work).
// pre: strands whose ordered rows are made in front of the MinHash launch — even (both strands of a read in one part), and 0 under the eager
// exchange, which makes all rows first by its own branch.  nowait = false only where there is a first part to wait for.
struct OrderedSchedule { int64_t pre; bool nowait, idle_gap; int prefill; };
inline OrderedSchedule ordered_schedule(const Switches& sw, int64_t group_read_bases, int64_t n_w1, int64_t n_weighted, int64_t nstr, bool eager_x) {
  const bool split_pays = group_read_bases >= 900000000LL && n_w1 >= 4 * n_weighted;
  int64_t pre = sw.ordered_first ? nstr : (nstr * (int64_t)(sw.ordered_split >= 0 ? sw.ordered_split : (split_pays ? 55 : 0))) / 100;
  pre &= ~(int64_t)1;
  if (eager_x || pre < 0) pre = 0;
  return OrderedSchedule{pre, sw.ordered_nowait || pre == 0, sw.ordered_first == 2, sw.w1_prefill};
}

}  // namespace mhap
