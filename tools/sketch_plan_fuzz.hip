// sketch_plan_fuzz.hip — the sketch driver's host rules (mhap_amd/csrc/sketch_plan.hpp) under the host sanitizers: the fixed cases of
// tests/test_host_logic.py and a few thousand random descriptor lists.  Host code only, no GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I mhap_amd/csrc tools/sketch_plan_fuzz.hip -o sketch_plan_fuzz && ./sketch_plan_fuzz [lists]
#include <cstdio>
#include <random>

#include "sketch_plan.hpp"

using namespace mhap;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int check_list(const std::vector<ReadDesc>& descs, int64_t group_bases, int k, int k2, bool fused) {
  const int64_t n = (int64_t)descs.size();
  auto is_mat = [&](const ReadDesc& d) { return (d.flags & MHAP_RD_RAW) || !fused || d.length > 24000; };
  const SketchPlan p = plan_launch_groups(descs.data(), n, group_bases, k, k2, is_mat);
  std::vector<ReadDesc> out((size_t)n);
  std::vector<int32_t> order;
  int64_t next = 0;
  for (const LaunchGroup& B : p.groups) {
    CHECK(B.r0 == next && B.r1 > B.r0 && B.r1 <= n && B.r1 - B.r0 <= p.max_nb);
    next = B.r1;
    int64_t tot = 0;
    for (int64_t i = B.r0; i < B.r1; i++) tot += descs[(size_t)i].length;
    CHECK(B.r1 - B.r0 == 1 || tot <= group_bases);                                        // only a group's first read may pass the budget
    CHECK(B.r1 == n || tot + descs[(size_t)B.r1].length > group_bases);                   // ... and the next read would
    const GroupLayout G = layout_group(descs.data() + B.r0, B.r1 - B.r0, k, k2, is_mat, out.data() + B.r0);
    CHECK(G.max_len == B.max_len && G.read_bases == tot);
    CHECK(G.key_elems <= p.max_key && G.h2_elems <= p.max_h2 && G.w_elems <= p.max_w && G.max_len <= p.max_len_all);
    for (int64_t i = B.r0; i < B.r1; i++) {
      const ReadDesc& d = out[(size_t)i];
      CHECK(d.w_off % 4 == 0 && d.key_off % 4 == 0 && d.h2_off % 4 == 0 && d.key_stride % 4 == 0 && d.h2_stride % 4 == 0);
      if (d.flags & MHAP_RD_SKIP) { CHECK(!(d.flags & MHAP_RD_MAT)); continue; }
      CHECK(d.w_off + 2 * (int64_t)d.key_stride <= G.w_elems);                            // both strands inside the group's arrays
      if (d.flags & MHAP_RD_MAT) CHECK(d.key_off + 2 * (int64_t)d.key_stride <= G.key_elems && d.h2_off + 2 * (int64_t)d.h2_stride <= G.h2_elems);
      else CHECK(d.key_off == 0 && d.h2_off == 0 && d.length <= G.max_len_codes);
    }
    if (length_order(out.data() + B.r0, B.r1 - B.r0, G.min_len, B.max_len, order)) {
      CHECK((int64_t)order.size() == B.r1 - B.r0 && 5LL * G.min_len < 4LL * B.max_len);
      std::vector<char> seen(order.size(), 0);
      for (size_t j = 0; j < order.size(); j++) {
        CHECK(order[j] >= 0 && (size_t)order[j] < order.size() && !seen[(size_t)order[j]]);
        seen[(size_t)order[j]] = 1;
        if (j == 0) continue;
        const int top = B.max_len / 128 + 1;   // (a skipped read beyond the longest kept one shares the front bucket)
        const int a = std::min(out[(size_t)(B.r0 + order[j - 1])].length / 128, top), b = std::min(out[(size_t)(B.r0 + order[j])].length / 128, top);
        CHECK(a > b || (a == b && order[j - 1] < order[j]));                               // longest first, stable within a bucket
      }
    }
    CHECK(slab_entries(B.max_len, k) >= 64 && 3 * slab_entries(B.max_len, k) >= 4LL * std::max(1, B.max_len - k + 1));
  }
  CHECK(next == n);
  return 0;
}

static int fixed_cases() {
  const int64_t G = 1LL << 30;
  CHECK(launch_group_bases(0, 0) == G && launch_group_bases((size_t)64 << 30, 0) == G && launch_group_bases((size_t)288 << 30, 0) == 4 * G);
  CHECK(launch_group_bases((size_t)256 << 30, 0) == 4 * G && launch_group_bases(((size_t)256 << 30) - 64, 0) == 4 * G - 1);
  CHECK(launch_group_bases((size_t)288 << 30, 200000) == 200000 && launch_group_bases(0, 3000) == 3000);
  std::vector<ReadDesc> d(5, ReadDesc{});
  const int len[5] = {100, 15, 16, 3000, 100};
  for (int i = 0; i < 5; i++) d[(size_t)i].length = len[i];
  auto never = [](const ReadDesc&) { return false; };
  const SketchPlan p = plan_launch_groups(d.data(), 5, 3000, 16, 12, never);
  CHECK(p.groups.size() == 3 && p.groups[0].r1 == 3 && p.groups[1].r1 == 4 && p.groups[1].max_len == 3000 && p.max_nb == 3);
  CHECK(plan_launch_groups(d.data(), 5, 2999, 16, 12, never).groups.size() == 3 && plan_launch_groups(d.data(), 5, 3100, 16, 12, never).groups.size() == 2);
  if (check_list(d, 3000, 16, 12, true) || check_list(d, 3000, 16, 12, false) || check_list({}, 1, 16, 12, true)) return 1;
  Switches sw;
  auto pre = [&](int64_t bases, int64_t w1, int64_t wt, int64_t nstr, bool eager) { return ordered_schedule(sw, bases, w1, wt, nstr, eager).pre; };
  CHECK(pre(900000000, 800, 200, 1000, false) == 550 && pre(899999999, 800, 200, 1000, false) == 0 && pre(900000000, 799, 200, 1000, false) == 0);
  sw.ordered_split = 33;
  CHECK(pre(0, 800, 200, 1000, false) == 330 && pre(0, 800, 200, 1002, false) == 330 && pre(0, 800, 200, 1010, false) == 332 && pre(0, 800, 200, 1000, true) == 0);
  sw.ordered_nowait = false;
  CHECK(!ordered_schedule(sw, 0, 800, 200, 1000, false).nowait && ordered_schedule(sw, 0, 800, 200, 1000, true).nowait);
  sw.ordered_split = 100; sw.ordered_first = 0;
  CHECK(pre(0, 1, 1, 1000, false) == 1000);
  sw.ordered_split = -1; sw.ordered_first = 2;
  CHECK(pre(0, 1, 1, 1000, false) == 1000 && ordered_schedule(sw, 0, 1, 1, 1000, false).idle_gap && pre(0, 1, 1, 0, false) == 0);
  return 0;
}

int main(int argc, char** argv) {
  if (fixed_cases()) return 1;
  const int lists = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937_64 rng(20261020);
  auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  int64_t reads = 0;
  for (int t = 0; t < lists; t++) {
    const int64_t n = t % 8 == 0 ? rnd(0, 70000) : rnd(0, 3000);   // (every eighth list up to the full 70 000 reads)
    const int max_read = (int)rnd(1, 4) * 10000;
    std::vector<ReadDesc> d((size_t)n, ReadDesc{});
    for (ReadDesc& r : d) {
      r.length = rnd(0, 9) == 0 ? (int)rnd(0, 200) : (int)rnd(0, max_read);
      r.flags = (rnd(0, 5) == 0 ? MHAP_RD_SKIP : 0) | (rnd(0, 4) == 0 ? MHAP_RD_RAW : 0) | (rnd(0, 1) ? MHAP_RD_FWDONLY : 0);
    }
    const int64_t group_bases = rnd(0, 3) == 0 ? rnd(1, 2000) : rnd(1, 40LL * max_read * (n / 4 + 1));
    const int k = rnd(0, 3) ? 16 : (int)rnd(1, 40), k2 = rnd(0, 3) ? 12 : (int)rnd(1, 40);
    if (check_list(d, group_bases, k, k2, rnd(0, 3) != 0)) { fprintf(stderr, "list %d: n %lld group_bases %lld k %d k2 %d\n", t, (long long)n, (long long)group_bases, k, k2); return 1; }
    reads += n;
  }
  printf("sketch_plan_fuzz: fixed cases and %d random lists (%lld reads) clean\n", lists, (long long)reads);
  return 0;
}
