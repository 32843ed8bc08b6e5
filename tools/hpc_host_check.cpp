// hpc_host_check.cpp — the host code of the homopolymer compression under the sanitizers, as a program of its own (no GPU, no HIP, nothing
// loaded into Python): mhap_hpc_expand_record, the grouping loop and the builder of the table of tiles (mhap_amd/csrc/hpc_common.hpp,
// hpc_host.cpp) taken through the edge records and the edge tables.  From the repository's root:
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/hpc_host_check.cpp mhap_amd/csrc/hpc_host.cpp -o hpc_host_check
//   ./hpc_host_check        (prints "hpc_host_check: ok" and exits 0; a failed check names its line and exits 1)
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "../mhap_amd/csrc/hpc_common.hpp"

using namespace mhap;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "hpc_host_check: line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

namespace {

// the restatement: heads and start[] of a read
std::vector<int32_t> starts_of(const std::vector<uint8_t>& x) {
  std::vector<int32_t> s;
  for (size_t p = 0; p < x.size(); p++) if (p == 0 || x[p] != x[p - 1]) s.push_back((int32_t)p);
  s.push_back((int32_t)x.size());
  return s;
}

void check_records(std::mt19937_64& rng) {
  for (int trial = 0; trial < 200; trial++) {
    std::vector<uint8_t> a(rng() % 40), b(rng() % 40);
    for (auto& c : a) c = "AC"[rng() % 2];
    for (auto& c : b) c = "GT"[rng() % 2];
    const std::vector<int32_t> sa = starts_of(a), sb = starts_of(b);   // exactly clen + 1 entries each: a read past them is caught
    const int32_t ca = (int32_t)sa.size() - 1, cb = (int32_t)sb.size() - 1, La = (int32_t)a.size(), Lb = (int32_t)b.size();
    for (int32_t p : {-1, 0, ca - 1, ca, ca / 2})
      for (int32_t q : {-1, 0, cb - 1, cb, cb / 2})
        for (int32_t rc : {0, 1}) {
          mhap_record in{}, out{};
          in.from_id = 7; in.to_id = 9; in.score = 0.5; in.raw = 3.0; in.to_rc = rc;
          in.a1 = p; in.a2 = q < ca ? q : ca; in.alen = ca; in.b1 = q; in.b2 = p < cb ? p : cb; in.blen = cb;
          CHECK(mhap_hpc_expand_record(&in, sa.data(), ca, sb.data(), cb, &out) == 0);
          CHECK(out.from_id == 7 && out.to_id == 9 && out.score == 0.5 && out.raw == 3.0 && out.to_rc == rc);
          CHECK(out.alen == La && out.blen == Lb);
          CHECK(out.a1 == (p < 0 ? -1 : p < ca ? sa[(size_t)p] : La));
          CHECK(out.b1 == (q < 0 ? -1 : q < cb ? sb[(size_t)q] : Lb));
          CHECK(out.a2 == (in.a2 < 0 ? -1 : in.a2 < ca ? sa[(size_t)in.a2 + 1] - 1 : La));
          CHECK(out.b2 == (in.b2 < 0 ? -1 : in.b2 < cb ? sb[(size_t)in.b2 + 1] - 1 : Lb));
          // the flip: the ends expanded on the reversed read's map and flipped are the flipped ends expanded on the forward map
          std::vector<uint8_t> r(b.rbegin(), b.rend());
          const std::vector<int32_t> sr = starts_of(r);
          CHECK(Lb - hpc_hi(sr.data(), cb, q) - 1 == hpc_lo(sb.data(), cb, cb - q - 1));
          CHECK(Lb - hpc_lo(sr.data(), cb, q) - 1 == hpc_hi(sb.data(), cb, cb - q - 1));
        }
    mhap_record r{};
    CHECK(mhap_hpc_expand_record(nullptr, sa.data(), ca, sb.data(), cb, &r) == -1);
    CHECK(mhap_hpc_expand_record(&r, sa.data(), -1, sb.data(), cb, &r) == -1);
  }
}

void check_plan(const std::vector<int32_t>& lengths, int64_t cap) {
  const int64_t n = (int64_t)lengths.size();
  const std::vector<HpcGroup> groups = hpc_plan_groups(lengths.data(), n, cap);
  std::vector<int32_t> first, owner;
  std::vector<HpcTile> tiles;
  std::vector<int64_t> offsets((size_t)n);
  for (int64_t i = 0; i < n; i++) offsets[(size_t)i] = 1000 * i + 7;   // anywhere: the table does not look at the bases
  CHECK(hpc_build_tiles(offsets.data(), lengths.data(), n, first, owner, tiles));
  CHECK(tiles.size() == owner.size());
  CHECK((int64_t)first.size() == n + 1 && first[(size_t)n] == (int32_t)owner.size());
  int64_t r = 0, t = 0;
  for (const HpcGroup& g : groups) {
    CHECK(g.r0 == r && g.r1 > g.r0 && g.tile0 == t);   // whole reads, in order, none left out
    int64_t bases = 0, tiles = 0;
    for (int64_t i = g.r0; i < g.r1; i++) { bases += lengths[(size_t)i]; tiles += hpc_tiles_of(lengths[(size_t)i]); }
    CHECK(bases == g.bases && tiles == g.tiles);
    CHECK(g.bases <= cap || g.r1 - g.r0 == 1);           // over the cap: a read of its own
    if (g.r1 < n) CHECK(g.bases + lengths[(size_t)g.r1] > cap);   // closed only in front of the read that would not fit
    r = g.r1; t += g.tiles;
  }
  CHECK(r == n && t == (int64_t)owner.size());
  for (int64_t i = 0; i < n; i++) {
    CHECK(first[(size_t)i + 1] - first[(size_t)i] == hpc_tiles_of(lengths[(size_t)i]));
    for (int32_t k = first[(size_t)i]; k < first[(size_t)i + 1]; k++) {
      const HpcTile& tl = tiles[(size_t)k];
      CHECK(owner[(size_t)k] == i && tl.len == lengths[(size_t)i] && tl.pos == (k - first[(size_t)i]) * MHAP_HPC_TILE && tl.pos < tl.len);
      CHECK(tl.addr == offsets[(size_t)i] + tl.pos);
    }
  }
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261020);
  check_records(rng);
  const int32_t T = MHAP_HPC_TILE;
  check_plan({}, 3 * T);
  check_plan({0, 0, 0}, 3 * T);
  check_plan({T, 2 * T, 3 * T, 0, 3 * T + 1, 1, 0, 0, 3 * T - 1, T + 5, T, T, 0, 17, 5 * T + 3, 0, 2 * T, T - 1, 1, 1}, 3 * T);
  check_plan({INT32_MAX - 8, 1, INT32_MAX - 8}, HPC_GROUP_MAX);
  for (int trial = 0; trial < 50; trial++) {
    std::vector<int32_t> lengths(rng() % 60);
    for (auto& L : lengths) L = (int32_t)(rng() % 4 == 0 ? 0 : rng() % (3 * T));
    check_plan(lengths, (int64_t)(1 + rng() % (4 * T)));
  }
  printf("hpc_host_check: ok\n");
  return 0;
}
