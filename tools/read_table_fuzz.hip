// read_table_fuzz.hip — the record checks of the sessions' host side (mhap_amd/csrc/read_table.hpp: find_record_reads, range_ok,
// pack_item, ReadTable::pack_records) under the host sanitizers: random tables of reads (ids that repeat, empty reads) and random
// records (unknown ids, wrong lengths, ends before, inside and behind the read) against a plain restatement.  Host code only, no GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I mhap_amd/csrc tools/read_table_fuzz.hip -o read_table_fuzz && ./read_table_fuzz [tables]
#include <cstdio>
#include <random>

#include "read_table.hpp"

using namespace mhap;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); return 1; } } while (0)

enum { OK = 0, UNKNOWN, LENGTH, RANGE };

static bool ends_inside(const mhap_record& r) {
  return r.score == 0.0 || (0 <= r.a1 && r.a1 <= r.a2 && r.a2 < r.alen && 0 <= r.b1 && r.b1 <= r.b2 && r.b2 < r.blen);
}

// what a record is refused for, the lookup of both reads first, and the reads' positions (the first read of an id)
static int restated(const std::vector<int64_t>& ids, const std::vector<int32_t>& lengths, const mhap_record& r, bool ranged, int32_t (&idx)[2]) {
  const int64_t rid[2] = {r.from_id, r.to_id};
  const int32_t lens[2] = {r.alen, r.blen};
  for (int f = 0; f < 2; f++) {
    idx[f] = -1;
    for (size_t i = 0; i < ids.size() && idx[f] < 0; i++) if (ids[i] == rid[f]) idx[f] = (int32_t)i;
    if (idx[f] < 0) return UNKNOWN;
    if (lengths[(size_t)idx[f]] != lens[f]) return LENGTH;
  }
  return ranged && !ends_inside(r) ? RANGE : OK;
}

int main(int argc, char** argv) {
  const int tables = argc > 1 ? atoi(argv[1]) : 2000;
  std::mt19937_64 rng(20261020);
  auto rnd = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
  const char* words[4] = {"", " names read ", " gives read ", " aligns "};
  int64_t seen[4] = {0, 0, 0, 0};
  for (int t = 0; t < tables; t++) {
    ReadTable T;
    const int64_t n = rnd(0, 40), id_span = rnd(1, 60);
    for (int64_t i = 0; i < n; i++) {
      T.ids.push_back(rnd(-3, id_span));
      T.lengths.push_back(rnd(0, 4) == 0 ? 0 : (int32_t)rnd(1, 500));
      T.by_id.emplace(T.ids.back(), (int32_t)i);
    }
    T.n_reads = n;
    std::vector<mhap_record> recs((size_t)rnd(0, 30));
    for (mhap_record& r : recs) {
      r = mhap_record{};
      r.from_id = rnd(-3, id_span + 2); r.to_id = rnd(-3, id_span + 2);
      auto len_of = [&](int64_t id) { const auto it = T.by_id.find(id); return it == T.by_id.end() || rnd(0, 9) == 0 ? (int32_t)rnd(-1, 500) : T.lengths[(size_t)it->second]; };
      r.alen = len_of(r.from_id); r.blen = len_of(r.to_id);
      r.a1 = (int32_t)rnd(-1, 20); r.a2 = rnd(0, 3) ? (int32_t)rnd(r.a1, std::max<int64_t>(r.a1, r.alen - 1)) : (int32_t)rnd(-2, r.alen + 2);
      r.b1 = (int32_t)rnd(-1, 20); r.b2 = rnd(0, 3) ? (int32_t)rnd(r.b1, std::max<int64_t>(r.b1, r.blen - 1)) : (int32_t)rnd(-2, r.blen + 2);
      r.to_rc = (int32_t)rnd(0, 2); r.score = rnd(0, 5) ? 0.5 + 0.01 * (double)rnd(0, 50) : 0.0;
    }
    for (int64_t q = 0; q < (int64_t)recs.size(); q++) {   // record by record: the lookup, then the ends
      int32_t want[2], got[2] = {-7, -7};
      std::string err;
      const int plain = restated(T.ids, T.lengths, recs[(size_t)q], false, want);
      CHECK(T.find_reads("who", q, recs[(size_t)q], got, err) == (plain == OK));
      CHECK(plain != OK ? err.find(std::string("who: record ") + std::to_string(q) + words[plain]) == 0 : err.empty() && got[0] == want[0] && got[1] == want[1]);
      if (plain == OK) {
        const GItem it = pack_item(got, recs[(size_t)q]);
        CHECK(it.a == want[0] && it.brc >> 1 == want[1] && (it.brc & 1) == (recs[(size_t)q].to_rc != 0) && it.a1 == recs[(size_t)q].a1 && it.b2 == recs[(size_t)q].b2);
      }
      const int ranged = restated(T.ids, T.lengths, recs[(size_t)q], true, want);
      err.clear();
      CHECK(range_ok("who", q, recs[(size_t)q], err) == ends_inside(recs[(size_t)q]));
      seen[ranged]++;
    }
    std::vector<GItem> out;   // the whole call: refused at the first refused record, with that record's message
    std::string err;
    int64_t first = -1, why = OK;
    int32_t idx[2];
    for (int64_t q = 0; q < (int64_t)recs.size() && first < 0; q++)
      if ((why = restated(T.ids, T.lengths, recs[(size_t)q], true, idx)) != OK) first = q;
    CHECK(T.pack_records("who", recs.data(), (int64_t)recs.size(), out, err) == (first < 0));
    CHECK(first < 0 ? out.size() == recs.size() : err.find(std::string("who: record ") + std::to_string(first) + words[why]) == 0);
  }
  printf("%d tables: %lld records taken, %lld unknown, %lld of another length, %lld with ends outside\n", tables, (long long)seen[OK],
         (long long)seen[UNKNOWN], (long long)seen[LENGTH], (long long)seen[RANGE]);
  return seen[OK] && seen[UNKNOWN] && seen[LENGTH] && seen[RANGE] ? 0 : 1;
}
