// capi_switches.hpp — what the drivers of mhap_capi.hip know by name: the words of the handle's counter block and the MHAP_* environment
// switches that file reads, one field each.  Nothing is cached: every read_* below runs where its variables were always read (tests switch
// them between calls inside one process).  docs/DESIGN.switches.md lists what each one does.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "kernels.hpp"

namespace mhap {

// h->counters: 32 words of 8 bytes.  A sketch launch group zeroes all of them, a candidate pass of a search the first SC_LAST_JOIN + 1.  The
// kernels get each word as a pointer of its own (the weight and MinHash kernels the block's base); OJ_GROUP_BAD is the one offset the device knows.
enum SketchCounter { KC_BASE = 0, KC_LIST_W1 = 4, KC_LIST_WEIGHTED = 5 };   // lengths of the two MinHash work lists, written by the weight kernel
enum SearchCounter {
  SC_CAND = 0, SC_REC = 1, SC_COMPARED = 2,   // candidates, records, pairs compared: what a chunk's tail needs
  SC_SPLITS = 3, SC_ELEMENTS = 4,             // the query tiers' statistics
  SC_SLOW0 = 5,                               // pairs handed over by join level 0
  SC_BIG_A = 6, SC_WORK0 = 7, SC_BIG_B = 8,   // queries handed on by the first / the middle tier; level 0's work counter
  SC_WORK1 = 9, SC_SLOW1 = 10, SC_SLOW2 = 11, SC_WORK2 = 12,
  SC_INDEX_MISSING = 15,                      // MHAP_DEBUG_INDEX: postings the self-check did not find
  SC_LAST_TIER = SC_BIG_B, SC_LAST_JOIN = SC_SLOW2 + OJ_GROUP_BAD   // (the last word a tier's / a join pass's read-back needs)
};
constexpr size_t counter_bytes(int last_word) { return (size_t)(last_word + 1) * 8; }

struct Switches {
  // sketch_staged, once per call
  long long batch_bases = 0;       // MHAP_BATCH_BASES=n > 0: bases per launch group (else by the free memory)
  bool fused_hash = true;          // MHAP_FUSED_HASH=0: every strand MHAP_RD_MAT
  // sketch_staged, at every launch group
  bool no_length_order = false;    // MHAP_NO_LENGTH_ORDER (set): reads in input order whatever their lengths
  int minhash_wgs_per_cu = 0;      // MHAP_MINHASH_WGS_PER_CU=1..8 (else 0: what the kernel's budget gives)
  int ordered_first = 0;           // MHAP_ORDERED_FIRST=1|2: all of the ordered kernel first / and an idle gap behind it
  int ordered_split = -1;          // MHAP_ORDERED_SPLIT=p: per cent of the strands in the first part (above 100: 100; unset: the rule)
  bool ordered_nowait = true;      // MHAP_ORDERED_NOWAIT=0: the weighted strands' MinHash launch waits for the first part
  int w1_prefill = 0;              // MHAP_W1_PREFILL=n: n fills of the queue buffer in front of the MinHash launch
  bool no_eager_index = false;     // MHAP_NO_EAGER_INDEX (set): the first search builds the index
  // search_core, once per call
  bool bruteforce = false;         // MHAP_CANDIDATES=bruteforce
  bool query_list_host = false;    // MHAP_QUERY_LIST_HOST (set)
  bool count_own = false;          // MHAP_COUNT_OWN (set)
  bool query_chunk_set = false;    // MHAP_QUERY_CHUNK (set, whatever it says: the chunk is then never shrunk)
  long long query_chunk = 262144;  // MHAP_QUERY_CHUNK=n >= CAND_TQ, rounded down to a multiple of it (below: ignored)
  long long overlap_blocks = 0;    // MHAP_OVERLAP_BLOCKS=n > 0 (else 16 per CU)
  bool lane_only = false;          // MHAP_OVERLAP=lane
  int join_wide = 2;               // MHAP_JOIN_WIDE=0|1: further passes of the join kernel (first character only; anything else: both)
  int join_mode = 0;               // MHAP_JOIN_MODE=alone|pair|team: 1, 2, 3 (anything else 0: by the candidates per query)
  bool pipeline = true;            // MHAP_SEARCH_PIPELINE=0: the tail of every chunk inline
  bool first_tier_only = false;    // MHAP_INDEX_TIERS=1
  bool index_dense = false;        // MHAP_INDEX_DENSE=1
  int index_mid = -1;              // MHAP_INDEX_MID=1|other: with / without the middle tier (unset -1: by the index size)
  int overlap_prune = -1;          // MHAP_OVERLAP_PRUNE=1|other: on / off (unset -1: by the candidates per query)
  // one each
  bool debug_index = false;        // MHAP_DEBUG_INDEX (set), ensure_inverted_index
  bool no_triangular = false;      // MHAP_NO_TRIANGULAR (set), self_search

  static int num(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
  static bool first_is(const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; }
  static bool equals(const char* name, const char* v) { const char* e = getenv(name); return e && strcmp(e, v) == 0; }
  static int tristate(const char* name) { const char* e = getenv(name); return e ? (e[0] == '1' ? 1 : 0) : -1; }

  void read_index_build() { debug_index = getenv("MHAP_DEBUG_INDEX") != nullptr; }
  void read_self_search() { no_triangular = getenv("MHAP_NO_TRIANGULAR") != nullptr; }
  void read_sketch_call() {
    if (const char* e = getenv("MHAP_BATCH_BASES")) batch_bases = atoll(e);
    if (const char* e = getenv("MHAP_FUSED_HASH")) fused_hash = atoi(e) != 0;
  }
  void read_sketch_group() {
    no_length_order = getenv("MHAP_NO_LENGTH_ORDER") != nullptr;
    const int w = num("MHAP_MINHASH_WGS_PER_CU", 0);
    minhash_wgs_per_cu = w >= 1 && w <= 8 ? w : 0;
    ordered_first = num("MHAP_ORDERED_FIRST", 0);
    ordered_split = std::min(100, num("MHAP_ORDERED_SPLIT", -1));
    ordered_nowait = num("MHAP_ORDERED_NOWAIT", 1) != 0;
    w1_prefill = num("MHAP_W1_PREFILL", 0);
    no_eager_index = getenv("MHAP_NO_EAGER_INDEX") != nullptr;
  }
  void read_search() {
    bruteforce = equals("MHAP_CANDIDATES", "bruteforce");
    query_list_host = getenv("MHAP_QUERY_LIST_HOST") != nullptr;
    count_own = getenv("MHAP_COUNT_OWN") != nullptr;
    if (const char* e = getenv("MHAP_QUERY_CHUNK")) { query_chunk_set = true; const long long v = atoll(e); if (v >= CAND_TQ) query_chunk = (v / CAND_TQ) * CAND_TQ; }
    if (const char* e = getenv("MHAP_OVERLAP_BLOCKS")) overlap_blocks = atoll(e);
    lane_only = equals("MHAP_OVERLAP", "lane");
    join_wide = first_is("MHAP_JOIN_WIDE", '0') ? 0 : (first_is("MHAP_JOIN_WIDE", '1') ? 1 : 2);
    join_mode = equals("MHAP_JOIN_MODE", "alone") ? 1 : (equals("MHAP_JOIN_MODE", "pair") ? 2 : (equals("MHAP_JOIN_MODE", "team") ? 3 : 0));
    pipeline = !first_is("MHAP_SEARCH_PIPELINE", '0');
    first_tier_only = first_is("MHAP_INDEX_TIERS", '1');
    index_dense = first_is("MHAP_INDEX_DENSE", '1');
    index_mid = tristate("MHAP_INDEX_MID");
    overlap_prune = tristate("MHAP_OVERLAP_PRUNE");
  }
};

}  // namespace mhap
