// vote_common.hpp — the device side of the pile-up votes, written once for read correction (correct_kernels.hip), the unitig consensus
// (consensus_kernels.hip) and the variant sites (variant_kernels.hip): a view's item, the walk over the columns of its path, which casts
// the votes, and the vote kernel over it; the workgroup scan of the lengths a call emits; the decision of the call for one position and
// the qualities of the bytes it emits.  What a vote weighs is a compile-time policy (UnitWeight here, the weighted two in
// weighted_vote.hpp); the host side of a table is vote_table.hpp.
// The contract is the "read correction" section of include/mhap_hip.h; correct_kernels.hip describes the table's planes and the walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/mhap_hip.h"
#include "device_common.hpp"

namespace mhap {

constexpr uint32_t OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8;   // BAM's codes (realign_kernels.hip)
constexpr uint32_t RUN_MAX = (1u << 28) - 1;   // the longest run of a path: a longer one is split into several of its code
constexpr int CK_WORDS = 12;         // words per position: 24 counters of 16 bits
constexpr int CK_KI = 4;              // inserted bytes voted on per junction
constexpr uint32_t CK_CAP = 65535;    // accepted views per target
constexpr int CK_T = 256;             // threads of the call kernel

// one accepted view of one record
struct VoteItem {
  int64_t a_off, b_off;     // first stored byte of read A, of read B
  int64_t v_words;          // first word of the target's planes
  int64_t ops_off;          // the record's runs in the uploaded ops
  int32_t alen, blen;
  int32_t i0, j0;           // first row of s1, first column of s2 (in the aligner's orientation)
  int32_t n_ops;
  int32_t view;             // 0: target A; 1: target B
  int32_t rc;               // s2 is the reverse complement of read B
  int32_t pad;
};

// The check of every add that takes records with their paths: the runs ops[o0, o1) of record r are a path from (a1, j0) to (a2, j1),
// '=' at both ends, and no two adjacent runs have one code unless the earlier is a run split at 2^28 - 1 columns (the walk takes the
// second for the continuation of the first).  i0, j0: the path's first row and column; false with what the refusal says of the record.
inline bool path_spells_record(const mhap_record& r, const std::vector<uint32_t>& ops, int64_t o0, int64_t o1, int64_t& i0, int64_t& j0,
                               std::string& what) {
  const bool rc = r.to_rc != 0;
  i0 = r.a1; j0 = rc ? (int64_t)r.blen - r.b2 - 1 : r.b1;
  const int64_t j1 = rc ? (int64_t)r.blen - r.b1 - 1 : r.b2;
  int64_t rows = 0, cols = 0;
  bool ok = o1 - o0 <= INT32_MAX && (ops[(size_t)o0] & 15u) == OP_EQ && (ops[(size_t)o1 - 1] & 15u) == OP_EQ;
  for (int64_t u = o0; u < o1 && ok; u++) {
    const uint32_t op = ops[(size_t)u], code = op & 15u;
    const int64_t len = op >> 4;
    if (len < 1 || (code != OP_EQ && code != OP_X && code != OP_I && code != OP_D)) ok = false;
    if (code != OP_D) rows += len;
    if (code != OP_I) cols += len;
  }
  ok = ok && i0 >= 0 && j0 >= 0 && r.a2 < r.alen && j1 < r.blen && rows == (int64_t)r.a2 - i0 + 1 && cols == j1 - j0 + 1;
  if (!ok) { what = "has runs that are not a path between its aligned ends"; return false; }
  for (int64_t u = o0 + 1; u < o1; u++) {
    const uint32_t prev = ops[(size_t)u - 1];
    if ((prev & 15u) == (ops[(size_t)u] & 15u) && (prev >> 4) != RUN_MAX) {
      what = "has runs " + std::to_string(u - 1 - o0) + " and " + std::to_string(u - o0) + " of one code, and the earlier is not a run split at 2^28 - 1 columns";
      return false;
    }
  }
  return true;
}

__device__ inline int base_code(uint32_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// What a vote weighs, as a compile-time policy of the walk, the decision and the kernels: weigh(at) is the weight of the byte stored
// at index `at` of the bases, `neutral` the weight of a vote that has no byte (Del, span) and with it the unit U every comparison of
// the call is written in.  The unit policy is the unweighted contract: every vote 1, nothing loaded.  weighted_vote.hpp has the two of
// the "quality-weighted votes".
struct UnitWeight {
  static constexpr int neutral = 1;
  __device__ int operator()(int64_t) const { return 1; }
};

__device__ inline void vote(uint32_t* __restrict__ table, int64_t v_words, int tlen, int t, int counter, uint32_t w) {
  if ((unsigned)t >= (unsigned)tlen) return;   // (add validated the path: never taken)
  atomicAdd(table + v_words + (int64_t)(counter >> 1) * tlen + t, (counter & 1) ? w << 16 : w);
}

struct NoColumn { __device__ void operator()(bool, int, int) const {} };

// The column walk of one view: every column of the path `it` names casts its vote.  One wave; the caller is a kernel of 64 threads.
// The walk is written once, so its switches are compile-time: INS false leaves the insertion slots out (a table of three planes,
// "variant sites"), VOTE false casts no vote at all, each(diag, i, j) is called for every column by every lane that has one (diag:
// it is an '=' or 'X' column; lane 0 has a column whenever any lane has), which is what the variant judgement hangs its ballots on,
// and weigh is the weight policy: an evidence byte votes with weigh(the index it is stored at), Del and span with Weigh::neutral.
// The defaults are the walk as the unweighted correction and consensus use it.
template <bool VOTE = true, bool INS = true, class Each = NoColumn, class Weigh = UnitWeight>
__device__ inline void vote_walk(const uint8_t* __restrict__ bases, const VoteItem& it, const uint32_t* __restrict__ ops,
                                 uint32_t* __restrict__ table, Each each = Each(), Weigh weigh = Weigh()) {
  __shared__ int s_col[65], s_i[64], s_j[64];
  __shared__ uint32_t s_op[64];
  const int lane = threadIdx.x;
  const uint32_t* runs = ops + it.ops_off;
  const bool target_b = it.view != 0, rev = target_b && it.rc != 0;
  const int tlen = target_b ? it.blen : it.alen;
  int ci = it.i0, cj = it.j0;   // (i, j) of the first column of the chunk's first run
  for (int r0 = 0; r0 < it.n_ops; r0 += 64) {
    const int idx = r0 + lane;
    const uint32_t op = idx < it.n_ops ? runs[idx] : 0u;
    const int len = (int)(op >> 4);
    const uint32_t code = op & 15u;
    const int di = (code == OP_EQ || code == OP_X || code == OP_I) ? len : 0;
    const int dj = (code == OP_EQ || code == OP_X || code == OP_D) ? len : 0;
    int si = di, sj = dj, sc = len;   // inclusive scans over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ui = __shfl_up(si, d), uj = __shfl_up(sj, d), uc = __shfl_up(sc, d);
      if (lane >= d) { si += ui; sj += uj; sc += uc; }
    }
    __syncthreads();   // the previous chunk's columns are done with the arrays
    s_op[lane] = op; s_i[lane] = ci + si - di; s_j[lane] = cj + sj - dj; s_col[lane] = sc - len;
    if (lane == 63) s_col[64] = sc;
    __syncthreads();
    ci += __shfl(si, 63); cj += __shfl(sj, 63);
    const int total = s_col[64];
    for (int x = lane; x < total; x += 64) {
      int lo = 0, hi = 63;   // the last run of the chunk that starts at or before column x (runs of length 0 are padding at the end)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_col[mid] <= x) lo = mid; else hi = mid - 1;
      }
      // (several runs cannot start at one column except the padding, which starts at `total` > x)
      const uint32_t rop = s_op[lo];
      const int rlen = (int)(rop >> 4), c = x - s_col[lo], ridx = r0 + lo;
      const uint32_t rcode = rop & 15u;
      const bool diag = rcode == OP_EQ || rcode == OP_X;
      const int i = s_i[lo] + ((diag || rcode == OP_I) ? c : 0), j = s_j[lo] + ((diag || rcode == OP_D) ? c : 0);
      const bool consumes_target = diag || rcode == (target_b ? OP_D : OP_I);
      each(diag, i, j);
      if (!VOTE) continue;
      // The stored index of the column's evidence byte; its quality, where there is one, lies at the same index.  The byte is
      // complemented whenever the record is to_rc: view A reads s2 = rc(B), and view B is turned round.
      const int64_t at = target_b ? it.a_off + i : it.b_off + (it.rc ? it.blen - 1 - j : j);
      if (consumes_target) {
        const int t = !target_b ? i : rev ? it.blen - 1 - j : j;
        if (diag) {
          uint32_t e = bases[at];
          const uint32_t wt = (uint32_t)weigh(at);
          if (it.rc) e = rc_char(e);
          const int b = base_code(e);
          if (b >= 0) vote(table, it.v_words, tlen, t, b, wt);
        } else {
          vote(table, it.v_words, tlen, t, 4, Weigh::neutral);
        }
        // the view continues past t unless this is its last column: the path's last, or its first in the reversed view
        const bool view_end = rev ? (ridx == 0 && c == 0) : (ridx == it.n_ops - 1 && c == rlen - 1);
        if (!view_end) vote(table, it.v_words, tlen, t, 5, Weigh::neutral);
      } else if (INS) {
        // an Ins column: the group is this run (a run split at 2^28 - 1 columns continues a group whose first four slots are taken)
        const int k = rev ? rlen - 1 - c : c;
        if (k < CK_KI) {
          const int nb = rev ? ridx + 1 : ridx - 1;
          const bool split = nb >= 0 && nb < it.n_ops && (runs[nb] & 15u) == rcode;
          if (!split) {
            // the target position before the group in the view's order: the row / column consumed last, or next in the reversed view
            const int t = !target_b ? s_i[lo] - 1 : rev ? it.blen - 1 - s_j[lo] : s_j[lo] - 1;
            uint32_t e = bases[at];
            const uint32_t wt = (uint32_t)weigh(at);
            if (it.rc) e = rc_char(e);
            const int b = base_code(e);
            if (b >= 0) vote(table, it.v_words, tlen, t, 6 + 4 * k + b, wt);
          }
        }
      }
    }
  }
}

namespace {

// The vote kernel of the correction, the consensus and the variant sites: one wave per accepted view.
template <bool INS, class Weigh>
__global__ __launch_bounds__(64) void vote_kernel(const uint8_t* __restrict__ bases, const VoteItem* __restrict__ items,
                                                  const uint32_t* __restrict__ ops, uint32_t* __restrict__ table, Weigh weigh) {
  const VoteItem it = items[blockIdx.x];
  vote_walk<true, INS>(bases, it, ops, table, NoColumn(), weigh);
}

}  // namespace

// What every thread of a call kernel knows of the lengths the workgroup's CK_T threads emit: incl, the inclusive scan up to the
// thread within its wave; before, the sum of the waves in front of it; tile, the sum of all.  The thread's first byte lies at
// before + incl - n of the tile.  Two barriers; the first also says that every thread is done with the previous scan.
struct EmitScan { int incl, before, tile; };

__device__ inline EmitScan scan_emitted(int n) {
  __shared__ int wave_sum[CK_T / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  EmitScan s{n, 0, 0};
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(s.incl, d);
    if (lane >= d) s.incl += u;
  }
  __syncthreads();   // wave_sum of the previous tile has been read
  if (lane == 63) wave_sum[wave] = s.incl;
  __syncthreads();
  for (int u = 0; u < CK_T / 64; u++) { if (u < wave) s.before += wave_sum[u]; s.tile += wave_sum[u]; }
  return s;
}

// the decision for one position: the bytes it emits (at most 1 + CK_KI) and what it counts
struct Decision { int n; uint8_t bytes[1 + CK_KI]; int sub, del, ins, low; };

// U: the unit the counters are in, 1 or the weighted contract's neutral 2; own_w: the weight of the own byte.  min_cov is in votes.
template <int U>
__device__ inline Decision decide(const uint32_t* __restrict__ w, int64_t len, int64_t t, uint32_t own, int own_w, int min_cov) {
  Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
  const uint32_t w0 = w[t], w1 = w[len + t], w2 = w[2 * len + t];
  int base[4] = {(int)(w0 & 0xFFFFu), (int)(w0 >> 16), (int)(w1 & 0xFFFFu), (int)(w1 >> 16)};
  const int del = (int)(w2 & 0xFFFFu), span = (int)(w2 >> 16);
  const int d = base[0] + base[1] + base[2] + base[3] + del;
  if (d < U * min_cov) {
    D.bytes[D.n++] = (uint8_t)own; D.low = 1;
  } else {
    const int ob = base_code(own);
    if (ob >= 0) base[ob] += own_w;
    const int total = d + own_w;
    if (2 * del > total) D.del = 1;
    else {
      int best = 0;
      for (int b = 1; b < 4; b++) if (base[b] > base[best]) best = b;
      uint32_t out;
      if (base[best] == 0 || (ob >= 0 && base[ob] == base[best])) out = own;
      else out = (0x54474341u >> (8 * best)) & 0xFFu;   // "ACGT"
      D.bytes[D.n++] = (uint8_t)out;
      D.sub = out != own;
    }
  }
  if (t < len - 1 && span >= U * min_cov) {
    for (int k = 0; k < CK_KI; k++) {
      const uint32_t x0 = w[(3 + 2 * k) * len + t], x1 = w[(4 + 2 * k) * len + t];
      const int v[4] = {(int)(x0 & 0xFFFFu), (int)(x0 >> 16), (int)(x1 & 0xFFFFu), (int)(x1 >> 16)};
      int best = 0;
      for (int b = 1; b < 4; b++) if (v[b] > v[best]) best = b;
      if (2 * v[best] <= span + U) break;
      D.bytes[D.n++] = (uint8_t)((0x54474341u >> (8 * best)) & 0xFFu);
      D.ins += 1;
    }
  }
  return D;
}

// Base qualities ("base qualities" in include/mhap_hip.h): one byte 0 .. cap per byte of D = decide<U>(w, len, t, own, own_w, min_cov),
// from the same counters, in integers.  Q(m) = min(cap, per_vote * max(m, 0) / (10 U)) of the margin m, in units of U, between the
// votes for the byte and the rest.
constexpr int QUAL_BINS = 94;   // Phred 0 .. 93, what FASTQ can print

// the check of both quality entry points: per_vote 1 .. 1000, cap 1 .. 93
inline bool quality_params_ok(int per_vote, int cap, const char* who, std::string& err) {
  if (per_vote >= 1 && per_vote <= 1000 && cap >= 1 && cap < QUAL_BINS) return true;
  err = std::string(who) + ": per_vote must be 1 .. 1000 and cap 1 .. 93 (" + std::to_string(per_vote) + ", " + std::to_string(cap) + ")";
  return false;
}

template <int U>
__device__ inline int quality_of(int m, int per_vote, int cap) {
  if (m <= 0) return 0;
  const int64_t q = (int64_t)per_vote * m / (10 * U);
  return q < cap ? (int)q : cap;
}

template <int U>
__device__ inline void decide_quality(const uint32_t* __restrict__ w, int64_t len, int64_t t, uint32_t own, int own_w, const Decision& D,
                                      int per_vote, int cap, uint8_t* __restrict__ q) {
  if (D.n == 0) return;   // a called deletion without an insertion: no byte, no quality
  const uint32_t w0 = w[t], w1 = w[len + t], w2 = w[2 * len + t];
  const int base[4] = {(int)(w0 & 0xFFFFu), (int)(w0 >> 16), (int)(w1 & 0xFFFFu), (int)(w1 >> 16)};
  const int del = (int)(w2 & 0xFFFFu), span = (int)(w2 >> 16);
  const int n_base = D.n - D.ins;   // 1 unless the position is called deleted
  int m_last = 0;
  bool fixed = false;               // the last byte is not A, C, G or T: its 0 stands
  if (n_base) {
    const int e = base_code(D.bytes[0]);
    if (e < 0) fixed = true;
    else m_last = 2 * (base[e] + (own == D.bytes[0] ? own_w : 0)) - (base[0] + base[1] + base[2] + base[3] + del + own_w);
    q[0] = (uint8_t)(fixed ? 0 : quality_of<U>(m_last, per_vote, cap));
  }
  for (int k = 0; k < D.ins; k++) {
    const int e = base_code(D.bytes[n_base + k]);   // (decide emits A, C, G or T here)
    const uint32_t x = w[(3 + 2 * k + (e >> 1)) * len + t];
    m_last = 2 * (int)((e & 1) ? x >> 16 : x & 0xFFFFu) - (span + U);
    fixed = false;
    q[n_base + k] = (uint8_t)quality_of<U>(m_last, per_vote, cap);
  }
  // the last byte also answers for the junction not going on
  if (t < len - 1 && D.ins < CK_KI && !fixed) {
    const uint32_t x0 = w[(3 + 2 * D.ins) * len + t], x1 = w[(4 + 2 * D.ins) * len + t];
    int top = (int)(x0 & 0xFFFFu);
    if ((int)(x0 >> 16) > top) top = (int)(x0 >> 16);
    if ((int)(x1 & 0xFFFFu) > top) top = (int)(x1 & 0xFFFFu);
    if ((int)(x1 >> 16) > top) top = (int)(x1 >> 16);
    const int m_stop = span + U - 2 * top;
    if (m_stop < m_last) q[D.n - 1] = (uint8_t)quality_of<U>(m_stop, per_vote, cap);
  }
}

}  // namespace mhap
