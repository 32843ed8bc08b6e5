// weighted_vote.hpp — vote_common.hpp's walk, decision and qualities under the "quality-weighted votes" contract of include/mhap_hip.h:
// an evidence byte votes with the weight of its own Phred value, Del and span with the neutral 2, and every comparison of the call is
// the unweighted one in doubled units.  Code of its own next to vote_walk / decide / decide_quality, which stay what they are; the
// table, its planes, the item and the chunked walk are theirs (correct_kernels.hip describes them).
#pragma once
#include "vote_common.hpp"

namespace mhap {

constexpr int W_NEUTRAL = 2;
constexpr uint32_t WK_CAP = CK_CAP / 3;   // accepted views per target: a view adds at most 3 to a counter

struct Weights { int q_lo, q_hi; };

inline bool weight_params_ok(int q_lo, int q_hi, const char* who, std::string& err) {
  if (q_lo >= 0 && q_lo <= q_hi && q_hi < QUAL_BINS) return true;
  err = std::string(who) + ": the weights need 0 <= q_lo <= q_hi <= 93 (" + std::to_string(q_lo) + ", " + std::to_string(q_hi) + ")";
  return false;
}

__device__ inline int weight_of(uint32_t q, Weights W) { return 1 + ((int)q >= W.q_lo ? 1 : 0) + ((int)q >= W.q_hi ? 1 : 0); }

__device__ inline void vote_w(uint32_t* __restrict__ table, int64_t v_words, int tlen, int t, int counter, uint32_t w) {
  if ((unsigned)t >= (unsigned)tlen) return;   // (add validated the path: never taken)
  atomicAdd(table + v_words + (int64_t)(counter >> 1) * tlen + t, (counter & 1) ? w << 16 : w);
}

// vote_walk with weights.  The evidence byte's quality is loaded at the index the byte itself is loaded from, right behind it; the
// staging in LDS and the one pass over the chunk's columns are vote_walk's.
__device__ inline void vote_walk_weighted(const uint8_t* __restrict__ bases, const uint8_t* __restrict__ quals, Weights W, const VoteItem& it,
                                          const uint32_t* __restrict__ ops, uint32_t* __restrict__ table) {
  __shared__ int s_col[65], s_i[64], s_j[64];
  __shared__ uint32_t s_op[64];
  const int lane = threadIdx.x;
  const uint32_t* runs = ops + it.ops_off;
  const bool target_b = it.view != 0, rev = target_b && it.rc != 0;
  const int tlen = target_b ? it.blen : it.alen;
  int ci = it.i0, cj = it.j0;
  for (int r0 = 0; r0 < it.n_ops; r0 += 64) {
    const int idx = r0 + lane;
    const uint32_t op = idx < it.n_ops ? runs[idx] : 0u;
    const int len = (int)(op >> 4);
    const uint32_t code = op & 15u;
    const int di = (code == OP_EQ || code == OP_X || code == OP_I) ? len : 0;
    const int dj = (code == OP_EQ || code == OP_X || code == OP_D) ? len : 0;
    int si = di, sj = dj, sc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ui = __shfl_up(si, d), uj = __shfl_up(sj, d), uc = __shfl_up(sc, d);
      if (lane >= d) { si += ui; sj += uj; sc += uc; }
    }
    __syncthreads();
    s_op[lane] = op; s_i[lane] = ci + si - di; s_j[lane] = cj + sj - dj; s_col[lane] = sc - len;
    if (lane == 63) s_col[64] = sc;
    __syncthreads();
    ci += __shfl(si, 63); cj += __shfl(sj, 63);
    const int total = s_col[64];
    for (int x = lane; x < total; x += 64) {
      int lo = 0, hi = 63;
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_col[mid] <= x) lo = mid; else hi = mid - 1;
      }
      const uint32_t rop = s_op[lo];
      const int rlen = (int)(rop >> 4), c = x - s_col[lo], ridx = r0 + lo;
      const uint32_t rcode = rop & 15u;
      const bool diag = rcode == OP_EQ || rcode == OP_X;
      const int i = s_i[lo] + ((diag || rcode == OP_I) ? c : 0), j = s_j[lo] + ((diag || rcode == OP_D) ? c : 0);
      const bool consumes_target = diag || rcode == (target_b ? OP_D : OP_I);
      // the stored position of the column's evidence byte: complementing changes the byte, not where its quality lies
      const int64_t at = target_b ? it.a_off + i : it.b_off + (it.rc ? it.blen - 1 - j : j);
      if (consumes_target) {
        const int t = !target_b ? i : rev ? it.blen - 1 - j : j;
        if (diag) {
          uint32_t e = bases[at];
          const uint32_t q = quals[at];
          if (it.rc) e = rc_char(e);   // view A of a to_rc record reads s2 = rc(B); its view B is turned round: complemented either way
          const int b = base_code(e);
          if (b >= 0) vote_w(table, it.v_words, tlen, t, b, (uint32_t)weight_of(q, W));
        } else {
          vote_w(table, it.v_words, tlen, t, 4, W_NEUTRAL);
        }
        const bool view_end = rev ? (ridx == 0 && c == 0) : (ridx == it.n_ops - 1 && c == rlen - 1);
        if (!view_end) vote_w(table, it.v_words, tlen, t, 5, W_NEUTRAL);
      } else {
        const int k = rev ? rlen - 1 - c : c;
        if (k < CK_KI) {
          const int nb = rev ? ridx + 1 : ridx - 1;
          const bool split = nb >= 0 && nb < it.n_ops && (runs[nb] & 15u) == rcode;
          if (!split) {
            const int t = !target_b ? s_i[lo] - 1 : rev ? it.blen - 1 - s_j[lo] : s_j[lo] - 1;
            uint32_t e = bases[at];
            const uint32_t q = quals[at];
            if (it.rc) e = rc_char(e);
            const int b = base_code(e);
            if (b >= 0) vote_w(table, it.v_words, tlen, t, 6 + 4 * k + b, (uint32_t)weight_of(q, W));
          }
        }
      }
    }
  }
}

// decide() in weighted units; own_w: the weight of the own byte (the neutral 2 for a draft byte)
__device__ inline Decision decide_weighted(const uint32_t* __restrict__ w, int64_t len, int64_t t, uint32_t own, int own_w, int min_cov) {
  Decision D{0, {0, 0, 0, 0, 0}, 0, 0, 0, 0};
  const uint32_t w0 = w[t], w1 = w[len + t], w2 = w[2 * len + t];
  int base[4] = {(int)(w0 & 0xFFFFu), (int)(w0 >> 16), (int)(w1 & 0xFFFFu), (int)(w1 >> 16)};
  const int del = (int)(w2 & 0xFFFFu), span = (int)(w2 >> 16);
  const int d = base[0] + base[1] + base[2] + base[3] + del;
  if (d < W_NEUTRAL * min_cov) {
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
  if (t < len - 1 && span >= W_NEUTRAL * min_cov) {
    for (int k = 0; k < CK_KI; k++) {
      const uint32_t x0 = w[(3 + 2 * k) * len + t], x1 = w[(4 + 2 * k) * len + t];
      const int v[4] = {(int)(x0 & 0xFFFFu), (int)(x0 >> 16), (int)(x1 & 0xFFFFu), (int)(x1 >> 16)};
      int best = 0;
      for (int b = 1; b < 4; b++) if (v[b] > v[best]) best = b;
      if (2 * v[best] <= span + W_NEUTRAL) break;
      D.bytes[D.n++] = (uint8_t)((0x54474341u >> (8 * best)) & 0xFFu);
      D.ins += 1;
    }
  }
  return D;
}

// Q of a margin in weighted units: the unweighted Q of half of it
__device__ inline int quality_of_weighted(int m, int per_vote, int cap) {
  if (m <= 0) return 0;
  const int64_t q = (int64_t)per_vote * m / 20;
  return q < cap ? (int)q : cap;
}

// decide_quality() in weighted units, for D = decide_weighted(w, len, t, own, own_w, min_cov)
__device__ inline void decide_quality_weighted(const uint32_t* __restrict__ w, int64_t len, int64_t t, uint32_t own, int own_w, const Decision& D,
                                               int per_vote, int cap, uint8_t* __restrict__ q) {
  if (D.n == 0) return;
  const uint32_t w0 = w[t], w1 = w[len + t], w2 = w[2 * len + t];
  const int base[4] = {(int)(w0 & 0xFFFFu), (int)(w0 >> 16), (int)(w1 & 0xFFFFu), (int)(w1 >> 16)};
  const int del = (int)(w2 & 0xFFFFu), span = (int)(w2 >> 16);
  const int n_base = D.n - D.ins;
  int m_last = 0;
  bool fixed = false;
  if (n_base) {
    const int e = base_code(D.bytes[0]);
    if (e < 0) fixed = true;
    else m_last = 2 * (base[e] + (own == D.bytes[0] ? own_w : 0)) - (base[0] + base[1] + base[2] + base[3] + del + own_w);
    q[0] = (uint8_t)(fixed ? 0 : quality_of_weighted(m_last, per_vote, cap));
  }
  for (int k = 0; k < D.ins; k++) {
    const int e = base_code(D.bytes[n_base + k]);
    const uint32_t x = w[(3 + 2 * k + (e >> 1)) * len + t];
    m_last = 2 * (int)((e & 1) ? x >> 16 : x & 0xFFFFu) - (span + W_NEUTRAL);
    fixed = false;
    q[n_base + k] = (uint8_t)quality_of_weighted(m_last, per_vote, cap);
  }
  if (t < len - 1 && D.ins < CK_KI && !fixed) {
    const uint32_t x0 = w[(3 + 2 * D.ins) * len + t], x1 = w[(4 + 2 * D.ins) * len + t];
    int top = (int)(x0 & 0xFFFFu);
    if ((int)(x0 >> 16) > top) top = (int)(x0 >> 16);
    if ((int)(x1 & 0xFFFFu) > top) top = (int)(x1 & 0xFFFFu);
    if ((int)(x1 >> 16) > top) top = (int)(x1 >> 16);
    const int m_stop = span + W_NEUTRAL - 2 * top;
    if (m_stop < m_last) q[D.n - 1] = (uint8_t)quality_of_weighted(m_stop, per_vote, cap);
  }
}

}  // namespace mhap
