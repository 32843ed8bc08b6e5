// realign_kernels.hip — the realignment stage: banded local alignment of reported overlaps on the GPU (mhap_align_pairs_banded), the
// alignments' paths as run-length CIGAR operations (mhap_align_pairs_banded_paths) and the host code that turns overlap records into
// banded pairs and back (mhap_realign_plan, mhap_realign_records, mhap_realign_records_paths).
//
// The contract is mhap_align_pairs' (include/mhap_hip.h) with one sentence added: a cell (i, j) outside the band |j - i - diag| <= band
// has H = 0 and E = F = -inf and carries nothing.  tests/align_banded_ref.py restates it on the CPU.
//
// Geometry.  The band is clipped to the matrix first: the diagonals d = j - i it keeps are [dlo, dlo + W), W <= 2 band + 1, and the rows
// that own an in-band cell are [ilo, ihi].  Nothing outside is touched, so a band that covers the matrix costs what the matrix costs
// and a band that misses it costs nothing.
//
// Schedule (the cell rule, the chain between lanes, the work claim and the launch path are align_common.hpp's; BandWalk below is this
// paragraph as code, for both kernels that walk a band).  As in align_kernels.hip, lane t owns a strip of R consecutive rows of s1 (R cells per step, in registers), walks along s2
// one column per step and hands the bottom row of its strip (H, F and their carried values) to lane t + 1: __shfl_up inside a wave,
// a double-buffered LDS slot between waves.  What changes is which columns a lane walks.  The band moves one column per row, so the
// columns of lane t's strip are those of lane t - 1's shifted right by R: with row0 the first row of the strip, lane t walks the
// W + R columns  cl0 = row0 + dlo - 1, ..., row0 + R - 1 + dlo + W - 1  (local index q = 0 .. W + R - 1; column cl0 itself holds no
// in-band cell of the strip, it is walked to pick up H(row0 - 1, cl0), the diagonal predecessor of the strip's first cell).  Lane
// t needs lane t - 1's bottom row at the same column one step earlier, and that column is lane t - 1's local index q + R, so lane t
// runs its index q at step s = q + t (R + 1): every lane starts R + 1 steps after the one above — R because the band moved, 1 because
// the chain advances — and at step s lane t is at column j = (pass row base + dlo - 1) + s - t.  Inside a row the E dependency
// (i, j - 1) -> (i, j) is the lane's own previous step; the F dependency (i, j) -> (i + 1, j) is the next register of the strip, or
// the lane below one step later.  For q >= W the cell above the strip is right of the band and the lane takes the boundary (H 0,
// F -inf) instead of its neighbour's registers; a cell of the strip's W + R columns that is outside the band (the two triangles of
// R (R + 1) / 2 cells at the ends of a strip) or outside the matrix is masked to the boundary, not computed into anything.
// A pass of L lanes therefore takes (L - 1)(R + 1) + W + R steps for L R rows, of which every lane works W + R: lanes idle
// (L - 1)(R + 1) steps each, which is why a batch with enough pairs to fill the device runs one wave per pair (L = 64: 567 idle steps
// next to W + R, and no barrier) and only a batch too small for that spreads a pair over four waves.
//
// Passes.  Rows beyond one pass's L R go to further passes.  The bottom row of a pass goes to HBM as 10 words per in-band column — W
// entries, indexed by the column's position in the band — and is the top boundary of the next pass: what crosses between passes is
// sized by 2 band + 1, not by the length of s2.
//
// Paths (mhap_align_pairs_banded_paths, mhap_realign_records_paths).  The kernel above already follows one path per pair — the header
// fixes the end cell, the predecessor preference and extension over opening — and reports its begin cell, columns and errors.  The path
// itself comes from two more kernels over the pairs that have an alignment, after the results are on the host:
//  * where the path lies: rows [read_begin, read_end], columns [ref_begin, ref_end], and, with I = columns - columns of s2 covered
//    insertions and D = columns - rows covered deletions on it, the I + D + 1 diagonals [-I, D] around its begin cell's (cut to the
//    pair's band).  Restricting the matrix to that changes no choice on the path: every value on the path is reached through cells on
//    the path, so it keeps its value, and every other value can only fall — the alternative a choice was preferred over stays
//    unpreferred in H (diagonal, then E, then F), and in E and F an extension that won still wins, an opening that won strictly still
//    wins.  The diagonal predecessor of the begin cell is outside the restriction, H = 0 as it was.
//  * trace_fill_kernel runs the same wavefront schedule over that sub-matrix without the carried fields (69 / 81 VGPRs instead of 165)
//    and stores 4 bits per cell: H's choice (diagonal on equal bytes, diagonal on different bytes, E, F), "E extended", "F extended".
//    Word (x, g) holds diagonal x of the 8 rows of row group g, so a lane's strip is one g; the pair's words are [x][g].
//  * trace_walk_kernel, one lane per pair, walks back from the end cell for exactly `columns` columns, one word serving up to 8 diagonal
//    steps, and writes the runs backwards from the end of a slice of 2 errors + 1 entries (no path has more runs); the host cuts the
//    slices down to the runs.  A walk that does not end in front of the begin cell is an error of the call, never a shorter path.
// Pairs go through in groups whose trace fits TRACE_BUDGET (2 GiB) or MHAP_REALIGN_TRACE_BYTES; a pair beyond it goes alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "align_common.hpp"
#include "device_common.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

// The band clipped to the m x n matrix: diagonals [dlo, dlo + W) and rows [ilo, ilo + rows).  W = 0: no cell is in the band.
struct BandGeom { int dlo, W, ilo, rows; };
__host__ __device__ inline BandGeom band_geom(int64_t m, int64_t n, int64_t diag, int64_t band) {
  const int64_t lim = (int64_t)1 << 40;          // beyond any matrix: keeps diag +- band inside int64
  diag = diag < -lim ? -lim : diag > lim ? lim : diag;
  band = band > lim ? lim : band;
  const int64_t lo = diag - band > -(m - 1) ? diag - band : -(m - 1), hi = diag + band < n - 1 ? diag + band : n - 1;
  if (m <= 0 || n <= 0 || band < 0 || hi < lo) return BandGeom{0, 0, 0, 0};
  const int64_t ilo = -hi > 0 ? -hi : 0, ihi = n - 1 - lo < m - 1 ? n - 1 - lo : m - 1;   // rows with a column j = i + d in [0, n)
  return BandGeom{(int)lo, (int)(hi - lo + 1), (int)ilo, (int)(ihi - ilo + 1)};
}

// Lanes and passes of a band of `rows` rows in a workgroup of T lanes: as few passes as T lanes allow, then as few lanes as that many
// passes need; rows past the last are masked.  No rows: no pass.
__host__ __device__ inline void band_shape(int rows, int T, int& passes, int& L) {
  passes = (rows + T * AL_R - 1) / (T * AL_R);
  L = passes > 0 ? (rows + passes * AL_R - 1) / (passes * AL_R) : 1;
}

// The schedule above for one lane: where lane t of L is in a pass and at a step of it.  align_banded_kernel and trace_fill_kernel take
// every bound, index and band test from here, so they cannot walk different cells.
struct BandWalk {
  int W, n, L, t;                        // the band's diagonals, the columns of s2, the lanes of a pass, this lane
  int pbase, row0, jc, s_begin, s_end;   // a pass: its first row, the lane's first row, the column before lane 0's first, the steps with work
  int q, j;                              // a step: the lane's local column index and its column of s2
  bool inq, active;                      // q is one of the lane's W + R columns; and j is a column of s2

  // Pass p of a band whose rows begin at ilo and whose diagonals begin at dlo.  Steps before lane 0 reaches column 0 and after the
  // last lane has left its columns or s2 (and `extra` steps more) have no active lane.
  __device__ __forceinline__ void pass(int ilo, int dlo, int p, int extra) {
    pbase = ilo + p * L * AL_R; row0 = pbase + t * AL_R; jc = pbase + dlo - 1;
    s_begin = jc < 0 ? -jc : 0;
    s_end = min((L - 1) * (AL_R + 1) + W + AL_R, n - jc + L - 1 + extra);
  }
  // lane t at step s: local column q = s - t (R + 1), column j = jc + s - t
  __device__ __forceinline__ void step(int s) {
    q = s - t * (AL_R + 1); j = jc + s - t;
    inq = t < L && q >= 0 && q < W + AL_R;
    active = inq && j >= 0 && j < n;
  }
  // the cell above the strip at this column is the boundary: right of the band for q >= W, above the band's first row for lane 0 of
  // pass 0 (lane 0 of a later pass reads the previous pass's bottom row at position q)
  __device__ __forceinline__ bool above_is_boundary(int p) const { return q >= W || (t == 0 && p == 0); }
  // row r of the strip (its byte c1) has a cell of the band at this column: its in-band columns are the local indices r + 1 .. r + W
  __device__ __forceinline__ bool inband(uint32_t c1, int r) const { return c1 != AL_PAD && (unsigned)(q - 1 - r) < (unsigned)W; }
  // the strip's bottom row is in the band at local indices R .. R + W - 1: position q - R of the W the next pass reads
  __device__ __forceinline__ bool hands_down(int p, int passes) const { return t == L - 1 && p + 1 < passes && q >= AL_R; }
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void align_banded_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ pairs,
                                                               const int32_t* __restrict__ order, int n_order, int* __restrict__ next,
                                                               int32_t* __restrict__ scratch, int64_t scratch_stride,
                                                               int32_t* __restrict__ results) {
  constexpr int T = NW * 64;
  __shared__ Edge hand[2][NW > 1 ? NW - 1 : 1];
  const int t = threadIdx.x;
  int32_t* edge = scratch ? scratch + (int64_t)blockIdx.x * scratch_stride : nullptr;
  for (;;) {
    const int k = claim_next(next);
    if (k >= n_order) return;
    const int pi = order[k];
    const int64_t* pr = pairs + 7 * (int64_t)pi;
    const int64_t a_off = pr[0], b_off = pr[2];
    const int m = (int)pr[1], n = (int)pr[3];
    const bool b_rc = pr[4] != 0;
    const BandGeom g = band_geom(m, n, pr[5], pr[6]);
    const int ihi = g.ilo + g.rows - 1;
    BandWalk w;
    w.W = g.W; w.n = n; w.t = t;
    int passes;
    band_shape(g.rows, T, passes, w.L);
    BestEnd lane_best{0, 0, 0, {0, 0, 0, 0}};   // this lane's best end cell over all passes
    for (int p = 0; p < passes; p++) {
      Strip S;
      S.reset();
      w.pass(g.ilo, g.dlo, p, 0);
#pragma unroll
      for (int r = 0; r < AL_R; r++) {
        const int i = w.row0 + r;
        S.c1[r] = (t < w.L && i <= ihi) ? (uint32_t)bases[a_off + i] : AL_PAD;
      }
      for (int s = w.s_begin; s < w.s_end; s++) {
        w.step(s);
        Edge in = edge_from_above<NW>(S.out, hand, s);
        if (w.active) {
          if (w.above_is_boundary(p)) in = edge_boundary();
          else if (t == 0) in = edge_load(edge + w.q, w.W);
          const uint32_t c2 = b_rc ? rc_char(bases[b_off + (n - 1 - w.j)]) : (uint32_t)bases[b_off + w.j];
          S.column(in, c2, w.row0, w.j, [&](uint32_t c1, int r) { return w.inband(c1, r); });
          if (w.hands_down(p, passes)) edge_store(edge + (w.q - AL_R), w.W, S.out);
        } else {
          S.dH = 0;   // the diagonal predecessor of a lane's first column is left of the band or of the matrix
        }
        edge_to_below<NW>(S.out, hand, s);
      }
      if (better_end(S.best, lane_best)) lane_best = S.best;
      __syncthreads();   // the pass's bottom row (HBM) before the next pass reads it
    }
    write_best_end<T>(lane_best, results + 7 * (int64_t)pi);
  }
}

constexpr int64_t BA_SCRATCH_BUDGET = (int64_t)1 << 30;   // bytes of pass boundaries in flight; fewer workgroups beyond that

// The wide form's share of n items whose band has rows(q) rows and W(q) diagonals, and their order.  An item with more rows than one
// wave holds goes to the four-wave kernel only while such items are too few to give every compute unit its waves; with more of them a
// wave per item idles less (the header comment) and needs no barrier.  w_big, w_small: the widest band of each form that needs a
// second pass, which is what a workgroup keeps in HBM between passes.
template <class Rows, class Width>
std::vector<int32_t> band_order(const HandleView& v, int64_t n, Rows rows, Width W, size_t& n_big, int64_t& w_big, int64_t& w_small) {
  int64_t n_tall = 0;
  for (int64_t q = 0; q < n; q++) n_tall += rows(q) > 64 * AL_R;
  const bool spread = n_tall < 4LL * v.num_cus;
  std::vector<int32_t> order = longest_first(
      n, [&](int64_t q) { return spread && rows(q) > 64 * AL_R; }, [&](int64_t q) { return (double)rows(q) * (double)W(q); }, n_big);
  w_big = w_small = 0;
  for (size_t u = 0; u < order.size(); u++) {
    const int32_t q = order[u];
    if (rows(q) > (u < n_big ? AL_NWB : 1) * 64 * AL_R) (u < n_big ? w_big : w_small) = std::max<int64_t>(u < n_big ? w_big : w_small, W(q));
  }
  return order;
}

// `pairs` (host, validated) against the bases already in B.bases; everything on v.stream, results on the host when it returns.
int banded_run(const HandleView& v, AlignBufs& B, const int64_t* pairs, int64_t n, int32_t* results, const char* who) {
  std::vector<BandGeom> geo((size_t)n);
  for (int64_t q = 0; q < n; q++) geo[(size_t)q] = band_geom(pairs[7 * q + 1], pairs[7 * q + 3], pairs[7 * q + 5], pairs[7 * q + 6]);
  size_t n_big;
  int64_t w_big, w_small;
  const std::vector<int32_t> order = band_order(v, n, [&](int64_t q) { return geo[(size_t)q].rows; }, [&](int64_t q) { return geo[(size_t)q].W; },
                                                n_big, w_big, w_small);
  // HBM rows between passes: 10 words per diagonal, one set per workgroup; 2 and 8 workgroups per compute unit are two waves per SIMD
  const FormShape big{grid_size(n_big, 2, v, 10 * w_big, BA_SCRATCH_BUDGET / 2), 10 * w_big};
  const FormShape small{grid_size((size_t)n - n_big, 8, v, 10 * w_small, BA_SCRATCH_BUDGET / 2), 10 * w_small};
  hipError_t e;
  if ((e = B.results.ensure(28 * n)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
  const int rc = launch_forms(v, who, B, align_banded_kernel<AL_NWB>, align_banded_kernel<1>, pairs, 56, order, n_big, big, small, B.results.as<int32_t>());
  return rc != MHAP_OK ? rc : download_results(v, who, B, results, n);
}

// ---- paths: the alignment itself, as run-length operations -----------------------------------------------------------------------------
// (the file header, "Paths", is the design)

constexpr uint32_t OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8;   // BAM's codes
constexpr uint32_t OP_MAXLEN = (1u << 28) - 1;                // a longer run is split
constexpr int64_t TRACE_BUDGET = (int64_t)2 << 30;            // bytes of direction nibbles in flight; MHAP_REALIGN_TRACE_BYTES overrides

// The sub-matrix of one pair that has an alignment: rows [read_begin, read_end] of s1, columns [ref_begin, ref_end] of s2 and the
// diagonals the path can have visited.  i, j, d below are relative to its first cell.
struct TracePair {
  int64_t a_off, b_off;        // first byte of the rows' bases; first STORED byte of the columns' bases (their last when rc)
  int64_t trace_off, ops_off;  // the pair's words in the trace buffer, its slice of the ops buffer
  int32_t m, n, rc;
  int32_t dlo, W, ilo, rows;   // diagonals [dlo, dlo + W), rows [ilo, ilo + rows) with a cell on one of them
  int32_t G;                   // row groups of 8: passes x lanes of the kernel that fills the trace
  int32_t cols, ops_cap;       // columns of the path; entries of the ops slice (2 errors + 1, and one per split)
};

// the diagonals [lo, hi] clipped to the m x n matrix (band_geom without the centre and half-width)
inline BandGeom diag_geom(int64_t m, int64_t n, int64_t lo, int64_t hi) {
  lo = std::max<int64_t>(lo, -(m - 1)); hi = std::min<int64_t>(hi, n - 1);
  if (m <= 0 || n <= 0 || hi < lo) return BandGeom{0, 0, 0, 0};
  const int64_t ilo = -hi > 0 ? -hi : 0, ihi = n - 1 - lo < m - 1 ? n - 1 - lo : m - 1;
  return BandGeom{(int)lo, (int)(hi - lo + 1), (int)ilo, (int)(ihi - ilo + 1)};
}

// align_banded_kernel's schedule over a TracePair, carrying no path fields and keeping no best cell: what it leaves is one nibble per
// in-band cell — bits 0-1 H's choice (0 diagonal on equal bytes, 1 diagonal on different bytes, 2 E, 3 F; the choice of a cell with
// H = 0 is never read, a walk ends by its column count), bit 2 "E extended", bit 3 "F extended".  Word (x, g) of a pair holds diagonal
// dlo + x of the 8 rows ilo + 8 g ...: a lane's strip is one g, its 8 cells of one step lie on 8 diagonals, so a lane keeps the 8 words
// in flight in registers (acc[k]: diagonal index q - 1 - k), completes one per step and stores it whole.
template <int NW>
__global__ __launch_bounds__(NW * 64) void trace_fill_kernel(const uint8_t* __restrict__ bases, const TracePair* __restrict__ tps,
                                                             const int32_t* __restrict__ order, int n_order, int* __restrict__ next,
                                                             int32_t* __restrict__ scratch, int64_t scratch_stride,
                                                             uint32_t* __restrict__ trace) {
  constexpr int T = NW * 64;
  __shared__ EdgeHF hand[2][NW > 1 ? NW - 1 : 1];
  const int t = threadIdx.x;
  int32_t* edge = scratch ? scratch + (int64_t)blockIdx.x * scratch_stride : nullptr;   // H, then F, of the W entries between passes
  for (;;) {
    const int k = claim_next(next);
    if (k >= n_order) return;
    const TracePair tp = tps[order[k]];
    const int n = tp.n, W = tp.W, ihi = tp.ilo + tp.rows - 1;
    const bool b_rc = tp.rc != 0;
    BandWalk w;
    w.W = W; w.n = n; w.t = t;
    int passes;
    band_shape(tp.rows, T, passes, w.L);
    const int64_t G = (int64_t)passes * w.L;
    uint32_t* tr = trace + tp.trace_off;
    for (int p = 0; p < passes; p++) {
      uint32_t c1[AL_R], acc[AL_R];
      int Hp[AL_R], Ep[AL_R];
      // AL_R steps more than align_banded_kernel takes at the right edge of s2: the words in flight there still have to come out
      w.pass(tp.ilo, tp.dlo, p, AL_R);
#pragma unroll
      for (int r = 0; r < AL_R; r++) {
        const int i = w.row0 + r;
        c1[r] = (t < w.L && i <= ihi) ? (uint32_t)bases[tp.a_off + i] : AL_PAD;
        Hp[r] = 0; Ep[r] = AL_NEG; acc[r] = 0;
      }
      int dH = 0;
      EdgeHF out{0, AL_NEG};
      for (int s = w.s_begin; s < w.s_end; s++) {
        w.step(s);
        EdgeHF in = edge_from_above<NW>(out, hand, s);
        if (w.active) {
          if (w.above_is_boundary(p)) in = EdgeHF{0, AL_NEG};
          else if (t == 0) in = EdgeHF{edge[w.q], edge[W + w.q]};
          const uint32_t c2 = b_rc ? rc_char(bases[tp.b_off + (n - 1 - w.j)]) : (uint32_t)bases[tp.b_off + w.j];
          int upH = in.H, upF = in.F, diagH = dH;
#pragma unroll
          for (int r = 0; r < AL_R; r++) {
            const bool mis = c1[r] != c2;
            Cell c = cell_rule(diagH, Hp[r], Ep[r], upH, upF, mis);
            const uint32_t nib = (c.take_d ? (mis ? 1u : 0u) : c.take_e ? 2u : 3u) | (c.ext ? 4u : 0u) | (c.fx ? 8u : 0u);
            if (w.inband(c1[r], r)) acc[r] |= nib << (4 * r);
            else { c.H = 0; c.E = AL_NEG; c.F = AL_NEG; }
            diagH = Hp[r];
            Hp[r] = c.H; Ep[r] = c.E;
            upH = c.H; upF = c.F;
          }
          dH = in.H;
          out = EdgeHF{upH, upF};
          if (w.hands_down(p, passes)) { edge[w.q - AL_R] = out.H; edge[W + w.q - AL_R] = out.F; }
        } else {
          dH = 0;
        }
        if (w.inq) {   // diagonal index q - AL_R has had its 8 rows (those outside the matrix or the band stay 0)
          if (w.q >= AL_R) tr[(int64_t)(w.q - AL_R) * G + (p * w.L + t)] = acc[AL_R - 1];
#pragma unroll
          for (int r = AL_R - 1; r > 0; r--) acc[r] = acc[r - 1];
          acc[0] = 0;
        }
        edge_to_below<NW>(out, hand, s);
      }
      __syncthreads();
    }
  }
}

// One lane per pair walks its nibbles from the end cell for exactly `cols` columns and writes the runs backwards from the end of the
// pair's slice, so that they stand in path order at the slice's tail.  A word serves up to 8 diagonal steps; it is fetched again only
// when the walk leaves its 8 rows or its diagonal.  n_ops[q]: the runs written, or -1 when the walk left the sub-matrix, overran its
// slice or did not end in front of the begin cell — the trace and the first pass disagree, which the host reports as an error.
__global__ __launch_bounds__(64) void trace_walk_kernel(const TracePair* __restrict__ tps, int n_pairs, const uint32_t* __restrict__ trace,
                                                        uint32_t* __restrict__ ops, int32_t* __restrict__ n_ops) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= n_pairs) return;
  const TracePair tp = tps[q];
  const uint32_t* tr = trace + tp.trace_off;
  uint32_t* slice = ops + tp.ops_off;
  int pos = tp.ops_cap, i = tp.m - 1, j = tp.n - 1, st = 0, left = tp.cols;   // st: 0 in H, 1 in E, 2 in F
  int64_t have = -1;
  uint32_t word = 0, code = 0, len = 0;
  bool ok = true;
  for (int64_t guard = 2 * (int64_t)tp.cols + 2; left > 0 && guard > 0; guard--) {
    const int x = j - i - tp.dlo, ri = i - tp.ilo;
    if (i < 0 || j < 0 || (unsigned)x >= (unsigned)tp.W || (unsigned)ri >= (unsigned)tp.rows) { ok = false; break; }
    const int64_t idx = (int64_t)x * tp.G + (ri >> 3);
    if (idx != have) { word = tr[idx]; have = idx; }
    const uint32_t nib = (word >> (4 * (ri & 7))) & 15u;
    uint32_t c;
    if (st == 0) {
      const uint32_t hc = nib & 3u;
      if (hc >= 2u) { st = (int)hc - 1; continue; }
      c = hc == 0u ? OP_EQ : OP_X; i--; j--;
    } else if (st == 1) { c = OP_D; j--; st = (nib & 4u) ? 1 : 0; }
    else { c = OP_I; i--; st = (nib & 8u) ? 2 : 0; }
    left--;
    if (c == code && len < OP_MAXLEN) len++;
    else {
      if (len) { if (pos == 0) { ok = false; break; } slice[--pos] = len << 4 | code; }
      code = c; len = 1;
    }
  }
  if (ok && len) { if (pos == 0) ok = false; else slice[--pos] = len << 4 | code; }
  ok = ok && left == 0 && i == -1 && j == -1 && st == 0;
  n_ops[q] = ok ? tp.ops_cap - pos : -1;
}

int64_t trace_budget() {
  if (const char* e = getenv("MHAP_REALIGN_TRACE_BYTES")) {
    char* end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && *end == '\0' && v >= 1) return (int64_t)v;
  }
  return TRACE_BUDGET;
}

// The paths of `pairs` (validated, their bases in B.bases) whose `results` banded_run has just returned, appended to `out`.  q0: the
// index of pairs[0] in the caller's numbering, for messages.
int paths_run(const HandleView& v, AlignBufs& B, const int64_t* pairs, int64_t n, const int32_t* results, int64_t q0,
              mhap_align_paths& out, const char* who) {
  // the sub-matrix of every pair that has an alignment.  With I = columns - (ref_end - ref_begin + 1) insertions and D = columns -
  // (read_end - read_begin + 1) deletions on the path, the path stays on the diagonals [-I, D] around its begin cell's.
  std::vector<TracePair> tps;
  std::vector<int64_t> owner;       // index into pairs
  std::vector<int64_t> est_words;   // trace words, an upper bound over both kernel forms
  for (int64_t q = 0; q < n; q++) {
    const int64_t* p = pairs + 7 * q;
    const int32_t* a = results + 7 * q;
    if (a[0] <= 0 || a[5] <= 0) continue;
    TracePair tp{};
    tp.m = a[2] - a[1] + 1; tp.n = a[4] - a[3] + 1; tp.rc = p[4] != 0;
    tp.a_off = p[0] + a[1];
    tp.b_off = tp.rc ? p[2] + (p[3] - 1 - a[4]) : p[2] + a[3];
    const BandGeom g = band_geom(p[1], p[3], p[5], p[6]);
    const int64_t d0 = (int64_t)a[3] - a[1], ins = (int64_t)a[5] - tp.n, del = (int64_t)a[5] - tp.m;
    const BandGeom s = diag_geom(tp.m, tp.n, std::max<int64_t>(-ins, g.dlo - d0), std::min<int64_t>(del, (int64_t)g.dlo + g.W - 1 - d0));
    tp.dlo = s.dlo; tp.W = s.W; tp.ilo = s.ilo; tp.rows = s.rows;
    tp.cols = a[5];
    tp.ops_cap = (int32_t)std::min<int64_t>(2 * (int64_t)a[6] + 1 + a[5] / OP_MAXLEN, a[5]);
    if (s.W <= 0 || ins < 0 || del < 0) { *v.err = std::string(who) + ": internal error: pair " + std::to_string(q0 + q) + " has an alignment outside its band"; return MHAP_E_HIP; }
    tps.push_back(tp);
    owner.push_back(q);
    est_words.push_back((int64_t)s.W * ((s.rows + AL_R - 1) / AL_R + (s.rows + 64 * AL_R - 1) / (64 * AL_R)));
  }
  const int64_t budget = trace_budget();
  const size_t first_offset = out.offsets.size();   // offsets[first_offset + q] = end of pair q's runs
  out.offsets.resize(first_offset + (size_t)n, out.offsets.back());
  std::vector<int32_t> counts;
  std::vector<uint32_t> slices;
  std::vector<std::vector<uint32_t>> runs((size_t)n);   // per pair, until the offsets are known (groups finish in pair order)
  hipError_t e;
  for (size_t g0 = 0; g0 < tps.size();) {
    // a group: pairs in order while their trace fits the budget; a pair beyond the budget goes alone
    size_t g1 = g0;
    int64_t bytes = 0;
    while (g1 < tps.size() && (g1 == g0 || bytes + 4 * est_words[g1] <= budget) && g1 - g0 < ((size_t)1 << 20)) bytes += 4 * est_words[g1++];
    const int64_t ng = (int64_t)(g1 - g0);
    size_t n_big;
    int64_t w_big, w_small;
    const std::vector<int32_t> order = band_order(v, ng, [&](int64_t u) { return tps[g0 + (size_t)u].rows; }, [&](int64_t u) { return tps[g0 + (size_t)u].W; },
                                                  n_big, w_big, w_small);   // banded_run's rule
    std::vector<char> wide((size_t)ng, 0);
    for (size_t u = 0; u < n_big; u++) wide[(size_t)order[u]] = 1;
    int64_t words = 0, n_slices = 0;
    for (size_t u = g0; u < g1; u++) {
      TracePair& tp = tps[u];
      int passes, L;
      band_shape(tp.rows, wide[u - g0] ? AL_NWB * 64 : 64, passes, L);
      tp.G = passes * L;
      tp.trace_off = words; words += (int64_t)tp.W * tp.G;
      tp.ops_off = n_slices; n_slices += tp.ops_cap;
    }
    // 69 and 81 VGPRs: the fill kernels fit twice the workgroups per compute unit of banded_run's; H and F of W entries between passes
    const FormShape big{grid_size(n_big, 4, v), 2 * w_big}, small{grid_size((size_t)ng - n_big, 16, v), 2 * w_small};
    const std::string which = "pair " + std::to_string(q0 + owner[g0]) + (ng > 1 ? " and the " + std::to_string(ng - 1) + " after it" : "");
    if ((e = B.trace.ensure((size_t)std::max<int64_t>(words, 1) * 4)) != hipSuccess)
      return hip_fail(v, who, "hipMalloc of " + std::to_string(words * 4) + " bytes of trace for " + which, e);
    if ((e = B.n_ops.ensure(4 * (size_t)ng)) != hipSuccess) return hip_fail(v, who, "hipMalloc", e);
    if ((e = B.ops.ensure(4 * (size_t)n_slices)) != hipSuccess) return hip_fail(v, who, "hipMalloc of the runs of " + which, e);
    const int rc = launch_forms(v, who, B, trace_fill_kernel<AL_NWB>, trace_fill_kernel<1>, (const TracePair*)tps.data() + g0, sizeof(TracePair), order,
                                n_big, big, small, B.trace.as<uint32_t>());
    if (rc != MHAP_OK) return rc;
    hipLaunchKernelGGL(trace_walk_kernel, dim3((unsigned)((ng + 63) / 64)), dim3(64), 0, v.stream, B.items.as<TracePair>(), (int)ng,
                       B.trace.as<uint32_t>(), B.ops.as<uint32_t>(), B.n_ops.as<int32_t>());
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(v, who, "launch", e);
    counts.resize((size_t)ng);
    slices.resize((size_t)n_slices);
    if ((e = hipMemcpyAsync(counts.data(), B.n_ops.p, 4 * (size_t)ng, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
    if ((e = hipMemcpyAsync(slices.data(), B.ops.p, 4 * (size_t)n_slices, hipMemcpyDeviceToHost, v.stream)) != hipSuccess) return hip_fail(v, who, "download", e);
    if ((e = hipStreamSynchronize(v.stream)) != hipSuccess) return hip_fail(v, who, "kernel", e);
    for (int64_t u = 0; u < ng; u++) {
      const TracePair& tp = tps[g0 + (size_t)u];
      const int32_t c = counts[(size_t)u];
      if (c < 0) {
        *v.err = std::string(who) + ": internal error: the trace of pair " + std::to_string(q0 + owner[g0 + (size_t)u]) + " does not lead back to its begin cell";
        return MHAP_E_HIP;
      }
      const uint32_t* tail = slices.data() + tp.ops_off + (tp.ops_cap - c);
      runs[(size_t)owner[g0 + (size_t)u]].assign(tail, tail + c);
    }
    g0 = g1;
  }
  for (int64_t q = 0; q < n; q++) {
    out.ops.insert(out.ops.end(), runs[(size_t)q].begin(), runs[(size_t)q].end());
    out.offsets[first_offset + (size_t)q] = (int64_t)out.ops.size();
  }
  return MHAP_OK;
}

int check_pairs(const int64_t* pairs, int64_t n, int64_t n_bases, std::string* err, const char* who) {
  for (int64_t q = 0; q < n; q++) {
    const int64_t* p = pairs + 7 * q;
    for (int f = 0; f < 2; f++) {
      const int64_t off = p[2 * f], len = p[2 * f + 1];
      if (off < 0 || len < 0 || len > INT32_MAX / 4 || off > n_bases - len) {
        *err = std::string(who) + ": pair " + std::to_string(q) + " has a segment outside the " + std::to_string(n_bases) + " bases";
        return MHAP_E_INVALID;
      }
    }
    if (p[6] < 0) { *err = std::string(who) + ": pair " + std::to_string(q) + " has a negative band (" + std::to_string(p[6]) + ")"; return MHAP_E_INVALID; }
  }
  return MHAP_OK;
}

inline int64_t floor_div2(int64_t x) { return x >= 0 ? x / 2 : -((-x + 1) / 2); }

// the plan of one record; `map` finds a read by id
int plan_one(const mhap_record& r, int64_t q, const std::unordered_map<int64_t, int64_t>& map, const int64_t* offsets, const int32_t* lengths,
             double max_shift, int32_t band, int64_t* out, std::string* err) {
  int64_t idx[2];
  const int64_t ids[2] = {r.from_id, r.to_id};
  const int32_t lens[2] = {r.alen, r.blen};
  for (int f = 0; f < 2; f++) {
    const auto it = map.find(ids[f]);
    if (it == map.end()) { *err = "mhap_realign_plan: record " + std::to_string(q) + " names read " + std::to_string(ids[f]) + ", which is not among the reads"; return MHAP_E_INVALID; }
    idx[f] = it->second;
    if (lengths[idx[f]] != lens[f]) {
      *err = "mhap_realign_plan: record " + std::to_string(q) + " gives read " + std::to_string(ids[f]) + " the length " + std::to_string(lens[f]) +
             ", the reads say " + std::to_string(lengths[idx[f]]);
      return MHAP_E_INVALID;
    }
  }
  const bool rc = r.to_rc != 0;
  const int64_t b1 = rc ? (int64_t)r.blen - r.b2 - 1 : r.b1, b2 = rc ? (int64_t)r.blen - r.b1 - 1 : r.b2;   // MatchResult's flip undone
  out[0] = offsets[idx[0]]; out[1] = r.alen; out[2] = offsets[idx[1]]; out[3] = r.blen; out[4] = rc ? 1 : 0;
  out[5] = floor_div2((b1 + b2) - ((int64_t)r.a1 + r.a2));
  if (band > 0) out[6] = band;
  else {
    // the tolerance the second stage applies around its median shift (BottomOverlapSketch.java:205)
    const int64_t span = std::max<int64_t>((int64_t)r.a2 - r.a1, b2 - b1);
    const double w = (double)span * max_shift;   // (int) of a double as Java casts it: toward zero, saturating; anything below 1 gives 1
    out[6] = w >= 2147483647.0 ? 2147483647 : w >= 1.0 ? (int64_t)w : 1;
  }
  return MHAP_OK;
}

int build_map(const int64_t* read_ids, int64_t n_reads, std::unordered_map<int64_t, int64_t>& map) {
  map.reserve((size_t)n_reads * 2);
  for (int64_t i = 0; i < n_reads; i++) map.emplace(read_ids[i], i);   // (the first read of an id wins)
  return MHAP_OK;
}

thread_local std::string g_plan_err;

}  // namespace
}  // namespace mhap

using namespace mhap;

namespace {

// mhap_align_pairs_banded, and with `paths` the path of every pair as well (an object the caller then owns)
int align_banded_impl(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t* results,
                      mhap_align_paths** paths, const char* who) {
  if (paths) *paths = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (n < 0 || n_bases < 0 || (n > 0 && (!pairs || !results)) || (n_bases > 0 && !bases)) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 pairs in one call"; return MHAP_E_INVALID; }
  if (n == 0) { if (paths) *paths = new mhap_align_paths(); return MHAP_OK; }
  int rc = check_pairs(pairs, n, n_bases, v.err, who);
  if (rc != MHAP_OK) return rc;
  AlignBufs B;
  mhap_align_paths* out = paths ? new mhap_align_paths() : nullptr;
  rc = upload_bases(v, B, bases, n_bases, who);
  if (rc == MHAP_OK) rc = banded_run(v, B, pairs, n, results, who);
  if (rc == MHAP_OK && out) rc = paths_run(v, B, pairs, n, results, 0, *out, who);
  if (rc != MHAP_OK) delete out;
  else if (paths) *paths = out;
  return rc;
}

}  // namespace

extern "C" int mhap_align_pairs_banded(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n, int32_t* results) {
  return align_banded_impl(h, bases, n_bases, pairs, n, results, nullptr, "mhap_align_pairs_banded");
}

extern "C" int mhap_align_pairs_banded_paths(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* pairs, int64_t n,
                                             int32_t* results, mhap_align_paths** out) {
  if (!out) return MHAP_E_INVALID;
  return align_banded_impl(h, bases, n_bases, pairs, n, results, out, "mhap_align_pairs_banded_paths");
}

extern "C" int mhap_align_paths_info(const mhap_align_paths* p, int64_t* n, int64_t* n_ops) {
  if (!p) return MHAP_E_INVALID;
  if (n) *n = (int64_t)p->offsets.size() - 1;
  if (n_ops) *n_ops = (int64_t)p->ops.size();
  return MHAP_OK;
}

extern "C" int mhap_align_paths_copy(const mhap_align_paths* p, int64_t* op_offsets, uint32_t* ops) {
  if (!p || !op_offsets || (!ops && !p->ops.empty())) return MHAP_E_INVALID;
  std::copy(p->offsets.begin(), p->offsets.end(), op_offsets);
  std::copy(p->ops.begin(), p->ops.end(), ops);
  return MHAP_OK;
}

extern "C" void mhap_align_paths_free(mhap_align_paths* p) { delete p; }

extern "C" int mhap_align_paths_from_runs(const int64_t* op_offsets, int64_t n, const uint32_t* ops, mhap_align_paths** out) {
  if (out) *out = nullptr;
  if (!out || !op_offsets || n < 0 || op_offsets[0] != 0) return MHAP_E_INVALID;
  for (int64_t q = 0; q < n; q++)
    if (op_offsets[q + 1] < op_offsets[q]) return MHAP_E_INVALID;
  if (op_offsets[n] > 0 && !ops) return MHAP_E_INVALID;
  mhap_align_paths* p = new mhap_align_paths();
  p->offsets.assign(op_offsets, op_offsets + n + 1);
  p->ops.assign(ops, ops + op_offsets[n]);
  *out = p;
  return MHAP_OK;
}

extern "C" const char* mhap_realign_plan_error(void) { return g_plan_err.c_str(); }

extern "C" int mhap_realign_plan(const mhap_record* recs, int64_t n, const int64_t* read_ids, const int64_t* offsets, const int32_t* lengths,
                                 int64_t n_reads, double max_shift, int32_t band, int64_t* pairs) {
  g_plan_err.clear();
  if (n < 0 || n_reads < 0 || band < 0 || (n > 0 && (!recs || !pairs)) || (n_reads > 0 && (!read_ids || !offsets || !lengths))) {
    g_plan_err = "mhap_realign_plan: null or negative argument";
    return MHAP_E_INVALID;
  }
  std::unordered_map<int64_t, int64_t> map;
  build_map(read_ids, n_reads, map);
  for (int64_t q = 0; q < n; q++) {
    const int rc = plan_one(recs[q], q, map, offsets, lengths, max_shift, band, pairs + 7 * q, &g_plan_err);
    if (rc != MHAP_OK) return rc;
  }
  return MHAP_OK;
}

namespace {

// mhap_realign_records, and with `paths` the path of every record's planned pair as well (an object the caller then owns)
int realign_impl(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                 const int32_t* lengths, int64_t n_reads, const mhap_record* recs, int64_t n, int32_t band, mhap_record* out,
                 int32_t* detail, mhap_align_paths** paths, const char* who) {
  if (paths) *paths = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (n < 0 || n_bases < 0 || n_reads < 0 || band < 0 || (n > 0 && (!recs || !out)) || (n_bases > 0 && !bases) ||
      (n_reads > 0 && (!read_ids || !offsets || !lengths))) {
    *v.err = std::string(who) + ": null or negative argument";
    return MHAP_E_INVALID;
  }
  if (n == 0) { if (paths) *paths = new mhap_align_paths(); return MHAP_OK; }
  for (int64_t i = 0; i < n_reads; i++)
    if (offsets[i] < 0 || lengths[i] < 0 || offsets[i] > n_bases - lengths[i]) {
      *v.err = std::string(who) + ": read " + std::to_string(i) + " lies outside the " + std::to_string(n_bases) + " bases";
      return MHAP_E_INVALID;
    }
  std::unordered_map<int64_t, int64_t> map;
  build_map(read_ids, n_reads, map);
  // The bases go up once.  Records go through in batches of at most BATCH: 56 + 28 bytes of pairs and results and 4 of work order per
  // record (5.8 MB) on each side, and the pass boundaries of the workgroups in flight (at most BA_SCRATCH_BUDGET, 1 GiB), whatever n is.
  constexpr int64_t BATCH = 1 << 16;
  AlignBufs B;
  mhap_align_paths* po = paths ? new mhap_align_paths() : nullptr;
  int rc = upload_bases(v, B, bases, n_bases, who);
  std::vector<int64_t> pairs((size_t)std::min(n, BATCH) * 7);
  std::vector<int32_t> res((size_t)std::min(n, BATCH) * 7);
  for (int64_t q0 = 0; q0 < n && rc == MHAP_OK; q0 += BATCH) {
    const int64_t c = std::min(BATCH, n - q0);
    for (int64_t q = 0; q < c && rc == MHAP_OK; q++)
      rc = plan_one(recs[q0 + q], q0 + q, map, offsets, lengths, v.max_shift, band, pairs.data() + 7 * q, v.err);
    if (rc != MHAP_OK) break;
    rc = banded_run(v, B, pairs.data(), c, res.data(), who);
    if (rc != MHAP_OK) break;
    if (po && (rc = paths_run(v, B, pairs.data(), c, res.data(), q0, *po, who)) != MHAP_OK) break;
    for (int64_t q = 0; q < c; q++) {
      const mhap_record& r = recs[q0 + q];
      const int32_t* a = res.data() + 7 * q;
      mhap_record o = r;
      o.pad = 0;
      const bool ok = a[0] > 0 && a[5] > 0;
      if (ok) {
        o.a1 = a[1]; o.a2 = a[2];
        o.b1 = r.to_rc ? r.blen - a[4] - 1 : a[3];
        o.b2 = r.to_rc ? r.blen - a[3] - 1 : a[4];
        o.score = 1.0 - (double)a[6] / (double)a[5];
      } else {
        o.a1 = o.a2 = o.b1 = o.b2 = 0; o.score = 0.0;
      }
      out[q0 + q] = o;
      if (detail) { detail[3 * (q0 + q)] = ok ? a[0] : 0; detail[3 * (q0 + q) + 1] = ok ? a[5] : 0; detail[3 * (q0 + q) + 2] = ok ? a[6] : 0; }
    }
  }
  if (rc != MHAP_OK) delete po;
  else if (paths) *paths = po;
  return rc;
}

}  // namespace

extern "C" int mhap_realign_records(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                                    const int32_t* lengths, int64_t n_reads, const mhap_record* recs, int64_t n, int32_t band,
                                    mhap_record* out, int32_t* detail) {
  return realign_impl(h, bases, n_bases, read_ids, offsets, lengths, n_reads, recs, n, band, out, detail, nullptr, "mhap_realign_records");
}

extern "C" int mhap_realign_records_paths(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                                          const int32_t* lengths, int64_t n_reads, const mhap_record* recs, int64_t n, int32_t band,
                                          mhap_record* out, int32_t* detail, mhap_align_paths** paths) {
  if (!paths) return MHAP_E_INVALID;
  return realign_impl(h, bases, n_bases, read_ids, offsets, lengths, n_reads, recs, n, band, out, detail, paths, "mhap_realign_records_paths");
}
