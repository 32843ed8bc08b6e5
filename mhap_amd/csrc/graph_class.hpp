// graph_class.hpp — the class of a realigned record ("string graph" in include/mhap_hip.h), written once: classify_kernel
// (graph_kernels.hip) classes every record of the graph with it, and the placement kernels of the unitig consensus
// (consensus_kernels.hip) ask it which records may place a read.  Also the 32-byte record both keep on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mhap {

enum { G_NONE = 0, G_INTERNAL, G_A_CONTAINED, G_B_CONTAINED, G_SHORT, G_DOVETAIL, G_CLASSES };

// a record as it goes up: the two reads' positions in the table (brc = 2 B + to_rc), the aligned ends, the identity
struct GItem { int32_t a, brc, a1, a2, b1, b2; double score; };
static_assert(sizeof(GItem) == 32, "a record is two 16-byte words");

struct GParams { int32_t max_hang, permille, min_ovlp, fuzz; double min_identity; };

// the aligned intervals of a record in the aligner's frame: A forward over [qs, qe) of ql, B with strand to_rc over [ts, te) of tl
struct GGeom { int32_t qs, qe, ql, ts, te, tl, tl5, tl3, q3; };

// The first rule that holds; g is filled whenever the class is not G_NONE.  ql, tl: the lengths of the two reads.
__host__ __device__ inline int graph_class(int32_t A, int32_t B, int32_t o, int32_t a1, int32_t a2, int32_t b1, int32_t b2, double score,
                                           int32_t ql, int32_t tl, const GParams& P, GGeom& g) {
  if (A == B || score == 0.0 || score < P.min_identity) return G_NONE;
  g.qs = a1; g.qe = a2 + 1; g.ql = ql; g.tl = tl;
  g.ts = o ? tl - b2 - 1 : b1; g.te = o ? tl - b1 : b2 + 1;
  g.tl5 = g.ts; g.tl3 = tl - g.te; g.q3 = ql - g.qe;
  const int32_t ext5 = g.qs < g.tl5 ? g.qs : g.tl5, ext3 = g.q3 < g.tl3 ? g.q3 : g.tl3;
  const int64_t span = (int64_t)g.qe - g.qs, ext = (int64_t)ext5 + ext3;
  if (ext5 > P.max_hang || ext3 > P.max_hang || span * 1000 < (span + ext) * P.permille) return G_INTERNAL;
  if (g.qs <= g.tl5 && g.q3 <= g.tl3) return G_A_CONTAINED;
  if (g.qs >= g.tl5 && g.q3 >= g.tl3) return G_B_CONTAINED;
  if (span + ext < P.min_ovlp || (int64_t)g.te - g.ts + ext < P.min_ovlp) return G_SHORT;
  return G_DOVETAIL;
}

}  // namespace mhap
