// hpc_common.hpp — the rules of "homopolymer compression" (include/mhap_hip.h) that host and device share, and the host's planning
// of a compression, written once and without a HIP call: lo / hi of a read's map and a record's expansion through two maps
// (expand_kernel and mhap_hpc_expand_record), the groups of whole reads and the table of tiles (mhap_hpc_compress).  A host compiler
// without HIP takes this file as it is (tools/hpc_host_check.cpp runs it under the sanitizers).
#pragma once
#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HPC_HD __host__ __device__
#else
#define HPC_HD
#endif

#include "../../include/mhap_hip.h"

namespace mhap {

// start: the clen + 1 entries of a read's map, start[clen] = L
HPC_HD inline int32_t hpc_lo(const int32_t* start, int32_t clen, int32_t p) { return p < 0 ? -1 : p < clen ? start[p] : start[clen]; }
HPC_HD inline int32_t hpc_hi(const int32_t* start, int32_t clen, int32_t p) { return p < 0 ? -1 : p < clen ? start[p + 1] - 1 : start[clen]; }

// the six fields of a record that the expansion rewrites
struct HpcEnds { int32_t a1, a2, alen, b1, b2, blen; };
HPC_HD inline HpcEnds hpc_expand(int32_t a1, int32_t a2, int32_t b1, int32_t b2, const int32_t* start_from, int32_t clen_from,
                                 const int32_t* start_to, int32_t clen_to) {
  return HpcEnds{hpc_lo(start_from, clen_from, a1), hpc_hi(start_from, clen_from, a2), start_from[clen_from],
                 hpc_lo(start_to, clen_to, b1),     hpc_hi(start_to, clen_to, b2),     start_to[clen_to]};
}

constexpr int64_t HPC_GROUP_DEFAULT = (int64_t)1 << 28, HPC_GROUP_MAX = (int64_t)1 << 30;

// Reads [r0, r1) of the table, `bases` raw bases and `tiles` tiles in all; tile0: the first of them in the table of tiles.
struct HpcGroup { int64_t r0, r1, bases, tile0, tiles; };

inline int64_t hpc_tiles_of(int32_t length) { return ((int64_t)length + MHAP_HPC_TILE - 1) / MHAP_HPC_TILE; }

// Whole reads in table order, a group closed in front of the read that would take it past `cap` raw bases; a read longer than the cap
// is a group of its own.  Lengths are >= 0 (the caller has checked).  Every read is in exactly one group, empty ones included.
inline std::vector<HpcGroup> hpc_plan_groups(const int32_t* lengths, int64_t n, int64_t cap) {
  std::vector<HpcGroup> groups;
  HpcGroup g{0, 0, 0, 0, 0};
  for (int64_t r = 0; r < n; r++) {
    if (g.r1 > g.r0 && g.bases + lengths[r] > cap) {
      groups.push_back(g);
      g = HpcGroup{r, r, 0, g.tile0 + g.tiles, 0};
    }
    g.r1 = r + 1;
    g.bases += lengths[r];
    g.tiles += hpc_tiles_of(lengths[r]);
  }
  if (g.r1 > g.r0) groups.push_back(g);
  return groups;
}

// A tile as the kernels read it, one 16-byte word: where its first byte lies in the bases, its first position in its read, the read's length.
struct HpcTile { int64_t addr; int32_t pos, len; };
static_assert(sizeof(HpcTile) == 16, "a tile is one 16-byte word");

// The table of tiles: tile_first[r] = the first tile of read r (n + 1 entries, the last one the number of tiles), tile_read[t] = the
// read of tile t, tiles[t] its place; tile t covers positions [(t - tile_first[r]) * TILE, ...) of its read.  An empty read has no
// tile.  False when the tiles, and a scan block behind them, do not fit an int32.
inline bool hpc_build_tiles(const int64_t* offsets, const int32_t* lengths, int64_t n, std::vector<int32_t>& tile_first, std::vector<int32_t>& tile_read,
                            std::vector<HpcTile>& tiles) {
  int64_t total = 0;
  for (int64_t r = 0; r < n; r++) total += hpc_tiles_of(lengths[r]);
  if (total > INT32_MAX - MHAP_HPC_SCAN_BLOCK) return false;
  tile_first.resize((size_t)n + 1);
  tile_read.resize((size_t)total);
  tiles.resize((size_t)total);
  int64_t t = 0;
  for (int64_t r = 0; r < n; r++) {
    tile_first[(size_t)r] = (int32_t)t;
    for (int64_t k = 0, nk = hpc_tiles_of(lengths[r]); k < nk; k++, t++) {
      tile_read[(size_t)t] = (int32_t)r;
      tiles[(size_t)t] = HpcTile{offsets[r] + k * MHAP_HPC_TILE, (int32_t)(k * MHAP_HPC_TILE), lengths[r]};
    }
  }
  tile_first[(size_t)n] = (int32_t)t;
  return true;
}

}  // namespace mhap
