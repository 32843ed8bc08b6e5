// hpc_kernels.hip — reads with every run of equal bytes collapsed to one, the map from each compressed position to its raw run, and
// records carried through that map (mhap_hpc_compress / _info / _copy / _times / _expand_records / _free).  The contract — heads, the
// compressed read, start[], lo / hi and the expansion — is the prose of include/mhap_hip.h ("homopolymer compression");
// tests/hpc_ref.py restates it.  The rules host and device share, the groups and the table of tiles are hpc_common.hpp's.
//
// A stream compaction in two passes over tiles of MHAP_HPC_TILE positions, one workgroup of 256 lanes per tile; a read of L bases
// has ceil(L / TILE) tiles of its own, so no tile holds two reads, and the host builds the table of tiles from the read table.
// load:   a lane takes the 16 positions tpos + 16 lane ..  A read begins anywhere, so the lane loads the aligned 16-byte word that
//         holds its first byte, gets the word behind it from the next lane (the last lane of a wave loads that one itself) and
//         shifts the pair by the tile's misalignment, which is one value for the workgroup.  The byte in front of the lane's first
//         comes from the lane before; the first lane of a wave loads it, and never for position 0: the byte in front of a read is
//         not looked at.  head bit j = byte j differs from the byte before it, or the position is 0; positions >= L have no bit.
//         Where a tile lies (address, position, the read's length) is one 16-byte word of the table of tiles, HpcTile: one load in
//         front of the bytes' own, not a chain of four through the read table.
// pass 1: count_kernel adds the lanes' head counts up, one number per tile.
// scan:   scan_kernel, one workgroup of 1024 lanes, turns a group's tile counts into exclusive offsets in place, MHAP_HPC_SCAN_BLOCK
//         at a time with a carry, and leaves the group's total.  The host reads the totals of all groups once, gives every group its
//         place in the output (the only 64-bit numbers of a launch) and sizes the output exactly.
// reads:  reads_kernel, one lane per read: coff and clen from the offsets of the read's first tile and of the tile behind its last;
//         an empty read has no tile, so its one map entry, 0, is written here.
// pass 2: write_kernel loads and flags the tile again, ranks the heads — lane order is position order, so the rank of a lane's first
//         head is the heads of the lanes before it: 16 ballots, one per bit, each masked to the lower lanes and counted, plus the
//         totals of the waves before (LDS) — and puts head bytes and raw positions into LDS at their ranks, the bytes shifted by the
//         output's misalignment.  Then the workgroup writes the positions as consecutive int32 and the bytes as whole aligned words;
//         only the partial words at the two ends of the tile's output go out byte by byte (the neighbours own the rest of them).
//         The last tile of a read writes the sentinel start[clen] = L.  No global atomic in either pass.
// counts: the positions are in LDS, so pass 2 also counts the runs that lie between two heads of its tile and keeps the tile's first
//         and last head; edge_kernel, one lane per tile, ends the run of each tile's last head at the next head of the read, wherever
//         that is, and sums up: the runs longer than 1 and the longest (two atomics per workgroup of 256 tiles).
// expand: one lane per record with hpc_expand; the host resolves ids to rows and puts the six rewritten fields into a copy.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

#include "hpc_common.hpp"
#include "kernels.hpp"
#include "mhap_internal.hpp"

namespace mhap {
namespace {

typedef unsigned long long u64;

enum { HPC_T = HPC_TILE_THREADS, HPC_WAVES = HPC_T / 64, SCAN_T = HPC_SCAN_THREADS, SCAN_PER = 4 };
static_assert(HPC_T * 16 == MHAP_HPC_TILE, "a tile is one 16-byte load per lane");
static_assert(SCAN_T * SCAN_PER == MHAP_HPC_SCAN_BLOCK, "a scan block is four counts per lane");
// counts: reads, raw bases, compressed bases, runs longer than 1, longest run, empty reads
enum { HC_READS = 0, HC_RAW, HC_COMPRESSED, HC_LONG_RUNS, HC_LONGEST, HC_EMPTY };
static_assert(HC_EMPTY + 1 == MHAP_HPC_COUNTS, "the counts of the header");

template <int S>
__device__ inline void shift_words(const uint32_t (&d)[8], int sh, uint32_t (&b)[4]) {
#pragma unroll
  for (int k = 0; k < 4; k++) b[k] = __funnelshift_r(d[k + S], d[k + S + 1], sh);
}

// The lane's 16 bytes of the tile at position tpos of a read of L bytes, the tile's first byte at bases + addr (b, little-endian: byte
// j is position tpos + 16 tid + j), and their head bits.  Every lane of the workgroup calls it.
__device__ inline uint32_t tile_heads(const uint8_t* __restrict__ bases, int64_t addr, int32_t L, int32_t tpos, int tid, int lane, uint32_t (&b)[4]) {
  const int m = (int)(addr & 15);                        // the same for every lane
  const uint8_t* word = bases + (addr - m) + 16 * tid;   // the aligned word with the lane's first byte: positions p0 - m .. p0 - m + 15
  const int32_t p0 = tpos + 16 * tid;
  uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
  if ((int64_t)p0 - m < L) w0 = *(const uint4*)word;     // (the word begins inside the read or up to 15 bytes in front of the tile)
  if (m != 0) {
    w1.x = __shfl_down(w0.x, 1); w1.y = __shfl_down(w0.y, 1); w1.z = __shfl_down(w0.z, 1); w1.w = __shfl_down(w0.w, 1);
    if (lane == 63) {
      w1 = make_uint4(0, 0, 0, 0);
      if ((int64_t)p0 - m + 16 < L) w1 = *(const uint4*)(word + 16);
    }
  }
  const uint32_t d[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  const int sh = (m & 3) * 8;
  switch (m >> 2) {
    case 0: shift_words<0>(d, sh, b); break;
    case 1: shift_words<1>(d, sh, b); break;
    case 2: shift_words<2>(d, sh, b); break;
    default: shift_words<3>(d, sh, b); break;
  }
  uint32_t before = __shfl_up(b[3], 1) >> 24;            // the byte in front of the lane's first
  if (lane == 0 && p0 > 0 && p0 < L) before = bases[addr + 16 * tid - 1];
  uint32_t heads = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = b[k] ^ ((b[k] << 8) | before);
    before = b[k] >> 24;
#pragma unroll
    for (int j = 0; j < 4; j++) heads |= ((x >> (8 * j)) & 0xFFu) != 0 ? 1u << (4 * k + j) : 0u;
  }
  if (p0 == 0) heads |= 1u;
  const int32_t left = L - p0;                           // positions of the lane inside the read
  return left >= 16 ? heads : left > 0 ? heads & ((1u << left) - 1u) : 0u;
}

__global__ __launch_bounds__(HPC_T) void count_kernel(const uint8_t* __restrict__ bases, const HpcTile* __restrict__ tiles, int32_t t0,
                                                      int32_t* __restrict__ tile_out) {
  __shared__ int32_t ws[HPC_WAVES];
  const int32_t t = t0 + (int32_t)blockIdx.x;
  const HpcTile tile = tiles[t];   // (one load in front of the bytes' own: the table of tiles says where they lie)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t b[4];
  int32_t c = __popc(tile_heads(bases, tile.addr, tile.len, tile.pos, tid, lane, b));
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) c += __shfl_down(c, s);
  if (lane == 0) ws[wave] = c;
  __syncthreads();
  if (tid == 0) tile_out[t] = ws[0] + ws[1] + ws[2] + ws[3];
}

// v[0 .. n) becomes its exclusive prefix sums; *total their sum
__global__ __launch_bounds__(SCAN_T) void scan_kernel(int32_t* __restrict__ v, int32_t n, int64_t* __restrict__ total) {
  __shared__ int32_t ws[SCAN_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t carry = 0;
  for (int32_t i0 = 0; i0 < n; i0 += MHAP_HPC_SCAN_BLOCK) {
    const int32_t i = i0 + SCAN_PER * tid;
    int32_t e[SCAN_PER], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++) { e[k] = s; s += i + k < n ? v[i + k] : 0; }
    int32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t u = __shfl_up(inc, d);
      if (lane >= d) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_T / 64; w++) { before += w < wave ? ws[w] : 0; all += ws[w]; }
    const int32_t base = carry + before + inc - s;
#pragma unroll
    for (int k = 0; k < SCAN_PER; k++) if (i + k < n) v[i + k] = base + e[k];
    carry += all;
    __syncthreads();   // (ws is written again by the next block)
  }
  if (tid == 0) *total = carry;
}

// reads r0 .. r0 + nr of a group whose tiles are t0 .. t0 + nt, whose heads number gtotal and whose output begins at cbase
__global__ __launch_bounds__(256) void reads_kernel(const int32_t* __restrict__ tile_first, const int32_t* __restrict__ tile_out,
                                                    const int32_t* __restrict__ lengths, int32_t r0, int32_t nr, int32_t t0, int32_t nt,
                                                    int32_t gtotal, int64_t cbase, int64_t n_reads, int64_t* __restrict__ coff,
                                                    int32_t* __restrict__ clen, int32_t* __restrict__ starts) {
  const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (i >= nr) return;
  const int32_t r = r0 + i, f = tile_first[r], l = tile_first[r + 1];
  const int32_t o0 = f < t0 + nt ? tile_out[f] : gtotal, o1 = l < t0 + nt ? tile_out[l] : gtotal;
  coff[r] = cbase + o0;
  clen[r] = o1 - o0;
  if (lengths[r] == 0) starts[cbase + o0 + r] = 0;
  if (r + 1 == n_reads) coff[r + 1] = cbase + o1;
}

// info[t] = {the tile's first head, its last head (-1: none), the runs longer than 1 that end inside the tile, the longest of those}
__global__ __launch_bounds__(HPC_T) void write_kernel(const uint8_t* __restrict__ bases, const HpcTile* __restrict__ tiles,
                                                      const int32_t* __restrict__ tile_read, const int32_t* __restrict__ tile_out, int32_t t0,
                                                      int64_t cbase, uint8_t* __restrict__ cbases, int32_t* __restrict__ starts,
                                                      int4* __restrict__ info) {
  __shared__ int32_t spos[MHAP_HPC_TILE];
  __shared__ uint32_t swords[MHAP_HPC_TILE / 4 + 1];   // the head bytes, in front of them the (G & 3) bytes that the output's word has before G
  __shared__ int32_t ws[HPC_WAVES], wmany[HPC_WAVES], wlong[HPC_WAVES];
  const int32_t t = t0 + (int32_t)blockIdx.x;
  const HpcTile tile = tiles[t];
  const int32_t r = tile_read[t], out0 = tile_out[t], L = tile.len, tpos = tile.pos;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t b[4];
  const uint32_t heads = tile_heads(bases, tile.addr, L, tpos, tid, lane, b);
  const u64 lower = ((u64)1 << lane) - 1;
  int32_t k = 0, wave_heads = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const u64 bal = __ballot((heads >> j) & 1u);
    k += __popcll(bal & lower);
    wave_heads += __popcll(bal);
  }
  if (lane == 0) ws[wave] = wave_heads;
  __syncthreads();
  int32_t tile_heads_n = 0;
#pragma unroll
  for (int w = 0; w < HPC_WAVES; w++) { k += w < wave ? ws[w] : 0; tile_heads_n += ws[w]; }
  const int64_t G = cbase + out0;   // the tile's first compressed byte; its first map entry is r further on
  const int sh = (int)(G & 3);
  uint8_t* sbytes = (uint8_t*)swords;
  const int32_t p0 = tpos + 16 * tid;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    if ((heads >> j) & 1u) {
      spos[k] = p0 + j;
      sbytes[sh + k] = (uint8_t)(b[j >> 2] >> (8 * (j & 3)));
      k++;
    }
  }
  __syncthreads();
  int32_t* smap = starts + (G + r);
  for (int32_t q = tid; q < tile_heads_n; q += HPC_T) smap[q] = spos[q];
  if (tid == 0 && (int64_t)tpos + MHAP_HPC_TILE >= L) smap[tile_heads_n] = L;
  uint8_t* gbytes = cbases + (G - sh);     // a word boundary of the output: LDS byte q goes to gbytes[q] for q in [sh, sh + heads)
  const int32_t end = sh + tile_heads_n;
  for (int32_t w = tid; 4 * w < end; w += HPC_T) {
    const int32_t q0 = 4 * w;
    if (q0 >= sh && q0 + 4 <= end) { ((uint32_t*)gbytes)[w] = swords[w]; continue; }
    for (int32_t q = q0 < sh ? sh : q0; q < q0 + 4 && q < end; q++) gbytes[q] = sbytes[q];
  }
  // the runs between two heads of this tile; the run of the last head ends in a later tile or with the read (edge_kernel)
  int32_t many = 0, longest = 0;
  for (int32_t q = tid; q + 1 < tile_heads_n; q += HPC_T) {
    const int32_t d = spos[q + 1] - spos[q];
    many += d > 1;
    longest = d > longest ? d : longest;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    many += __shfl_down(many, s);
    const int32_t o = __shfl_down(longest, s);
    longest = o > longest ? o : longest;
  }
  if (lane == 0) { wmany[wave] = many; wlong[wave] = longest; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < HPC_WAVES; w++) { many += wmany[w]; longest = wlong[w] > longest ? wlong[w] : longest; }
  info[t] = tile_heads_n > 0 ? make_int4(spos[0], spos[tile_heads_n - 1], many, longest) : make_int4(-1, -1, 0, 0);
}

// One lane per tile of a group (tiles t0 .. t0 + nt): the run of the tile's last head ends at the first head of a later tile of the
// read, or with the read; the tile's own counts and that run are summed over the workgroup and leave by two atomics, counts[0] += the
// runs longer than 1, counts[1] = max of the longest.  A lane walks over the tiles without a head behind its own, each of which no
// other lane walks over: a read that is one run of many megabases is the slow case (a tile per microsecond or so).
__global__ __launch_bounds__(256) void edge_kernel(const HpcTile* __restrict__ tiles, const int32_t* __restrict__ tile_read,
                                                   const int32_t* __restrict__ tile_first, const int4* __restrict__ info, int32_t t0, int32_t nt,
                                                   u64* __restrict__ counts) {
  __shared__ u64 wl[4], wm[4];
  const int32_t i = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  u64 many = 0, longest = 0;
  if (i < nt) {
    const int32_t t = t0 + i;
    const int4 me = info[t];
    many = (u64)me.z; longest = (u64)me.w;
    if (me.y >= 0) {
      const int32_t tend = tile_first[tile_read[t] + 1];
      int32_t t2 = t + 1, next = -1;
      while (t2 < tend && (next = info[t2].x) < 0) t2++;
      const int32_t d = (t2 < tend ? next : tiles[t].len) - me.y;
      many += d > 1;
      if ((u64)d > longest) longest = (u64)d;
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    many += __shfl_down(many, s);
    const u64 o = __shfl_down(longest, s);
    if (o > longest) longest = o;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wl[wave] = many; wm[wave] = longest; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; w++) { many += wl[w]; if (wm[w] > longest) longest = wm[w]; }
  if (many) atomicAdd(counts, many);
  if (longest) atomicMax(counts + 1, longest);
}

struct XItem { int32_t ra, rb, a1, a2, b1, b2; };
static_assert(sizeof(XItem) == 24, "an expansion item");
// out: two 16-byte words per record, {a1, a2, b1, b2} and {alen, blen, 0, 0}
__global__ __launch_bounds__(256) void expand_kernel(const XItem* __restrict__ items, int64_t n, const int64_t* __restrict__ coff_a,
                                                     const int32_t* __restrict__ clen_a, const int32_t* __restrict__ starts_a,
                                                     const int64_t* __restrict__ coff_b, const int32_t* __restrict__ clen_b,
                                                     const int32_t* __restrict__ starts_b, int4* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const XItem it = items[q];
  const HpcEnds e = hpc_expand(it.a1, it.a2, it.b1, it.b2, starts_a + coff_a[it.ra] + it.ra, clen_a[it.ra], starts_b + coff_b[it.rb] + it.rb,
                               clen_b[it.rb]);
  out[2 * q] = make_int4(e.a1, e.a2, e.b1, e.b2);
  out[2 * q + 1] = make_int4(e.alen, e.blen, 0, 0);
}

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace
}  // namespace mhap

using namespace mhap;

struct mhap_hpc {
  mhap_handle* h = nullptr;
  int device = 0;
  int64_t n = 0, total = 0;
  std::vector<int64_t> ids;
  std::vector<int32_t> raw_len, clen;
  std::unordered_map<int64_t, int32_t> by_id;
  int64_t counts[MHAP_HPC_COUNTS] = {0, 0, 0, 0, 0, 0};
  double ms[4] = {0.0, 0.0, 0.0, 0.0};   // upload, the two passes with the scan and the reads' rows, edge_kernel, the whole call
  DevBuf d_cbases, d_starts, d_coff, d_clen;
  void release() { for (DevBuf* b : {&d_cbases, &d_starts, &d_coff, &d_clen}) b->release(); }
};

namespace {

bool reads_ok(const HandleView& v, const char* who, int64_t n_bases, const int64_t* offsets, const int32_t* lengths, int64_t n) {
  for (int64_t r = 0; r < n; r++) {
    if (lengths[r] < 0 || lengths[r] > INT32_MAX - 8) {
      *v.err = std::string(who) + ": read " + std::to_string(r) + " has a negative length or one above 2^31 - 9";
      return false;
    }
    if (offsets[r] < 0 || offsets[r] > n_bases || lengths[r] > n_bases - offsets[r]) {
      *v.err = std::string(who) + ": read " + std::to_string(r) + " (" + std::to_string(lengths[r]) + " bases at " + std::to_string(offsets[r]) +
               ") does not lie in the " + std::to_string(n_bases) + " bases";
      return false;
    }
  }
  return true;
}

// everything a compression holds besides the object: freed when the call ends, failed or not
struct Scratch {
  DevBuf bases, len, tiles, tile_read, tile_first, tile_out, info, totals, counts;
  hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Scratch() {
    for (DevBuf* b : {&bases, &len, &tiles, &tile_read, &tile_first, &tile_out, &info, &totals, &counts}) b->release();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

template <class T> hipError_t upload(DevBuf& b, const T* src, size_t count, hipStream_t st, size_t pad = 0) {
  hipError_t e = b.ensure(std::max<size_t>(sizeof(T) * count + pad, 16));
  if (e == hipSuccess && count > 0) e = hipMemcpyAsync(b.p, src, sizeof(T) * count, hipMemcpyHostToDevice, st);
  return e;
}

}  // namespace

extern "C" int mhap_hpc_compress(mhap_handle* h, const uint8_t* bases, int64_t n_bases, const int64_t* read_ids, const int64_t* offsets,
                                 const int32_t* lengths, int64_t n_reads, int64_t group_bases, mhap_hpc** out) {
  const char* who = "mhap_hpc_compress";
  if (out) *out = nullptr;
  if (!h) return MHAP_E_INVALID;
  HandleView v = handle_view(h);
  if (!out || n_bases < 0 || n_reads < 0 || (n_bases > 0 && !bases) || (n_reads > 0 && (!read_ids || !offsets || !lengths)) || group_bases < 0) {
    *v.err = std::string(who) + ": null or negative argument";
    return MHAP_E_INVALID;
  }
  if (group_bases > HPC_GROUP_MAX) { *v.err = std::string(who) + ": group_bases above 2^30"; return MHAP_E_INVALID; }
  if (n_reads >= ((int64_t)1 << 30)) { *v.err = std::string(who) + ": 2^30 reads or more"; return MHAP_E_INVALID; }
  if (!reads_ok(v, who, n_bases, offsets, lengths, n_reads)) return MHAP_E_INVALID;
  const double t_begin = wall_ms();
  const std::vector<HpcGroup> groups = hpc_plan_groups(lengths, n_reads, group_bases > 0 ? group_bases : HPC_GROUP_DEFAULT);
  std::vector<int32_t> tile_first, tile_read;
  std::vector<HpcTile> tiles;
  if (!hpc_build_tiles(offsets, lengths, n_reads, tile_first, tile_read, tiles)) { *v.err = std::string(who) + ": 2^31 tiles or more"; return MHAP_E_INVALID; }
  const int64_t n_tiles = (int64_t)tile_read.size(), n_groups = (int64_t)groups.size();

  mhap_hpc* c = new mhap_hpc();
  c->h = h; c->device = v.device; c->n = n_reads;
  c->ids.assign(read_ids, read_ids + n_reads);
  c->raw_len.assign(lengths, lengths + n_reads);
  c->by_id.reserve((size_t)n_reads * 2);
  for (int64_t r = 0; r < n_reads; r++) {
    c->by_id.emplace(read_ids[r], (int32_t)r);   // (the first read of an id wins, as in mhap_realign_plan)
    c->counts[HC_RAW] += lengths[r];
    c->counts[HC_EMPTY] += lengths[r] == 0;
  }
  c->counts[HC_READS] = n_reads;

  (void)hipSetDevice(v.device);
  Scratch s;
  hipStream_t st = v.stream;
  hipError_t e = hipSuccess;
  const char* what = "the events";
  for (hipEvent_t& ev : s.ev) if (e == hipSuccess) e = hipEventCreate(&ev);
  auto mark = [&](int i) { if (e == hipSuccess) e = hipEventRecord(s.ev[i], st); };
  auto fail = [&]() {
    (void)hipStreamSynchronize(st);   // (the uploads read host memory of this call)
    c->release();
    delete c;
    return hip_fail(v, who, what, e);
  };
  mark(0);
  what = "hipMalloc or upload of the reads";
  if (e == hipSuccess) e = upload(s.bases, bases, (size_t)n_bases, st, 32);   // (a lane's aligned words may end up to 31 bytes behind the last read)
  if (e == hipSuccess) e = upload(s.len, lengths, (size_t)n_reads, st);
  if (e == hipSuccess) e = upload(s.tiles, tiles.data(), (size_t)n_tiles, st);
  if (e == hipSuccess) e = upload(s.tile_read, tile_read.data(), (size_t)n_tiles, st);
  if (e == hipSuccess) e = upload(s.tile_first, tile_first.data(), (size_t)n_reads + 1, st);
  if (e == hipSuccess) e = s.tile_out.ensure(4 * (size_t)std::max<int64_t>(n_tiles, 1));
  if (e == hipSuccess) e = s.totals.ensure(8 * (size_t)std::max<int64_t>(n_groups, 1));
  if (e == hipSuccess) e = s.info.ensure(16 * (size_t)std::max<int64_t>(n_tiles, 1));
  if (e == hipSuccess) e = s.counts.ensure(16);
  if (e == hipSuccess) e = hipMemsetAsync(s.totals.p, 0, 8 * (size_t)std::max<int64_t>(n_groups, 1), st);
  if (e == hipSuccess) e = hipMemsetAsync(s.counts.p, 0, 16, st);
  mark(1);
  // pass 1 and the scan, group by group
  what = "pass 1";
  for (int64_t g = 0; g < n_groups && e == hipSuccess; g++) {
    const HpcGroup& G = groups[(size_t)g];
    if (G.tiles == 0) continue;
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)G.tiles), dim3(HPC_T), 0, st, s.bases.as<uint8_t>(), s.tiles.as<HpcTile>(), (int32_t)G.tile0,
                       s.tile_out.as<int32_t>());
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_T), 0, st, s.tile_out.as<int32_t>() + G.tile0, (int32_t)G.tiles, s.totals.as<int64_t>() + g);
    e = hipGetLastError();
  }
  mark(2);
  std::vector<int64_t> totals((size_t)std::max<int64_t>(n_groups, 1), 0);
  if (e == hipSuccess && n_groups > 0) e = hipMemcpyAsync(totals.data(), s.totals.p, 8 * (size_t)n_groups, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail();
  std::vector<int64_t> cbase((size_t)n_groups + 1, 0);
  for (int64_t g = 0; g < n_groups; g++) cbase[(size_t)g + 1] = cbase[(size_t)g] + totals[(size_t)g];
  c->total = cbase[(size_t)n_groups];
  c->counts[HC_COMPRESSED] = c->total;
  // the output, sized exactly (the bytes to a whole word)
  what = "hipMalloc of the compressed reads";
  e = c->d_cbases.ensure((size_t)c->total + 16);
  if (e == hipSuccess) e = c->d_starts.ensure(4 * (size_t)(c->total + n_reads) + 16);
  if (e == hipSuccess) e = c->d_coff.ensure(8 * (size_t)(n_reads + 1));
  if (e == hipSuccess) e = c->d_clen.ensure(4 * (size_t)std::max<int64_t>(n_reads, 1));
  if (e == hipSuccess) e = hipMemsetAsync(c->d_coff.p, 0, 8, st);   // (coff[0]; with reads, the kernel writes it again)
  mark(3);
  what = "pass 2";
  for (int64_t g = 0; g < n_groups && e == hipSuccess; g++) {
    const HpcGroup& G = groups[(size_t)g];
    const int64_t nr = G.r1 - G.r0;
    hipLaunchKernelGGL(reads_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st, s.tile_first.as<int32_t>(), s.tile_out.as<int32_t>(),
                       s.len.as<int32_t>(), (int32_t)G.r0, (int32_t)nr, (int32_t)G.tile0, (int32_t)G.tiles, (int32_t)totals[(size_t)g], cbase[(size_t)g],
                       n_reads, c->d_coff.as<int64_t>(), c->d_clen.as<int32_t>(), c->d_starts.as<int32_t>());
    if (G.tiles > 0)
      hipLaunchKernelGGL(write_kernel, dim3((unsigned)G.tiles), dim3(HPC_T), 0, st, s.bases.as<uint8_t>(), s.tiles.as<HpcTile>(), s.tile_read.as<int32_t>(),
                         s.tile_out.as<int32_t>(), (int32_t)G.tile0, cbase[(size_t)g], c->d_cbases.as<uint8_t>(), c->d_starts.as<int32_t>(), s.info.as<int4>());
    e = hipGetLastError();
  }
  mark(4);
  what = "the run counts";
  for (int64_t g = 0; g < n_groups && e == hipSuccess; g++) {
    const HpcGroup& G = groups[(size_t)g];
    if (G.tiles == 0) continue;
    hipLaunchKernelGGL(edge_kernel, dim3((unsigned)((G.tiles + 255) / 256)), dim3(256), 0, st, s.tiles.as<HpcTile>(), s.tile_read.as<int32_t>(),
                       s.tile_first.as<int32_t>(), s.info.as<int4>(), (int32_t)G.tile0, (int32_t)G.tiles, s.counts.as<u64>());
    e = hipGetLastError();
  }
  mark(5);
  u64 runs[2] = {0, 0};
  c->clen.resize((size_t)n_reads);
  if (e == hipSuccess) e = hipMemcpyAsync(runs, s.counts.p, sizeof runs, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && n_reads > 0) e = hipMemcpyAsync(c->clen.data(), c->d_clen.p, 4 * (size_t)n_reads, hipMemcpyDeviceToHost, st);
  mark(6);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail();
  c->counts[HC_LONG_RUNS] = (int64_t)runs[0];
  c->counts[HC_LONGEST] = (int64_t)runs[1];
  float a = 0.f, b = 0.f;
  (void)hipEventElapsedTime(&a, s.ev[0], s.ev[1]); c->ms[0] = a;
  (void)hipEventElapsedTime(&a, s.ev[1], s.ev[2]); (void)hipEventElapsedTime(&b, s.ev[3], s.ev[4]); c->ms[1] = (double)a + b;
  (void)hipEventElapsedTime(&a, s.ev[4], s.ev[5]); c->ms[2] = a;
  c->ms[3] = wall_ms() - t_begin;
  *out = c;
  return MHAP_OK;
}

extern "C" int mhap_hpc_info(const mhap_hpc* c, int64_t* counts) {
  if (!c || !counts) return MHAP_E_INVALID;
  for (int k = 0; k < MHAP_HPC_COUNTS; k++) counts[k] = c->counts[k];
  return MHAP_OK;
}

extern "C" int mhap_hpc_times(const mhap_hpc* c, double* ms) {
  if (!c || !ms) return MHAP_E_INVALID;
  for (int k = 0; k < 4; k++) ms[k] = c->ms[k];
  return MHAP_OK;
}

extern "C" int mhap_hpc_copy(const mhap_hpc* c, uint8_t* cbases, int64_t* coff, int32_t* clen, int32_t* starts) {
  const char* who = "mhap_hpc_copy";
  if (!c) return MHAP_E_INVALID;
  HandleView v = handle_view(c->h);
  (void)hipSetDevice(c->device);
  hipError_t e = hipSuccess;
  if (cbases && c->total > 0) e = hipMemcpyAsync(cbases, c->d_cbases.p, (size_t)c->total, hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess && coff) e = hipMemcpyAsync(coff, c->d_coff.p, 8 * (size_t)(c->n + 1), hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess && clen && c->n > 0) e = hipMemcpyAsync(clen, c->d_clen.p, 4 * (size_t)c->n, hipMemcpyDeviceToHost, v.stream);
  if (e == hipSuccess && starts && c->total + c->n > 0) e = hipMemcpyAsync(starts, c->d_starts.p, 4 * (size_t)(c->total + c->n), hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);
  if (e == hipSuccess) e = es;
  return e == hipSuccess ? MHAP_OK : hip_fail(v, who, "download", e);
}

extern "C" int mhap_hpc_expand_records(const mhap_hpc* from_side, const mhap_hpc* to_side, const mhap_record* in, int64_t n, mhap_record* out) {
  const char* who = "mhap_hpc_expand_records";
  if (!from_side) return MHAP_E_INVALID;
  const mhap_hpc* side[2] = {from_side, to_side ? to_side : from_side};
  HandleView v = handle_view(from_side->h);
  if (n < 0 || (n > 0 && (!in || !out))) { *v.err = std::string(who) + ": null or negative argument"; return MHAP_E_INVALID; }
  if (n > INT32_MAX) { *v.err = std::string(who) + ": more than 2^31 - 1 records in one call"; return MHAP_E_INVALID; }
  if (side[1]->device != side[0]->device) { *v.err = std::string(who) + ": the two sides are on different devices"; return MHAP_E_INVALID; }
  if (n == 0) return MHAP_OK;
  std::vector<XItem> items((size_t)n);
  for (int64_t q = 0; q < n; q++) {
    const mhap_record& r = in[q];
    const int64_t rid[2] = {r.from_id, r.to_id};
    const int32_t lens[2] = {r.alen, r.blen};
    int32_t row[2];
    for (int f = 0; f < 2; f++) {
      const auto it = side[f]->by_id.find(rid[f]);
      if (it == side[f]->by_id.end()) {
        *v.err = std::string(who) + ": record " + std::to_string(q) + " names read " + std::to_string(rid[f]) + ", which is not among the " + (f ? "`to`" : "`from`") + " reads";
        return MHAP_E_INVALID;
      }
      row[f] = it->second;
      if (side[f]->clen[(size_t)row[f]] != lens[f]) {
        *v.err = std::string(who) + ": record " + std::to_string(q) + " gives read " + std::to_string(rid[f]) + " the length " + std::to_string(lens[f]) +
                 ", compressed it has " + std::to_string(side[f]->clen[(size_t)row[f]]);
        return MHAP_E_INVALID;
      }
    }
    items[(size_t)q] = XItem{row[0], row[1], r.a1, r.a2, r.b1, r.b2};
  }
  (void)hipSetDevice(side[0]->device);
  DevBuf d_items, d_out;
  hipError_t e = d_items.ensure(sizeof(XItem) * (size_t)n);
  if (e == hipSuccess) e = d_out.ensure(32 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_items.p, items.data(), sizeof(XItem) * (size_t)n, hipMemcpyHostToDevice, v.stream);
  std::vector<int32_t> got(8 * (size_t)n);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v.stream, d_items.as<XItem>(), n, side[0]->d_coff.as<int64_t>(),
                       side[0]->d_clen.as<int32_t>(), side[0]->d_starts.as<int32_t>(), side[1]->d_coff.as<int64_t>(), side[1]->d_clen.as<int32_t>(),
                       side[1]->d_starts.as<int32_t>(), d_out.as<int4>());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), d_out.p, 32 * (size_t)n, hipMemcpyDeviceToHost, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);   // (the upload reads a host vector of this call: waited for whatever happened)
  if (e == hipSuccess) e = es;
  d_items.release(); d_out.release();
  if (e != hipSuccess) return hip_fail(v, who, "upload, kernel or download", e);
  for (int64_t q = 0; q < n; q++) {
    const int32_t* g = got.data() + 8 * (size_t)q;
    out[q] = in[q];
    out[q].a1 = g[0]; out[q].a2 = g[1]; out[q].b1 = g[2]; out[q].b2 = g[3]; out[q].alen = g[4]; out[q].blen = g[5];
  }
  return MHAP_OK;
}

extern "C" void mhap_hpc_free(mhap_hpc* c) {
  if (!c) return;
  HandleView v = handle_view(c->h);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(v.stream);
  c->release();
  delete c;
}
