// pvoc_device.hpp — what the Pvoc kernel files share (pvoc_kernels.hip, pvoc_ops.hip, pvoc_pair.hip, pvoc_time.hip,
// pvoc_delay.hip, pvoc_shape.hip, pvoc_desc.hip, pvoc_trace.hip, pvoc_demix.hip, pvoc_adsyn.hip):
//   pvoc_item, pvoc_grid, pvoc_group_row, pvoc_groups   the decoding of a grid-stride item, the cap on a launch's
//                          workgroups and the group kernels' scheme (k_pvoc_desc<W>, k_pvoc_trace<W>): pvoc_group.hpp's,
//                          included here, which pitch_kernels.hip shares
//   pvoc_bin               the bin a lane of a tile kernel takes of an item
//   pvoc_tiles             the tiles, items and grid of a tile launch
//   kTimeWG, kTimeRun      the item of the kernels along the frames (pvoc_time.hip, pvoc_delay.hip): a tile of bins, a run of frames
//   desc_dpp, desc_xor, desc_fold   the in-wave moves and the fold of the descriptors' TREE SUM (k_pvoc_desc<W>, k_pvoc_demix_az<LOGM>):
//                          tree_moves.hpp's, included here
//   pvoc_empty, pvoc_clamp01, pvoc_morph   the frame operations' EMPTY bin, clamp and interpolation rule
//   pvoc_scale_source      the pitch scale's source map (k_pvoc_map, k_pvoc_formant, k_pvoc_warp)
//   pvoc_scan              the chunked scan that turns the per-chunk sums of phase increments into the bases the
//                          chunks start from (k_pvoc_scan on uint32 words, k_adsyn_scan on uint64 ones)
#pragma once
#include "pvoc_group.hpp"
#include "pvoc_launch.hpp"
#include "tree_moves.hpp"

namespace clfa {

constexpr int kScanBins = 64, kScanSegs = 16;   // the scan's workgroup: a wave per segment of the chunk axis
constexpr int kTimeWG = 256;   // lanes = bins per workgroup tile (k_pvoc_blur, k_pvoc_freeze, k_pvoc_tail, k_pvoc_fill, k_pvoc_delay)
constexpr int kTimeRun = 8;    // consecutive frames per item of those

// The prologue of a tile kernel (a lane per bin, WG bins per tile): the item's (c, j) and the lane's bin k; false where
// the last tile reaches past bin M
template <int WG>
__device__ __forceinline__ bool pvoc_bin(long item, int tiles, long inner, int M, int &k, long &j, long &c) {
  int tile;
  pvoc_item(item, tiles, inner, tile, j, c);
  k = tile * WG + (int)threadIdx.x;
  return k <= M;
}

// A tile launch: tiles of `lanes` bins per row of M + 1, `outer` rows (channels x frames, runs, ...), an item per tile,
// at most per_cu workgroups per CU
struct PvocTiles {
  int tiles, grid;
  long items;
};
static inline PvocTiles pvoc_tiles(int M, int lanes, long outer, const DeviceInfo &di, int per_cu, int grid_max) {
  PvocTiles t;
  t.tiles = (M + 1 + lanes - 1) / lanes;
  t.items = outer * t.tiles;
  t.grid = pvoc_grid(t.items, (long)di.num_cus * per_cu, grid_max);
  return t;
}

// an EMPTY bin of the frame operations: silent, at its bin centre (cf = sr / size)
__device__ __forceinline__ cpx pvoc_empty(int j, float cf) {
#pragma clang fp contract(off)
  return mk(0.f, (float)j * cf);
}

__device__ __forceinline__ float pvoc_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // fmaxf(NaN, 0) = 0

constexpr int kSrcEmpty = -1, kSrcCopy = -2;   // what a frame operation's source map answers besides a bin

// the pitch scale's map k -> j
__device__ __forceinline__ int pvoc_scale_j(int k, float s) {
#pragma clang fp contract(off)
  const float t = (float)k * s;
  return (int)floorf(t + 0.5f);
}

// The pitch scale's source of bin j, 1 <= j <= M-1: k in 1..M-1, or kSrcEmpty (also for s outside [1/4, 4] or a NaN).
// k -> j is monotone, so the source — the last k of the serial definition — is the largest k with j(k) <= j if that k
// lands on j; it lies next to (j + 1/2) / s, and the two loops move the estimate there (a few steps: s >= 1/4).
// Shared by the scale map (pvoc_ops.hip) and the envelope warp (pvoc_shape.hip).
__device__ __forceinline__ int pvoc_scale_source(int j, int M, float s) {
#pragma clang fp contract(off)
  if (!(s >= 0.25f && s <= 4.f)) return kSrcEmpty;
  int k = (int)(((float)j + 0.5f) / s);
  k = k < 1 ? 1 : (k > M - 1 ? M - 1 : k);
  while (k < M - 1 && pvoc_scale_j(k + 1, s) <= j) k++;
  while (k >= 1 && pvoc_scale_j(k, s) > j) k--;
  return (k >= 1 && pvoc_scale_j(k, s) == j) ? k : kSrcEmpty;
}

// x0 where w == 0, x1 where w == 1 (the bits; the other side is not used), else fl(x0 + fl(w fl(x1 - x0))): the rule of
// the morph (pvoc_pair.hip) and of the smoothing along the frames (pvoc_time.hip)
__device__ __forceinline__ float pvoc_morph(float x0, float x1, float w) {
#pragma clang fp contract(off)
  const float d = x1 - x0;
  const float s = w * d;
  const float m = x0 + s;
  return w == 0.f ? x0 : (w == 1.f ? x1 : m);
}

// The scan of one column (one bin of one channel) by the kScanSegs lanes that share `lane`: wave `seg` takes the chunks
// [seg len, (seg + 1) len).  col: the column's entry of chunk 0, the chunks `stride` words apart, nch of them: their sums
// become their bases in place (the state plus the sums of the chunks before).  *state takes the total, and the one lane
// that stores it then runs store() (what else belongs to the new state).  Every lane of the workgroup calls this; a lane
// that is not live touches no memory.
// The barrier rule: every read of the old state is before the barrier, its one write after it.
template <class Word, class Store>
__device__ __forceinline__ void pvoc_scan(Word *col, long stride, long nch, bool live, Word *state, Store store) {
  __shared__ Word s_tot[kScanSegs][kScanBins];
  const int lane = threadIdx.x & (kScanBins - 1), seg = threadIdx.x / kScanBins;
  const long len = (nch + kScanSegs - 1) / kScanSegs;
  const long j0 = seg * len < nch ? seg * len : nch, j1 = j0 + len < nch ? j0 + len : nch;
  Word tot = 0, old = 0;
  if (live) {
    old = *state;
    for (long j = j0; j < j1; j++) tot += col[j * stride];
  }
  s_tot[seg][lane] = tot;
  __syncthreads();
  if (!live) return;
  Word run = old;
  for (int s = 0; s < seg; s++) run += s_tot[s][lane];
  if (seg == 0) {
    Word all = old;
    for (int s = 0; s < kScanSegs; s++) all += s_tot[s][lane];
    *state = all;
    store();
  }
  for (long j = j0; j < j1; j++) {
    const Word v = col[j * stride];
    col[j * stride] = run;
    run += v;
  }
}

}  // namespace clfa
