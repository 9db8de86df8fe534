// pvoc_group.hpp — the item decoding and the group scheme of the kernels that give a row of a channel to a group of lanes
// (k_pvoc_desc<W>, k_pvoc_trace<W>, k_pvoc_pitch<W>).  A header of its own under pvoc_device.hpp, which includes it: it
// needs nothing of the launchers of the frame operations (pvoc_launch.hpp), so pitch_kernels.hip, which has its own
// launch header as bank_kernels.hip and tanal_kernels.hip have, takes the scheme from here.
//   pvoc_item              the decoding of a grid-stride item
//   pvoc_grid              the cap on a launch's workgroups
//   pvoc_group_row, pvoc_groups   which row of a channel a group of W lanes takes of an item, and the items and grid of
//                          such a launch
#pragma once
#include <hip/hip_runtime.h>

#include "device_info.hpp"

namespace clfa {

// item -> (outer index c, inner index j < inner, tile), the tile fastest: neighbouring workgroups hold neighbouring rows
__device__ __forceinline__ void pvoc_item(long item, int tiles, long inner, int &tile, long &j, long &c) {
  const long rest = item / tiles;
  tile = (int)(item - rest * tiles);
  c = rest / inner;
  j = rest - c * inner;
}

// workgroups of a grid-stride launch: one per item, at most cap, at most grid_max where that is set (> 0)
static inline int pvoc_grid(long items, long cap, int grid_max) {
  if (grid_max > 0 && cap > grid_max) cap = grid_max;
  return (int)(items < cap ? items : cap);
}

// The group kernels: W = min(M, 256) lanes form a group that owns one row of a channel (a frame, a run of frames),
// kGroupWG / W groups share a workgroup, and an item is a (channel, kGroupWG / W consecutive rows).
constexpr int kGroupWG = 256;   // lanes of a workgroup = the largest W
static inline int pvoc_group_lanes(int M) { return M < kGroupWG ? M : kGroupWG; }

// The prologue of a group kernel: the lane's group g of the workgroup and its place j in it, the item's channel c and
// the group's row r of that channel (r may lie past the last row: the group then idles along)
template <int W>
__device__ __forceinline__ void pvoc_group_row(long item, long rgroups, int &g, int &j, long &r, long &c) {
  int tile;
  long rg;
  g = (int)threadIdx.x / W;
  j = (int)threadIdx.x & (W - 1);
  pvoc_item(item, 1, rgroups, tile, rg, c);
  r = rg * (kGroupWG / W) + g;
}

// A group launch over `rows` rows per channel: the groups of rows per channel, the items, the grid
struct PvocGroups {
  long rgroups, items;
  int grid;
};
template <int W>
static inline PvocGroups pvoc_groups(long rows, int channels, const DeviceInfo &di, int grid_max) {
  PvocGroups q;
  q.rgroups = (rows + kGroupWG / W - 1) / (kGroupWG / W);
  q.items = (long)channels * q.rgroups;
  q.grid = pvoc_grid(q.items, (long)di.num_cus * 8, grid_max);
  return q;
}

}  // namespace clfa
