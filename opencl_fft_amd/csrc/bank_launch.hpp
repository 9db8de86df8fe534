// bank_launch.hpp — the launcher of the filter bank on (amp, freq) frames (bank_kernels.hip) as pvoc_rows_host.cpp sees it:
// BankArgs and launch_pvoc_bands.  A header of its own, like tanal_launch.hpp: the kernel file shares the tree's moves
// (tree_moves.hpp) with the descriptors and nothing with the launchers of the frame operations (pvoc_launch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

// in: channels x F x (M + 1) (amp, freq) pairs, the amps read; out: channels x F x N float32, N = ncoef with dct, else B.
// The bank (bank_plan.hpp): bands B x (first, count, woff, 0); sched 17 row starts, then B band numbers; weights; dct_t
// the DCT table transposed, dct_t[b B + q] = D[q][b], so that the lanes of neighbouring q read neighbouring words.
struct BankArgs {
  int M = 0, channels = 0;
  long F = 0;
  const cpx *in = nullptr;
  float *out = nullptr;
  int B = 0, steps = 0;            // the bands; the bands of the schedule's longest row
  const int *bands = nullptr, *sched = nullptr;
  const float *weights = nullptr, *dct_t = nullptr;
  int power = 0, log = 0, dct = 0, ncoef = 0;
  float floor = 0.f;
  int grid_max = 0;                // > 0: at most this many workgroups
};
// one launch: k_pvoc_bands<R>, R the frames of a run (8 up to M = 512, then 4, 2, 1)
hipError_t launch_pvoc_bands(const BankArgs &a, const DeviceInfo &di, hipStream_t s);

}  // namespace clfa
