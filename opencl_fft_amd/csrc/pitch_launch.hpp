// pitch_launch.hpp — the launcher of the pitch estimate on (amp, freq) frames (pitch_kernels.hip) as pvoc_rows_host.cpp
// sees it: PvocPitchArgs and launch_pvoc_pitch.  A header of its own, like bank_launch.hpp and tanal_launch.hpp: the kernel file
// shares the group scheme (pvoc_group.hpp) with the descriptors and the trace and nothing with the launchers of the frame
// operations (pvoc_launch.hpp), so an edit there does not rebuild it.
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

struct PvocPitchWeights {
  float w[32];                     // w[h - 1] = (float)pow((double)decay, h - 1), h = 1..32 (kPitchHarm)
};
struct PvocPitchArgs {
  int M = 0, channels = 0;
  long F = 0;
  const cpx *in = nullptr;         // channels x F x (M + 1) (amp, freq) pairs
  float *rows = nullptr;           // channels x F x 4: F0, SAL, CONF, NPEAKS
  cpx *peaks = nullptr;            // NULL, or channels x F x npeaks pairs (amp, freq): the list, then (+0, +0)
  int npeaks = 1;                  // 1..32
  int lo = 1, hi = 1;              // the range of bins, 1 <= lo <= hi <= M - 1
  float thresh = 0.f, fmin = 0.f, fmax = 0.f, tol = 0.f;
  PvocPitchWeights weights;
  int grid_max = 0;                // > 0: at most this many workgroups
};
// one launch: k_pvoc_pitch<min(M, 256)>
hipError_t launch_pvoc_pitch(const PvocPitchArgs &a, const DeviceInfo &di, hipStream_t s);

}  // namespace clfa
