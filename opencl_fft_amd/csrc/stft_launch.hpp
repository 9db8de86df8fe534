// stft_launch.hpp — the launcher of the short-time transforms (stft_kernels.hip) as stft_host.cpp sees it: StftArgs and
// launch_stft.
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

// ---- short-time transforms (stft_kernels.hip) --------------------------------------
// packed real size 2^(logn + 1), logn 5..kLdsMaxLog.  forward: channels rows of `signal` (row c at c * stride floats) ->
// spec_out, nframes = channels * F frames of n complex; inverse: spec_in (nframes frames) -> rows of `out`, L = (F - 1) hop
// + size floats each.  window: size floats; cum (inverse, normalize only): [lo | hi] running sums of window^2 along steps
// of hop (2 * size floats); half / w2: the Clrfft tables of the direction.  aligned8: every frame start is 8-byte aligned.
struct StftArgs {
  int logn = 0;
  bool forward = true;
  int hop = 1, F = 0;
  long channels = 0, nframes = 0, stride = 0;
  bool aligned8 = true;
  int normalize = 0;
  int grid_max = 0;                // cap on a launch's workgroups (CLFA_STFT_GRID_MAX, 0 = none)
  const float *signal = nullptr;
  float *out = nullptr;
  const cpx *spec_in = nullptr;
  cpx *spec_out = nullptr;
  const float *window = nullptr;
  const double *cum = nullptr;     // the envelope's running sums (stft_plan.hpp)
  const cpx *half = nullptr, *w2 = nullptr;
};
hipError_t launch_stft(const StftArgs &a, const DeviceInfo &di, hipStream_t s);

}  // namespace clfa
