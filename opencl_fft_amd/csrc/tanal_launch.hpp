// tanal_launch.hpp — the launcher of the analysis of a stored signal at given time points (tanal_kernels.hip) as
// pvoc_signal_host.cpp sees it: PvocTanalArgs and launch_pvoc_tanal.  A header of its own: the kernel file shares the FFT engine
// with stft_kernels.hip and nothing with the launchers of the frame operations (pvoc_launch.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

// signal: channels rows of `samples` floats, row c at c * stride floats; window: 2 M floats; starts: Fout int32, shared by
// the channels; out: channels x Fout x (M + 1) (amp, freq) pairs.  Frame (c, g) is the Analysis of the windows at
// starts[g] - hop and starts[g], samples outside the row being +0.
struct PvocTanalArgs {
  int logn = 0;                    // log2(M): the transform length (complex)
  int M = 0, channels = 0, hop = 1;
  long Fout = 0, samples = 0, stride = 0;
  const float *signal = nullptr, *window = nullptr;
  const int *starts = nullptr;
  cpx *out = nullptr;
  const cpx *etab = nullptr;       // M + 1 expected advances e[k]
  const cpx *half = nullptr, *w2 = nullptr;   // the Clrfft tables of size (forward sign)
  float sh = 0.f, srs = 0.f;       // size / hop, sr / size
  int grid_max = 0;                // > 0: at most this many workgroups
};
// one launch: k_pvoc_tanal<logn>
hipError_t launch_pvoc_tanal(const PvocTanalArgs &a, const DeviceInfo &di, hipStream_t s);

}  // namespace clfa
