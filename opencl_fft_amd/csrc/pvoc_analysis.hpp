// pvoc_analysis.hpp — the bin map of clfa_pvoc (include/clfft_amd.h): z[k] of a packed spectrum, shared by k_pvoc_analyze
// (pvoc_kernels.hip) and k_pvoc_tanal (tanal_kernels.hip).  The conversion of a bin to (amp, freq) that goes with it is
// pvoc_analysis_bin.inc.  Nothing of the launchers or of the FFT engine: cpx.hpp alone.
#pragma once
#include "cpx.hpp"

namespace clfa {

// z[k] from p = P[k == M ? 0 : k] of a packed spectrum: bin 0 = (Re P[0], 0), bin M = (Im P[0], 0), bin M/2 conjugated
__device__ __forceinline__ cpx pvoc_bin_of(cpx p, int k, int M) {
  if (k == 0) return mk(p.x, 0.f);
  if (k == M) return mk(p.y, 0.f);
  if (k == (M >> 1)) return mk(p.x, -p.y);
  return p;
}

// z[k] of a packed row
__device__ __forceinline__ cpx pvoc_bin(const cpx *__restrict__ row, int k, int M) {
  return pvoc_bin_of(row[k == M ? 0 : k], k, M);
}

}  // namespace clfa
