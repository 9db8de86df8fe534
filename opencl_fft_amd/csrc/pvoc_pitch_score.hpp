// pvoc_pitch_score.hpp — the peak test and the score of one candidate of the pitch estimate of clfa_pvoc
// (include/clfft_amd.h, clfa_pvoc_pitch_dev), as k_pvoc_pitch of pitch_kernels.hip evaluates them.  Plain C++:
// tests/test_pvoc_pitch_cpu.py builds it with g++ and compares it with tests/pvoc_pitch_model.py, bit for bit.
//
// The score is serial over the list on purpose: the order of its additions is the definition's, and a lane that owns a
// candidate runs it alone.
//
// Every float32 step is rounded on its own: contraction is off in every function below.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLFA_PITCH_HD __host__ __device__ __forceinline__
#else
#define CLFA_PITCH_HD inline
#endif
#if defined(__clang__)
#define CLFA_PITCH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CLFA_PITCH_NO_CONTRACT   // g++: the test builds with -ffp-contract=off
#endif

namespace clfa {

constexpr int kPitchDiv = 8;        // CLFA_PVOC_PITCH_DIV: a candidate is a peak's freq over 1..8
constexpr int kPitchHarm = 32;      // CLFA_PVOC_PITCH_HARM: the harmonic numbers that count, 1..32
constexpr int kPitchPeaksMax = 32;  // CLFA_PVOC_PITCH_PEAKS_MAX

// PEAK: al, a, ar the amps of the bins k - 1, k, k + 1, q the freq of bin k.  A NaN makes its comparison false
CLFA_PITCH_HD bool pitch_is_peak(float al, float a, float ar, float q, float thresh) {
  return a > al && a >= ar && a >= thresh && q > 0.f && q <= 3.402823466e+38f;
}

// SCORE of the candidate c over the list (A[j], Q[j]), j < L, in list order from +0; w[h - 1] the weight of harmonic h
CLFA_PITCH_HD float pitch_score(const float *A, const float *Q, int L, float c, const float *w, float tol) {
  CLFA_PITCH_NO_CONTRACT
  float s = 0.f;
  for (int j = 0; j < L; j++) {
    const float r = Q[j] / c;   // the correctly rounded division
    const float h = rintf(r);
    if (h >= 1.f && h <= (float)kPitchHarm) {   // false for a NaN
      const float d = fabsf(r - h);
      const float e = d / h;
      if (e <= tol) {
        const float t = A[j] * w[(int)h - 1];
        s = s + t;
      }
    }
  }
  return s;
}

}  // namespace clfa
