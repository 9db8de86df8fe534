// pvoc_adsyn_plan.hpp — the arithmetic of the oscillator-bank resynthesis (clfa_pvoc_adsyn, include/clfft_amd.h;
// kernels: pvoc_adsyn.hip): the endpoint word of a frame, the start rule, the phase slope D, phase(j), the advance of a
// frame, and adsyn_step, which puts them together for one frame of one oscillator.  Plain functions of plain arguments,
// for the host and the device alike: tests/test_pvoc_adsyn_cpu.py builds them with g++ and checks them against Python
// integers.  Phases are uint64 in 2^-64 turn, frequencies int32 in 2^-32 turn per sample; every sum is taken mod 2^64,
// so any grouping of the frames' advances gives the bits of the serial sum.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef CLFA_PLAN_HD
#if defined(__HIPCC__)
#define CLFA_PLAN_HD __host__ __device__
#else
#define CLFA_PLAN_HD
#endif
#endif

namespace clfa {

// t = fl(fl(freq * fmod) * ks), or fl(freq * ks) without fmod: turns per sample, every product rounded on its own
CLFA_PLAN_HD inline float adsyn_turns(float freq, float fmod, bool has_fmod, float ks) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float t = freq;
  if (has_fmod) t = t * fmod;
  return t * ks;
}

// the endpoint word: |t| < 1/2 -> rint(t 2^32), exact in double and |.| <= 2^31 - 128; anything else (NaN, infinities,
// at or above Nyquist) is silent: false, w = 0
CLFA_PLAN_HD inline bool adsyn_word(float t, int32_t &w) {
  if (!(fabsf(t) < 0.5f)) {
    w = 0;
    return false;
  }
  w = (int32_t)rint((double)t * 4294967296.0);
  return true;
}

// (W_f, A_f) of one bin of one frame; a NaN amp with a good t is kept
CLFA_PLAN_HD inline void adsyn_endpoint(float amp, float freq, float fmod, bool has_fmod, float ks, int32_t &w, float &a) {
  a = adsyn_word(adsyn_turns(freq, fmod, has_fmod, ks), w) ? amp : 0.f;
}

// the start rule: an oscillator that was silent starts at its new frequency (a rule on values: -0 counts, NaN does not)
CLFA_PLAN_HD inline int32_t adsyn_start(float a0, int32_t w0, int32_t wf) { return a0 == 0.f ? wf : w0; }

// D = floor_div((W_f - W0) 2^30, hop) * 4 mod 2^64, the floor towards minus infinity; |(W_f - W0) 2^30| < 2^62
CLFA_PLAN_HD inline uint64_t adsyn_slope(int32_t w0, int32_t wf, int hop) {
  const int64_t n = ((int64_t)wf - (int64_t)w0) * ((int64_t)1 << 30);
  int64_t q = n / hop;
  if (n < 0 && q * hop != n) q--;
  return (uint64_t)q << 2;
}

// j (j + 1) / 2 for j <= 16384 (and far beyond)
CLFA_PLAN_HD inline uint32_t adsyn_tri(uint32_t j) { return (uint32_t)(((uint64_t)j * (j + 1)) >> 1); }

// phase(j) = P + j (W0 2^32) + (j (j + 1) / 2) D mod 2^64, j = 1..hop
CLFA_PLAN_HD inline uint64_t adsyn_phase(uint64_t p, int32_t w0, uint64_t d, uint32_t j) {
  return p + ((uint64_t)(uint32_t)(j * (uint32_t)w0) << 32) + (uint64_t)adsyn_tri(j) * d;
}

// the top 32 bits of phase(j), as the hot loop forms them: j (W0 2^32) only reaches the high word.  tri = adsyn_tri(j)
CLFA_PLAN_HD inline uint32_t adsyn_phase_hi(uint64_t p, int32_t w0, uint64_t d, uint32_t j, uint32_t tri) {
  return (uint32_t)((p + (uint64_t)tri * d) >> 32) + j * (uint32_t)w0;
}

// the advance of a frame: phase(hop) - P.  It depends on the frame's endpoint and the one before only
CLFA_PLAN_HD inline uint64_t adsyn_advance(int32_t w0, uint64_t d, int hop) { return adsyn_phase(0, w0, d, (uint32_t)hop); }

// one frame of one oscillator: (w, a) comes in as the endpoint of the frame before and goes out as this frame's; ws = W0
// after the start rule, d = D; returns the frame's advance
CLFA_PLAN_HD inline uint64_t adsyn_step(int32_t &w, float &a, float amp, float freq, float fmod, bool has_fmod, float ks,
                                        int hop, int32_t &ws, uint64_t &d) {
  int32_t wf;
  float af;
  adsyn_endpoint(amp, freq, fmod, has_fmod, ks, wf, af);
  ws = adsyn_start(a, w, wf);
  d = adsyn_slope(ws, wf, hop);
  w = wf;
  a = af;
  return adsyn_advance(ws, d, hop);
}

}  // namespace clfa
