// adsyn_step (opencl_fft_amd/csrc/pvoc_adsyn_plan.hpp) against the composition of the functions it is made of, over the
// value grid of tests/test_pvoc_adsyn_cpu.py: silent endpoints, -0 and NaN amps, negative differences, every hop.
// A program of its own, for a sanitizer build (tests/test_pvoc_adsyn_cpu.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I../../opencl_fft_amd/csrc adsyn_step_check.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pvoc_adsyn_plan.hpp"

using namespace clfa;

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0 || (std::isnan(a) && std::isnan(b)); }

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float ks = (float)(1.0 / 48000.0);
  const int top = 2147483647 - 127;   // 2^31 - 128, the largest endpoint word
  const float freqs[] = {0.f, -0.f, 1e-30f, 23999.9f, 24000.f, -24000.f, 23999.998f, -23999.998f, 1e9f, inf, -inf, nan,
                         -17000.25f, 440.f, 12345.678f, -3.f};
  const float fmods[] = {1.f, 0.5f, 2.f, nan};   // the first: without fmod
  const int words[] = {0, 1, -1, top, -top, 2, -2, 12345, -12345, 1 << 30, -(1 << 30), top - 128};
  const float a0s[] = {0.f, -0.f, 1e-45f, 1.f, nan};
  const float amps[] = {3.f, 0.f, -0.f, nan};
  std::vector<int> hops;
  for (int h = 1; h <= 64; h++) hops.push_back(h);
  hops.insert(hops.end(), {255, 256, 16384});
  long cases = 0, silent = 0, negative_inexact = 0, restarted = 0;
  for (float freq : freqs)
    for (size_t m = 0; m < sizeof fmods / sizeof *fmods; m++)
      for (int w0 : words)
        for (float a0 : a0s)
          for (float amp : amps)
            for (int hop : hops) {
              const bool has = m != 0;
              int32_t wf, ws_want;
              float af;
              adsyn_endpoint(amp, freq, fmods[m], has, ks, wf, af);
              ws_want = adsyn_start(a0, w0, wf);
              const uint64_t d_want = adsyn_slope(ws_want, wf, hop), adv_want = adsyn_advance(ws_want, d_want, hop);
              int32_t w = w0, ws = 0;
              float a = a0;
              uint64_t d = 0;
              const uint64_t adv = adsyn_step(w, a, amp, freq, fmods[m], has, ks, hop, ws, d);
              if (w != wf || !same_bits(a, af) || ws != ws_want || d != d_want || adv != adv_want) {
                std::printf("MISMATCH freq %g fmod %g (%d) w0 %d a0 %g amp %g hop %d\n", freq, fmods[m], (int)has, w0, a0, amp, hop);
                return 1;
              }
              cases++;
              silent += !adsyn_word(adsyn_turns(freq, fmods[m], has, ks), wf);
              restarted += ws_want != w0;
              negative_inexact += wf < ws_want && (((int64_t)wf - ws_want) * ((int64_t)1 << 30)) % hop != 0;
            }
  std::printf("adsyn_step ok: %ld cases, %ld silent endpoints, %ld restarts, %ld negative inexact slopes\n", cases, silent,
              restarted, negative_inexact);
  return silent > 0 && restarted > 0 && negative_inexact > 1000 ? 0 : 2;
}
