// pvoc_demix_bin.hpp — one bin and one frame's window of the stereo demix of clfa_pvoc (include/clfft_amd.h,
// clfa_pvoc_demix_dev), as the kernels of pvoc_demix.hip evaluate them.  Plain C++: tests/test_pvoc_demix_cpu.py builds
// it with g++ and compares it with the literal scan of tests/pvoc_demix_model.py, bit for bit.
//
// The definition scans d[n] = |h(n)|, h(n) = fl(quiet - fl(g[n] loud)), g[n] = fl((float)n / (float)P), over n = 0..P.
// g is non-decreasing in n and every rounding is monotone, so h is monotone in n (down for loud >= 0, up for loud < 0) and
// |h| falls, or rises, or falls to where h changes sign and rises from there.  Hence
//   mx  is |h(0)| or |h(P)|;
//   m   is |h| at 0, at the last n before the sign changes (or P), or at the first n from which it has changed;
//   nmin, the lowest n with d[n] == m, is 0, the first n of the plateau that ends before the change, or the first n after it.
// Two bisections of at most log2(P) + 1 steps each find the change of sign and the start of the plateau: about 2 log2(P)
// evaluations of h instead of P + 1.  A NaN anywhere in the scan is a NaN at n = 0 (g[0] = 0: an infinite loud gives
// 0 * inf), so one test of h(0) covers it.
//
// Every float32 step is rounded on its own: contraction is off in every function below.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLFA_DEMIX_HD __host__ __device__ __forceinline__
#else
#define CLFA_DEMIX_HD inline
#endif
#if defined(__clang__)
#define CLFA_DEMIX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CLFA_DEMIX_NO_CONTRACT   // g++: the test builds with -ffp-contract=off
#endif

namespace clfa {

constexpr int kDemixPointsMax = 1024;   // P = points, 1..1024

struct DemixBin {
  bool left;     // the side: L > R (a tie or a NaN is RIGHT)
  bool placed;   // no d[n] is a NaN and mag > 0
  int u;         // the azimuth, -P (hard left) .. P (hard right); meaningful where placed
  float mag;     // fl(mx - m)
};

// h(n) = fl(quiet - fl(g[n] loud))
CLFA_DEMIX_HD float demix_h(int n, float Pf, float loud, float quiet) {
  CLFA_DEMIX_NO_CONTRACT
  const float g = (float)n / Pf;   // the correctly rounded division
  const float p = g * loud;
  return quiet - p;
}

// the first n of a..b at which pred holds: pred holds at b, and from the first n on
template <class Pred>
CLFA_DEMIX_HD int demix_first(int a, int b, Pred pred) {
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (pred(mid)) b = mid;
    else a = mid + 1;
  }
  return b;
}

CLFA_DEMIX_HD DemixBin demix_bin(float L, float R, int P) {
  CLFA_DEMIX_NO_CONTRACT
  DemixBin r;
  r.left = L > R;
  r.placed = false;
  r.u = 0;
  r.mag = 0.f;
  const float loud = r.left ? L : R, quiet = r.left ? R : L, Pf = (float)P;
  const float h0 = demix_h(0, Pf, loud, quiet);
  if (h0 != h0) return r;
  const float hP = demix_h(P, Pf, loud, quiet);
  const float d0 = fabsf(h0), dP = fabsf(hP);
  const float mx = d0 > dP ? d0 : dP;
  float m = d0;
  int nmin = 0;
  if (h0 != 0.f) {
    // the sign of h(0) has gone: h <= 0 after a positive h(0), h >= 0 after a negative one
    const bool pos = h0 > 0.f;
    const auto changed = [&](int n) {
      const float h = demix_h(n, Pf, loud, quiet);
      return pos ? h <= 0.f : h >= 0.f;
    };
    const bool changes = pos ? hP <= 0.f : hP >= 0.f;
    const int nc = changes ? demix_first(1, P, changed) : P + 1;
    // 0 .. e keep the sign: |h| is monotone there, its smallest value at 0 or on the plateau that ends at e
    const int e = nc - 1;
    const float he = demix_h(e, Pf, loud, quiet), de = fabsf(he);
    if (de < d0) {
      m = de;
      nmin = demix_first(0, e, [&](int n) { return demix_h(n, Pf, loud, quiet) == he; });
    }
    if (changes) {   // from nc on |h| does not fall: nc is the only other candidate, and loses a tie to a lower n
      const float dc = fabsf(demix_h(nc, Pf, loud, quiet));
      if (dc < m) {
        m = dc;
        nmin = nc;
      }
    }
  }
  r.mag = mx - m;
  r.placed = r.mag > 0.f;
  r.u = r.left ? nmin - P : P - nmin;
  return r;
}

// the window of a frame: its centre c on the azimuth axis and its half width H, from the frame's (pos, width)
struct DemixWindow {
  int c, H;
};
CLFA_DEMIX_HD DemixWindow demix_window(float pos, float width, int P) {
  CLFA_DEMIX_NO_CONTRACT
  DemixWindow w;
  const float pc = fminf(fmaxf(pos, -1.f), 1.f);   // fmaxf(NaN, -1) = -1
  w.c = (int)rintf(pc * (float)P);
  const float ww = fminf(fmaxf(width, 1.f), (float)(2 * P + 1));   // fmaxf(NaN, 1) = 1
  w.H = (int)ww / 2;
  return w;
}
CLFA_DEMIX_HD bool demix_inside(DemixWindow w, int u) {
  const int d = u - w.c;
  return (d < 0 ? -d : d) <= w.H;
}

}  // namespace clfa
