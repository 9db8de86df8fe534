// fft_route.hpp — which kernels an FFT plan runs for a batch, decided once.  Plain C++ (no HIP header):
// tests/test_fft_route_cpu.py builds it with g++ and checks every rule against a table written out in Python.
//
// `cus` is the device's CU count (= fourstep_grid()).  Rules, first match:
//   not a power of two: m in 256..8192    BlueLds          logn <= 13                       Lds
//   not a power of two: other m           Bluestein        logn > 16                        Big
//   complex 16384:                 batch * 4 > cus         Cfft2x13
//   packed real 32768 / 65536:     batch > cus / 8         Rfft2x13 / Rfft2x14
//   packed real 131072:            batch * 4 > cus         RealRes16
//   what is left of logn 14..16 runs the complex transform (real plans: unpack / pack as passes of their own):
//                                  batch * 4 <= cus && batch <= 65535   FourStepSpread
//                                  otherwise               FourStep (logn 14, 15) / Res16 (logn 16)
// The fused real kernels put one workgroup on a transform (13-23 us for a single one); a few transforms are faster spread
// over the column / row blocks of the four-step pair plus the pack kernel (11 us): the crossover was measured between 32
// and 64 transforms on 256 CUs, hence cus / 8.
#pragma once

namespace clfa {

// Largest complex length the single-workgroup LDS kernel handles; above it the four-step kernel
// (two phases, the intermediate in LDS + registers + a small global scratch) takes over.
constexpr int kLdsMaxLog = 13;
constexpr int kMaxLog = 16;       // reference int32 index bound, cl_fft.cpp:32
constexpr int kBig2MaxLog = 22;   // the largest two-pass size above it (fft_big.inc)

enum FftMode { MODE_C2C = 0, MODE_R2C = 1, MODE_C2R = 2 };

enum class FftRoute {
  Lds,             // k_fft_tiny / k_fft_small / k_fft_lds: one launch, real plans with the pair map inside
  Cfft2x13,        // k_cfft_2x<13>: two 8192-point runs per transform, two workgroups per CU
  Rfft2x13,        // k_rfft_2x<13>: the same, with the pair maps in registers
  Rfft2x14,        // k_rfft_2x<14>: two 16384-point runs per transform, one HBM pass
  FourStepSpread,  // k_fft_4step_cols + k_fft_4step_rows: a few transforms, one workgroup per block
  FourStep,        // k_fft_4step: one persistent workgroup per CU
  Res16,           // k_fft_res16: n = 65536 resident on the CU
  RealRes16,       // ... with the pair map inside (one HBM pass), either direction
  Big,             // n > 65536: columns + rows (+ transpose), the batch in chunks
  BlueLds,         // k_blue_lds: Bluestein in one launch
  Bluestein        // chirp, two m-point sub-plans, chirp: the batch in chunks
};

struct FftShape {        // fixed at creation; only the batch varies per call
  bool real = false;     // Clrfft
  bool fwd = true;
  int n = 0;             // complex length (Clrfft: size / 2)
  int logn = 0;          // -1: not a power of two
  int blue_m = 0;        // ... then the length of the two power-of-two sub-plans
  int num_cus = 256;
};

// the shape of a plan of complex length n >= 2 (a length that is not a power of two runs Bluestein's algorithm around two
// transforms of the next power of two m >= 2 n - 1)
constexpr FftShape fft_shape(bool real, bool fwd, int n, int num_cus) {
  FftShape s{real, fwd, n, 0, 0, num_cus};
  while ((1 << s.logn) < n) s.logn++;
  if ((1 << s.logn) != n) {
    s.logn = -1;
    for (s.blue_m = 1; s.blue_m < 2 * n - 1;) s.blue_m <<= 1;
  }
  return s;
}

constexpr bool blue_lds_ok(int m) { return m >= 256 && m <= 8192; }

// the four-step launcher's own test (fft_4step.inc): also what Clpconv above the LDS sizes and the big-N rows take
constexpr bool fourstep_spread(long batch, int num_cus) { return batch * 4 <= num_cus && batch <= 65535; }

// the route of a batch above every threshold
constexpr FftRoute fft_route_many(const FftShape &s) {
  if (s.blue_m) return blue_lds_ok(s.blue_m) ? FftRoute::BlueLds : FftRoute::Bluestein;
  if (s.logn <= kLdsMaxLog) return FftRoute::Lds;
  if (s.logn > kMaxLog) return FftRoute::Big;
  if (s.real) return s.logn == 14 ? FftRoute::Rfft2x13 : s.logn == 15 ? FftRoute::Rfft2x14 : FftRoute::RealRes16;
  return s.logn == 14 ? FftRoute::Cfft2x13 : s.logn == 15 ? FftRoute::FourStep : FftRoute::Res16;
}

constexpr FftRoute fft_route(const FftShape &s, long batch) {
  const FftRoute many = fft_route_many(s);
  if (s.blue_m || s.logn <= kLdsMaxLog || s.logn > kMaxLog) return many;
  const bool eighth = many == FftRoute::Rfft2x13 || many == FftRoute::Rfft2x14;
  const bool fused = eighth || many == FftRoute::Cfft2x13 || many == FftRoute::RealRes16;
  if (fused && (eighth ? batch > s.num_cus / 8 : batch * 4 > s.num_cus)) return many;
  if (fourstep_spread(batch, s.num_cus)) return FftRoute::FourStepSpread;
  return s.logn == 16 ? FftRoute::Res16 : FftRoute::FourStep;
}

// every route some batch of the shape can take, as a mask of 1 << route
constexpr unsigned fft_routes(const FftShape &s) {
  unsigned m = 1u << (int)fft_route_many(s);
  if (!s.blue_m && s.logn > kLdsMaxLog && s.logn <= kMaxLog)
    m |= 1u << (int)FftRoute::FourStepSpread | 1u << (int)(s.logn == 16 ? FftRoute::Res16 : FftRoute::FourStep);
  return m;
}

// ---- facts of a route -------------------------------------------------------------------------------------------------
// the Lds route's three kernels: k_fft_tiny, else k_fft_small (sub-64-byte rows per transform, and the packed real
// transforms up to 256 bins, whose pair maps store 8-byte pieces: coalesced staging through LDS), else k_fft_lds
constexpr bool lds_tiny(int logn, int mode) { return logn <= 2 && mode == MODE_C2C; }
constexpr bool lds_small(int logn, int mode) { return logn >= 2 && (logn <= 6 || (mode != MODE_C2C && logn <= 8)); }
constexpr int fft_mode(const FftShape &s) { return !s.real ? MODE_C2C : s.fwd ? MODE_R2C : MODE_C2R; }

constexpr const char *route_kernel_name(FftRoute r, const FftShape &s) {
  switch (r) {
    case FftRoute::Lds: return lds_tiny(s.logn, fft_mode(s)) ? "k_fft_tiny" : lds_small(s.logn, fft_mode(s)) ? "k_fft_small" : "k_fft_lds";
    case FftRoute::Cfft2x13: return "k_cfft_2x";
    case FftRoute::Rfft2x13:
    case FftRoute::Rfft2x14: return "k_rfft_2x";
    case FftRoute::FourStepSpread: return "k_fft_4step_cols";
    case FftRoute::FourStep: return "k_fft_4step";
    case FftRoute::Res16:
    case FftRoute::RealRes16: return "k_fft_res16";
    case FftRoute::Big: return s.logn <= kBig2MaxLog ? "k_big2_cols" : "k_big_cols";   // two passes / three
    case FftRoute::BlueLds: return "k_blue_lds";
    case FftRoute::Bluestein: return "bluestein";
  }
  return "";
}

// real plans: the reference's pack / unpack is a pass of its own around the complex transform
constexpr bool route_pack_apart(FftRoute r) {
  return r != FftRoute::Lds && r != FftRoute::Rfft2x13 && r != FftRoute::Rfft2x14 && r != FftRoute::RealRes16;
}
// the route touches its source and its destination once each: a pinned host array may then run zero-copy
constexpr bool route_one_touch(FftRoute r, bool real) {
  return r != FftRoute::Big && r != FftRoute::BlueLds && r != FftRoute::Bluestein && !(real && route_pack_apart(r));
}

// what a route needs of its plan (the Bluestein routes keep their chirp, filter and sub-plans apart; real plans add w2)
enum FftNeed : unsigned {
  kNeedHalf = 1,      // FftTables::half of the length: W_n^k, k < n / 2 to n = 4096, the lane tables for n = 8192
  kNeedHalf2x = 2,    // ... of the half-length runs: the n = 8192 lane tables + W_16384^t (logn 14), the n = 16384 ones (logn 15)
  kNeedFour = 4,      // the four-step tables
  kNeedRes16 = 8,     // the resident kernel's tables
  kNeedFourWs = 16,   // a workspace of num_cus transforms (the resident kernel's slots are its first part;
                      // a complex n = 65536 plan appends kRes16CtrBytes: the shared assignment's counters)
  kNeedBig = 32       // the big-N tables and a workspace of one chunk, and what the routes of the row transform need
};
constexpr unsigned route_needs(FftRoute r) {
  switch (r) {
    case FftRoute::Lds: return kNeedHalf;
    case FftRoute::Cfft2x13:
    case FftRoute::Rfft2x13:
    case FftRoute::Rfft2x14: return kNeedHalf2x;
    case FftRoute::FourStepSpread:
    case FftRoute::FourStep: return kNeedFour | kNeedFourWs;
    case FftRoute::Res16:
    case FftRoute::RealRes16: return kNeedRes16 | kNeedFourWs;
    case FftRoute::Big: return kNeedBig;
    default: return 0;
  }
}
constexpr unsigned fft_needs(const FftShape &s) {
  unsigned needs = 0;
  for (int r = 0; r <= (int)FftRoute::Bluestein; r++)
    if (fft_routes(s) >> r & 1) needs |= route_needs((FftRoute)r);
  return needs;
}

}  // namespace clfa
