// fft_tables.hpp — the exact host tables only the FFT kernels read (four-step, lane-addressed, resident n = 65536, big
// sizes), built from host.hpp's fill_twiddle; for clfft_amd.cpp and pconv_host.cpp, the two files that create FFT plans'
// tables.  The tables every object shares (fill_twiddle, fill_w2, upload_half, upload_w2) stay in host.hpp.
#pragma once
#include "fft_launch.hpp"
#include "host.hpp"

namespace clfa {

// host tables of the four-step kernel: [half N1 | half N2 | lo: W_n^k, k < 2^loglo | hi: W_n^(k 2^loglo)]
inline void fill_fourstep_tables(std::vector<cpx> &all, int logn) {
  int l1, l2, llo;
  fourstep_split(logn, &l1, &l2, &llo);
  const int n = 1 << logn, n1 = 1 << l1, n2 = 1 << l2, lo = 1 << llo, hi = n >> llo;
  std::vector<cpx> part;
  all.clear();
  fill_twiddle(part, n1 / 2, n1, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + n1 / 2);
  fill_twiddle(part, n2 / 2, n2, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + n2 / 2);
  fill_twiddle(part, lo, n, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + lo);
  fill_twiddle(part, hi, n, lo, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + hi);
}

// lane-addressed tables of the two-level LDS transforms (fft_launch.hpp, kLane13Size / kLane14Size), every value rounded
// from double: [W_256^(j t), j, t < 16 | W_4096^(2^k j mod 4096), k < 4, j < 256 | tail].  The tail: logn 13 W_8192^t,
// t < 512 — with tail2x followed by W_16384^t, t < 512, the radix-2 step's lane constants of k_cfft_2x / k_rfft_2x<13>;
// logn 14 W_16384^(m t), m = 1, 2, 3, t < 1024
inline void fill_lane_tables(std::vector<cpx> &h, int logn, bool tail2x) {
  h.clear();
  auto w = [&](long k, long n) { h.push_back(mk((float)cos(k * 2 * kPI / n), -(float)sin(k * 2 * kPI / n))); };
  for (int j = 0; j < 16; j++)
    for (int t = 0; t < 16; t++) w(j * t, 256);
  for (int k = 0; k < 4; k++)
    for (int j = 0; j < 256; j++) w(((1 << k) * j) & 4095, 4096);
  if (logn == kLds14Log) {
    for (int m = 1; m <= 3; m++)
      for (int t = 0; t < 1024; t++) w(m * t, 16384);
    return;
  }
  for (int t = 0; t < 512; t++) w(t, 8192);
  for (int t = 0; tail2x && t < 512; t++) w(t, 16384);
}

// host tables of the resident n = 65536 kernel (fft_launch.hpp, kRes16TabSize), each value rounded from
// double like the reference's table (cl_fft.cpp:89-90)
inline void fill_res16_tables(std::vector<cpx> &all) {
  all.clear();
  std::vector<cpx> part;
  for (int t = 0; t < 16; t++)
    for (int j = 0; j < 16; j++) all.push_back(mk((float)cos((t * j) * 2 * kPI / 256), -(float)sin((t * j) * 2 * kPI / 256)));
  fill_twiddle(part, 256, 65536, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + 256);
  fill_twiddle(part, 256, 256, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + 256);
  for (int m = 1; m <= 8; m *= 2)
    for (int k = 0; k < 256; k++) {
      const int idx = (m * k) & 4095;
      all.push_back(mk((float)cos(idx * 2 * kPI / 4096), -(float)sin(idx * 2 * kPI / 4096)));
    }
}

// host tables of n = 2^17 .. 2^24 = N1 x N2 (fft_launch.hpp, launch_fft_big): [half N1 | W_n^e0 | W_n^(128 e1) |
// W_n^(16384 e2)], e = e0 + 128 e1 + 16384 e2 (big_tw(), fft_big.inc)
inline void fill_big_tables(std::vector<cpx> &all, int n, int n1) {
  std::vector<cpx> part;
  all.clear();
  fill_twiddle(part, n1 / 2, n1, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + n1 / 2);
  fill_twiddle(part, 128, n, 1, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + 128);
  fill_twiddle(part, 128, n, 128, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + 128);
  fill_twiddle(part, n / 16384, n, 16384, -1.f);
  all.insert(all.end(), part.begin(), part.begin() + n / 16384);
}

}  // namespace clfa
