// bank_plan.hpp — the host side of the filter bank on (amp, freq) frames (clfa_pvoc_bank_setup, include/clfft_amd.h) that
// needs no device (plain C++: tests/test_pvoc_bank_cpu.py builds it with g++): the validation of a bank, the schedule that
// deals its bands to the sixteen rows of k_pvoc_bands (bank_kernels.hip), and the DCT table.  pvoc_rows_host.cpp uploads what
// these make.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace clfa {

constexpr int kBankMax = 256;    // the most bands of a bank
constexpr int kBankRows = 16;    // rows of 16 lanes in a workgroup of k_pvoc_bands: a row takes a band at a time
constexpr int kBankLanes = 16;   // the lanes of the tree sum S16

// a band as the kernel reads it: its bins first .. first + count - 1, its weights at woff of the bank's weights
struct BankBand {
  int first, count, woff, pad;
};

// The rules of a bank over the bins 0 .. M: 1 <= nbands <= 256, every band inside the bins with at least one, every
// weight finite.  The ranges are checked before any weight is read: the weights are sum(count) values.
inline bool bank_ok(int M, int nbands, const int *first, const int *count, const float *weights) {
  if (nbands < 1 || nbands > kBankMax || !first || !count || !weights) return false;
  long total = 0;
  for (int b = 0; b < nbands; b++) {
    if (count[b] < 1 || first[b] < 0 || (long)first[b] + count[b] > (long)M + 1) return false;
    total += count[b];
  }
  for (long i = 0; i < total; i++)
    if (!std::isfinite(weights[i])) return false;
  return true;
}

// the bands with where their weights start
inline std::vector<BankBand> bank_bands(int nbands, const int *first, const int *count) {
  std::vector<BankBand> v(nbands);
  int woff = 0;
  for (int b = 0; b < nbands; b++) {
    v[b] = BankBand{first[b], count[b], woff, 0};
    woff += count[b];
  }
  return v;
}

// The schedule: kBankRows + 1 starts, then the nbands band numbers, row r taking sched[kBankRows + 1 + n] for
// sched[r] <= n < sched[r + 1] in that order.  Longest band first, each to the row with the fewest steps so far (a step:
// 16 bins; the lowest row on a tie), so the n-th bands of the four rows of a wave are of similar length and the rows end
// together.  The results do not depend on it: a band's sum is formed by one row, whichever.
inline std::vector<int> bank_schedule(int nbands, const int *count) {
  std::vector<int> order(nbands);
  for (int b = 0; b < nbands; b++) order[b] = b;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count[a] > count[b]; });
  std::vector<int> rows[kBankRows];
  long load[kBankRows] = {};
  for (int b : order) {
    int r = 0;
    for (int i = 1; i < kBankRows; i++)
      if (load[i] < load[r]) r = i;
    rows[r].push_back(b);
    load[r] += (count[b] + kBankLanes - 1) / kBankLanes;
  }
  std::vector<int> sched(kBankRows + 1, 0);
  for (int r = 0; r < kBankRows; r++) {
    sched[r + 1] = sched[r] + (int)rows[r].size();
    sched.insert(sched.end(), rows[r].begin(), rows[r].end());
  }
  return sched;
}

// D[q][b] = (float)(s_q cos(pi q (2b + 1) / (2B))), s_0 = sqrt(1 / B), s_q = sqrt(2 / B): the orthonormal DCT-II, in double
inline std::vector<float> bank_dct(int B) {
  const double pi = 3.141592653589793;
  std::vector<float> D((size_t)B * B);
  for (int q = 0; q < B; q++) {
    const double s = std::sqrt((q ? 2.0 : 1.0) / B);
    for (int b = 0; b < B; b++) D[(size_t)q * B + b] = (float)(s * std::cos(pi * q * (2 * b + 1) / (2.0 * B)));
  }
  return D;
}

}  // namespace clfa
