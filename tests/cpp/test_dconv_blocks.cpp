// C++ surface check for the extension members of cl_conv::Cldconv: several channels, whole signals per call
// (convolution_blocks), the block-wise calls on a multi-channel object, and the two-input "loop" route, against
// float64 evaluations of y_c[t] = sum_k h_c[k] x_c[t - 1 - k] (cl_dconv.cpp:32-43).
#include <cl_dconv.h>

#include <cmath>
#include <iostream>
#include <vector>

int main() {
  cl_device_id ids[32];
  cl_uint num = 0;
  if (clGetDeviceIDs(NULL, CL_DEVICE_TYPE_ALL, 32, ids, &num) != CL_SUCCESS) return 2;
  const int irsize = 300, vsize = 8, channels = 3, nblocks = 50, L = vsize * nblocks;
  cl_conv::Cldconv dc(ids[0], irsize, vsize, channels, NULL, NULL);
  if (dc.get_cl_err() != CL_SUCCESS) return 1;
  if (dc.channels() != channels || std::string(dc.blocks_kernel_name()) != "k_dconvb_fir" ||
      std::string(dc.blocks_kernel_name(true)) != "loop")
    return 1;
  unsigned s = 11;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) / 16777216.f - 0.5f; };
  std::vector<float> h(channels * irsize), x(channels * (L + vsize)), y(channels * L), y1(channels * vsize);
  for (auto &v : h) v = rnd();
  for (auto &v : x) v = rnd();
  if (dc.push_ir(h.data()) != CL_SUCCESS) return 1;
  // the whole signal in two calls (rows contiguous per call), then one more block through convolution()
  const int n0 = 7, n1 = nblocks - n0;
  std::vector<float> xa(channels * n0 * vsize), xb(channels * n1 * vsize), xc(channels * vsize);
  std::vector<float> ya(xa.size()), yb(xb.size());
  for (int c = 0; c < channels; c++) {
    for (int i = 0; i < n0 * vsize; i++) xa[c * n0 * vsize + i] = x[c * (L + vsize) + i];
    for (int i = 0; i < n1 * vsize; i++) xb[c * n1 * vsize + i] = x[c * (L + vsize) + n0 * vsize + i];
    for (int i = 0; i < vsize; i++) xc[c * vsize + i] = x[c * (L + vsize) + L + i];
  }
  if (dc.convolution_blocks(ya.data(), xa.data(), NULL, n0) != CL_SUCCESS) return 1;
  if (dc.convolution_blocks(yb.data(), xb.data(), NULL, n1) != CL_SUCCESS) return 1;
  if (dc.wp() != L % (irsize + vsize)) return 1;
  if (dc.convolution(y1.data(), xc.data()) != CL_SUCCESS) return 1;
  int bad = 0;
  auto want = [&](int c, int t) {
    double w = 0;
    for (int k = 0; k < irsize; k++)
      if (t - 1 - k >= 0) w += (double)h[c * irsize + k] * x[c * (L + vsize) + t - 1 - k];
    return w;
  };
  for (int c = 0; c < channels; c++) {
    for (int t = 0; t < L; t++) {
      const float got = t < n0 * vsize ? ya[c * n0 * vsize + t] : yb[c * n1 * vsize + t - n0 * vsize];
      if (std::fabs(want(c, t) - got) > 1e-5) bad++;
    }
    for (int i = 0; i < vsize; i++)
      if (std::fabs(want(c, L + i) - y1[c * vsize + i]) > 1e-5) bad++;
  }
  // two inputs on a fresh object: block 0 meets the coefficients in2's first block wrote at ring indices 0..7 (the rest
  // of the ring is zero) and a delay ring that holds in1's first block: y[t] = sum_{k < 8} in2[k] in1[t - 1 - k]
  cl_conv::Cldconv tv(ids[0], 16, 8, 2, NULL, NULL);
  std::vector<float> a(2 * 24), b(2 * 24), o(2 * 24);
  for (auto &v : a) v = rnd();
  for (auto &v : b) v = rnd();
  if (tv.convolution_blocks(o.data(), a.data(), b.data(), 3) != CL_SUCCESS) return 1;
  if (tv.wp() != 0) return 1;   // 3 blocks of 8 = one ring cycle of 24
  for (int c = 0; c < 2; c++)
    for (int t = 0; t < 8; t++) {
      double w = 0;
      for (int k = 0; k < 8 && t - 1 - k >= 0; k++) w += (double)b[c * 24 + k] * a[c * 24 + t - 1 - k];
      if (std::fabs(w - o[c * 24 + t]) > 1e-6) bad++;
    }
  if (dc.convolution_blocks(ya.data(), ya.data(), NULL, n0) != CL_INVALID_VALUE) bad++;   // out == in
  if (bad) {
    std::cout << bad << " mismatches" << std::endl;
    return 1;
  }
  std::cout << "OK" << std::endl;
  return 0;
}
