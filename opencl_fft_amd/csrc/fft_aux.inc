// fft_aux.inc (part of the translation unit fft_kernels.hip) — the FFT's element-wise kernels for gfx950 (MI355X):
//   k_r2c_pack / k_c2r_unpack, k_reorder  stand-alone forms of the reference's
//                conv / iconv / reorder kernels;
//   k_blue_pre / k_blue_mul / k_blue_post, k_blue_lds  Bluestein's algorithm for lengths that are no power of two.
#include "fft_wg.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// stand-alone pack / unpack / reorder
// ---------------------------------------------------------------------------------

// reference conv (cl_fft.cpp:178-191) over a batch; thread per pair
__global__ __launch_bounds__(256) void k_r2c_pack(cpx *__restrict__ data, const cpx *__restrict__ w2, int m,
                                                  long total_pairs, long out_off) {
  const int hp = m / 2;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total_pairs; g += (long)gridDim.x * 256) {
    long b = g / hp;
    int i = (int)(g % hp);
    const cpx *c = data + b * m;
    cpx *o = data + b * m + out_off;   // out_off = 0: in place
    if (i == 0) {
      cpx z = c[0];
      o[0] = mk((z.x + z.y) * .5f, (z.x - z.y) * .5f);
      if (out_off) o[hp] = c[hp];   // the bin the reference never visits (cl_fft.cpp:278) travels as it is
    } else {
      cpx oi, oj;
      r2c_pair(c[i], c[m - i], w2[i], oi, oj);
      o[i] = oi;
      o[m - i] = oj;
    }
  }
}
// reference iconv (cl_fft.cpp:192-205)
__global__ __launch_bounds__(256) void k_c2r_unpack(cpx *__restrict__ data, const cpx *__restrict__ w2, int m,
                                                    long total_pairs, long out_off) {
  const int hp = m / 2;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total_pairs; g += (long)gridDim.x * 256) {
    long b = g / hp;
    int i = (int)(g % hp);
    const cpx *c = data + b * m;
    cpx *o = data + b * m + out_off;
    if (i == 0) {
      cpx z = c[0];
      o[0] = mk(z.x + z.y, z.x - z.y);
      if (out_off) o[hp] = c[hp];
    } else {
      cpx oi, oj;
      c2r_pair(c[i], c[m - i], w2[i], oi, oj);
      o[i] = oi;
      o[m - i] = oj;
    }
  }
}

static int grid_for(long items) {
  long g = (items + 255) / 256;
  if (g > 256 * 32) g = 256 * 32;
  if (g < 1) g = 1;
  return (int)g;
}

hipError_t launch_r2c_pack(cpx *data, const cpx *w2, int m, long batch, hipStream_t s, long out_off) {
  long pairs = batch * (m / 2);
  if (pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_r2c_pack, dim3(grid_for(pairs)), dim3(256), 0, s, data, w2, m, pairs, out_off);
  return hipGetLastError();
}
hipError_t launch_c2r_unpack(cpx *data, const cpx *w2, int m, long batch, hipStream_t s, long out_off) {
  long pairs = batch * (m / 2);
  if (pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_c2r_unpack, dim3(grid_for(pairs)), dim3(256), 0, s, data, w2, m, pairs, out_off);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// arbitrary lengths (extension, SURVEY 8f row 4): Bluestein's chirp-z over the power-of-two kernels
// ---------------------------------------------------------------------------------
// The reference only knows powers of two (its callers pad, opcode.cpp:30-35).  For any other n,
//   X[k] = w[k] * sum_j (x[j] w[j]) conj(w)[k - j],   w[j] = exp(-+ i pi j^2 / n),
// a circular convolution of length m = 2^ceil(log2(2n - 1)): pre-multiply and zero-pad into the workspace,
// m-point forward transform (scaled 1/m), times B = DFT_m(conj(w) wrapped), m-point inverse transform
// (unscaled), post-multiply (and 1/n for forward plans).  Tables w, B come from the host in double.
__global__ __launch_bounds__(256) void k_blue_pre(const cpx *__restrict__ x, const cpx *__restrict__ w, cpx *__restrict__ a,
                                                  int n, int m, long total) {
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long b = g / m;
    const int j = (int)(g - b * m);
    a[g] = j < n ? cmul(x[b * n + j], w[j]) : mk(0.f, 0.f);
  }
}
__global__ __launch_bounds__(256) void k_blue_mul(cpx *__restrict__ a, const cpx *__restrict__ bt, int m, long total) {
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) a[g] = cmul(a[g], bt[g % m]);
}
__global__ __launch_bounds__(256) void k_blue_post(const cpx *__restrict__ a, const cpx *__restrict__ w, cpx *__restrict__ x,
                                                   int n, int m, float scale, long total) {
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long b = g / n;
    const int k = (int)(g - b * n);
    x[g] = cscale(cmul(a[b * m + k], w[k]), scale);
  }
}
// Bluestein in ONE launch for m <= 8192 (n <= 4096): a transform's chirp multiply, m-point forward transform, multiply by
// the chirp's spectrum, m-point inverse transform and second chirp multiply all happen in the registers + LDS of one
// workgroup, on the pass chains of k_fft_lds (same tables: the m-point plan's) — one read and one write of the data where
// the composed form (pre, plan, mul, plan, post) makes five passes over a zero-padded copy.  In place (x == y) is fine:
// a transform is read completely before any of it is written.
template <int LOGM>
__global__ __launch_bounds__(LdsGeom<LOGM>::WG, LdsGeom<LOGM>::MIN_WAVES) void k_blue_lds(const cpx *__restrict__ x, cpx *__restrict__ y,
                                                              const cpx *__restrict__ w, const cpx *__restrict__ bt,
                                                              const cpx *__restrict__ tab_g, int n, float scale, long batch) {
  using G = LdsGeom<LOGM>;
  constexpr int M = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW;
  static_assert(G::LOGE == 4 && LOGM >= 8 && LOGM <= 13, "16 points per lane");
  constexpr bool TWO = kLdsTwoLevel(LOGM);
  __shared__ cpx s_tab[TWO ? kLaneLds : G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = FPW == 1 ? 0 : tid / T, t0 = FPW == 1 ? tid : tid % T;
  for (int i = tid; i < (TWO ? kLane13Lds : M / 2); i += WG) s_tab[TWO ? lane_lds_index(i) : i] = tab_g[i];
  cpx wl = mk(1.f, 0.f);
  if constexpr (TWO) wl = tab_g[kLane13Lds + t0];
  cpx *xb = s_x + f * G::PADN;
  const long groups = (batch + FPW - 1) / FPW;
  __syncthreads();
#pragma unroll 1
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    int t = t0;   // opaque per iteration (see k_fft_lds)
    asm volatile("" : "+v"(t));
    const auto tab = [&]() {
      if constexpr (TWO) return LaneTab13{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl};
      else return static_cast<const cpx *>(s_tab);
    }();
    long b = g * FPW + f;
    b = b < batch ? b : batch - 1;   // lanes of a ragged last group redo the last transform (identical stores)
    const cpx *xi = x + b * (long)n;
    cpx v[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int j = t + T * e;
      v[e] = j < n ? cmul(xi[j], w[j]) : mk(0.f, 0.f);
    }
    wg_passes<LOGM, 4, 0, true>(v, t, tab, xb);
#pragma unroll
    for (int e = 0; e < E; e++) v[e] = cmul(v[e], bt[t + T * e]);
    wg_passes<LOGM, 4, 0, false>(v, t, tab, xb);
    cpx *yo = y + b * (long)n;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = t + T * e;
      if (k < n) yo[k] = cscale(cmul(v[e], w[k]), scale);
    }
  }
}
template <int LOGM>
static hipError_t launch_blue_lds_m(const cpx *x, cpx *y, const cpx *w, const cpx *bt, const cpx *tab, int n, float scale,
                                    long batch, const DeviceInfo &di, hipStream_t s) {
  using G = LdsGeom<LOGM>;
  const long groups = (batch + G::FPW - 1) / G::FPW;
  static int occ = 0;
  if (occ == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_blue_lds<LOGM>, G::WG, 0) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    occ = nb;
  }
  const long cap = (long)di.num_cus * occ;
  const int grid = (int)(groups < cap ? groups : cap);
  hipLaunchKernelGGL((k_blue_lds<LOGM>), dim3(grid < 1 ? 1 : grid), dim3(G::WG), 0, s, x, y, w, bt, tab, n, scale, batch);
  return hipGetLastError();
}
// x -> y (may be equal), batch transforms of n points; w = chirp (n), bt = its padded spectrum (m), tab = the m-point plan's
// LDS table (FftTables::half); scale = the plan's output factor times 1 / m
hipError_t launch_blue_lds(int m, const cpx *x, cpx *y, const cpx *w, const cpx *bt, const cpx *tab, int n, float scale,
                           long batch, const DeviceInfo &di, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  switch (m) {
    case 256: return launch_blue_lds_m<8>(x, y, w, bt, tab, n, scale, batch, di, s);
    case 512: return launch_blue_lds_m<9>(x, y, w, bt, tab, n, scale, batch, di, s);
    case 1024: return launch_blue_lds_m<10>(x, y, w, bt, tab, n, scale, batch, di, s);
    case 2048: return launch_blue_lds_m<11>(x, y, w, bt, tab, n, scale, batch, di, s);
    case 4096: return launch_blue_lds_m<12>(x, y, w, bt, tab, n, scale, batch, di, s);
    case 8192: return launch_blue_lds_m<13>(x, y, w, bt, tab, n, scale, batch, di, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_blue_pre(const cpx *x, const cpx *w, cpx *a, int n, int m, long batch, hipStream_t s) {
  const long total = batch * m;
  hipLaunchKernelGGL(k_blue_pre, dim3(grid_for(total)), dim3(256), 0, s, x, w, a, n, m, total);
  return hipGetLastError();
}
hipError_t launch_blue_mul(cpx *a, const cpx *bt, int m, long batch, hipStream_t s) {
  const long total = batch * m;
  hipLaunchKernelGGL(k_blue_mul, dim3(grid_for(total)), dim3(256), 0, s, a, bt, m, total);
  return hipGetLastError();
}
hipError_t launch_blue_post(const cpx *a, const cpx *w, cpx *x, int n, int m, float scale, long batch, hipStream_t s) {
  const long total = batch * n;
  hipLaunchKernelGGL(k_blue_post, dim3(grid_for(total)), dim3(256), 0, s, a, w, x, n, m, scale, total);
  return hipGetLastError();
}

// reference reorder (cl_fft.cpp:24-27): out[k] = in[bitrev(k)].  The table of
// cl_fft.cpp:96-101 is exactly the log2(n)-bit reversal, computed here with
// v_bfrev_b32 instead of a table read.
__global__ __launch_bounds__(256) void k_reorder(cpx *__restrict__ out, const cpx *__restrict__ in, int logn,
                                                 long total) {
  const unsigned mask = (1u << logn) - 1u;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    unsigned k = (unsigned)g & mask;
    unsigned r = __brev(k) >> (32 - logn);
    out[g] = in[(g - k) + r];
  }
}

hipError_t launch_reorder(cpx *out, const cpx *in, int logn, long batch, hipStream_t s) {
  long total = batch << logn;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_reorder, dim3(grid_for(total)), dim3(256), 0, s, out, in, logn, total);
  return hipGetLastError();
}

}  // namespace clfa
