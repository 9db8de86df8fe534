// pvoc_env.hpp — the cepstral envelope of (amp, freq) frames held in LDS (env of include/clfft_amd.h), shared by
// k_pvoc_formant (pvoc_ops.hip), k_pvoc_vocode (pvoc_pair.hip) and k_pvoc_warp (pvoc_shape.hip).  A workgroup of
// LdsGeom<LOGN>::WG lanes works FPW = LdsGeom::FPW frames of B = N + 1 bins at once (N = M = size / 2), frame fi in
// slot fi of the exchange buffer:
//   (1) L[k] = logf(fmaxf(amp[k], 1e-20f)) lands at samples k and size - k of the slot: the even extension Lext;
//   (2) the packed forward real transform of Lext on the pass chain of k_stft_analyze, scaled by 1 / N;
//   (3) the pair step: forward pair map, zeros above coefs and in the Nyquist half of bin 0, inverse pair map, in one
//       visit of every pair (i, N - i);
//   (4) the unscaled inverse on the chain of k_stft_synth;
//   (5) expf turns the first B samples of the slot into env, in place.
// What the three kernels share besides the stages: the bounds of a group of frames (PvocEnvGroup) and, on the host, their
// launch (launch_pvoc_env under pvoc_env_dispatch).  The __shared__ arrays, the staging of the twiddle tables into them
// and the loop over the groups stay in each kernel: a shared function changes the LDS layout or the staging's
// instructions (at n = 1024..4096 its two ds_write_b64 become one ds_write2st64_b64).
#pragma once
#include <type_traits>

#include "fft_wg.hpp"
#include "pvoc_device.hpp"

namespace clfa {

// n = 8192 reads its twiddle tables from L1/L2 (pvoc_ops.hip)
template <int LOGN> constexpr bool pvoc_env_tab_lds() { return LOGN <= 12; }

// Group g of FPW consecutive frames out of nframes: its first frame, its frames (fewer in a ragged last group, whose other
// slots run the chain on stale LDS and write nothing) and its bins
template <int LOGN> struct PvocEnvGroup {
  long b0;
  int nv, live;
  __device__ __forceinline__ PvocEnvGroup(long g, long nframes) {
    constexpr int FPW = LdsGeom<LOGN>::FPW;
    b0 = g * FPW;
    nv = nframes - b0 < FPW ? (int)(nframes - b0) : FPW;
    live = nv * (LdsGeom<LOGN>::N + 1);
  }
};

// One launch of an envelope kernel over the groups of nframes frames, as many workgroups as stay resident (asked once per
// kernel); args: the kernel's own
template <int LOGN, auto Kernel, class... Args>
static hipError_t launch_pvoc_env(long nframes, int grid_max, const DeviceInfo &di, hipStream_t s, Args... args) {
  using G = LdsGeom<LOGN>;
  static int occ = 0;
  if (!occ) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)Kernel, G::WG, 0) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    occ = nb;
  }
  const long groups = (nframes + G::FPW - 1) / G::FPW;
  const int grid = pvoc_grid(groups, (long)di.num_cus * occ, grid_max);
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(G::WG), 0, s, args...);
  return hipGetLastError();
}

// launch(std::integral_constant<int, LOGN>()) for logn = log2(size / 2) of the nine sizes
template <class Launch>
static hipError_t pvoc_env_dispatch(int logn, Launch launch) {
  switch (logn) {
#define CLFA_N(L) \
  case L: return launch(std::integral_constant<int, L>());
    CLFA_N(5) CLFA_N(6) CLFA_N(7) CLFA_N(8) CLFA_N(9) CLFA_N(10) CLFA_N(11) CLFA_N(12) CLFA_N(13)
#undef CLFA_N
    default:
      return hipErrorInvalidValue;
  }
}

template <int LOGN> struct PvocEnv {
  using G = LdsGeom<LOGN>;
  static constexpr int N = G::N, B = N + 1;
  static constexpr int ELEMS = G::FPW * B;                      // bins of a full group
  static constexpr int ITERS = (ELEMS + G::WG - 1) / G::WG;     // bins per lane: element idx = tid + i WG, i < ITERS
  // sample n of frame fi's real sequence (floats 2p, 2p + 1 of complex element p, padded)
  static __device__ __forceinline__ float &sample(cpx *s_x, int fi, int n) {
    return reinterpret_cast<float *>(s_x)[2 * (fi * G::PADN + lds_pad(n >> 1)) + (n & 1)];
  }
};

// Stages (1) to (5) for the `live` = frames x B bins of a group.  amp(idx) reads element idx (frame idx / B, bin
// idx % B) from memory, keeps what its kernel needs of it and returns the amplitude; it is called once per live
// element, by lane idx % WG.
// s_x must be free on entry (a barrier since its last use); on return env is in place and a barrier has passed.  The
// slots of a ragged group's missing frames run the chain on stale LDS.
template <int LOGN, class Amp>
__device__ __forceinline__ void pvoc_envelope(cpx *s_x, const cpx *tab, const cpx *w2, int coefs, int live, Amp amp) {
  using G = LdsGeom<LOGN>;
  using P = PvocEnv<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, B = P::B;
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  cpx *xb = s_x + f * G::PADN;
  for (int idx = tid; idx < live; idx += WG) {
    const int fi = idx / B, k = idx - fi * B;
    const float L = logf(fmaxf(amp(idx), 1e-20f));   // fmaxf(NaN, floor) = floor
    P::sample(s_x, fi, k) = L;
    if (k > 0 && k < N) P::sample(s_x, fi, 2 * N - k) = L;
  }
  __syncthreads();
  cpx v[E];
  pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
  wg_passes<LOGN, G::LOGE, 0, true>(v, t, tab, xb);
#pragma unroll
  for (int e = 0; e < E; e++) v[e] = cscale(v[e], 1.0f / (float)N);   // forward real plans scale by 1/M
  __syncthreads();
  dif_scatter_padded<LOGN, G::LOGE>(v, t, xb);
  __syncthreads();
  // one visit of every pair (i, N - i): the forward pair map (k_stft_analyze), the lifter on the packed bins, the
  // inverse pair map (k_stft_synth; its table is the forward one conjugated)
#pragma unroll
  for (int k = 0; k < E / 2; k++) {
    const int i = t + T * k, j = i == 0 ? N / 2 : N - i;
    const cpx ci = xb[lds_pad(i)], cj = xb[lds_pad(j)];
    const cpx w = w2[i];
    const bool z = i == 0;
    cpx oi, oj;
    r2c_pair(ci, cj, w, oi, oj);
    oi = mk(z ? (ci.x + ci.y) * .5f : oi.x, z ? 0.f : oi.y);   // bin 0 = (DC, Nyquist): the Nyquist half goes
    oj = mk(z ? cj.x : oj.x, z ? cj.y : oj.y);
    if (i > coefs) oi = mk(0.f, 0.f);
    if (j > coefs) oj = mk(0.f, 0.f);
    cpx ni, nj;
    c2r_pair(oi, oj, mk(w.x, -w.y), ni, nj);
    ni = mk(z ? oi.x + oi.y : ni.x, z ? oi.x - oi.y : ni.y);
    nj = mk(z ? oj.x : nj.x, z ? oj.y : nj.y);
    xb[lds_pad(i)] = ni;
    xb[lds_pad(j)] = nj;
  }
  __syncthreads();
  pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
  wg_passes<LOGN, G::LOGE, 0, false>(v, t, tab, xb);
  __syncthreads();
  dif_scatter_padded<LOGN, G::LOGE>(v, t, xb);
  __syncthreads();
  // env[k] = expf(logE[k]), k = 0..M, in place
  for (int idx = tid; idx < live; idx += WG) {
    const int fi = idx / B, k = idx - fi * B;
    float &e = P::sample(s_x, fi, k);
    e = expf(e);
  }
  __syncthreads();
}

}  // namespace clfa
