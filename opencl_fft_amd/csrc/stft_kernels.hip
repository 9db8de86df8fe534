// stft_kernels.hip — short-time analysis and windowed overlap-add synthesis (clfa_stft, include/clfft_amd.h).
//
//   k_stft_analyze  one launch per call: frame (c, f) = the window times x_c[f*hop ..] read straight from the signal
//                   (no framed copy), the packed real transform of the Clrfft route of that size, spectra out;
//   k_stft_synth    one launch per call: c2r of a run of consecutive frames, the synthesis window in registers, the
//                   overlap-add in an LDS ring in ascending frame order, normalisation in the pass that writes.
//
// Both drive the shared pass chain of the single-workgroup LDS FFT (fft_wg.hpp: pass_gather_padded, wg_passes,
// dif_scatter_padded) with the reference's pair maps (r2c_pair / c2r_pair, cl_fft.cpp:178-205) on the natural-order LDS
// copy — the recipe of k_fft_small (fft_lds.inc), for every packed size 64..16384 (complex n = 32..8192).  A workgroup
// holds FPW = LdsGeom::FPW frames at once; global accesses go in chunk order (element tid + WG e of the FPW * n
// elements), so a wave reads runs of whole frames.
#include "fft_wg.hpp"
#include "stft_launch.hpp"
#include "stft_plan.hpp"

namespace clfa {

namespace {

// start of frame b = c * F + f (in floats from the signal's start)
__device__ __forceinline__ long stft_frame_off(unsigned b, unsigned F, long stride, int hop) {
  const unsigned c = b / F, f = b - c * F;
  return (long)c * stride + (long)f * hop;
}

// one complex sample (two consecutive floats) of the signal: an 8-byte load where frame starts are 8-byte aligned,
// two 4-byte loads otherwise (odd hop, odd stride or a 4-byte aligned signal).  Plain loads: the frames overlap by
// (size - hop) / size, and the re-reads are meant to hit the on-die caches.
template <bool A8> __device__ __forceinline__ cpx stft_ld(const float *p) {
  if constexpr (A8) return *reinterpret_cast<const cpx *>(p);
  else return mk(p[0], p[1]);
}

__device__ __forceinline__ void st_nt8(cpx *p, cpx v) {
  __builtin_nontemporal_store(*reinterpret_cast<unsigned long long *>(&v), reinterpret_cast<unsigned long long *>(p));
}

}  // namespace

// grid-stride over groups of FPW consecutive frames (frame index b = c * F + f): the workgroups in flight at once hold
// neighbouring frames of the same rows, so the overlapping samples are re-read from L2 / MALL, not from HBM
template <int LOGN, bool A8>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_stft_analyze(const float *__restrict__ sig, long stride, int hop,
                                                                    int F, int nframes, const float *__restrict__ win,
                                                                    cpx *__restrict__ out, const cpx *__restrict__ tab_g,
                                                                    const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW, CHUNK = FPW * N;
  static_assert(CHUNK == WG * E, "one chunk = E rows of WG elements");
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_w2[N / 2];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) {
    s_tab[i] = tab_g[i];
    s_w2[i] = w2_g[i];
  }
  cpx *xb = s_x + f * G::PADN;
  const long groups = (nframes + FPW - 1) / FPW;
  long g = blockIdx.x;
  if (g >= groups) return;
  // element tid + WG e of a chunk: frame (tid + WG e) >> LOGN of the group, position (tid + WG e) & (N - 1) — the same
  // positions for every group, so the lane's window values are loaded once and stay in registers
  cpx wr[E], raw[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int p = (tid + WG * e) & (N - 1);
    wr[e] = mk(win[2 * p], win[2 * p + 1]);
  }
  auto park = [&](int e) -> cpx & {
    const int idx = tid + WG * e;
    return s_x[(idx >> LOGN) * G::PADN + lds_pad(idx & (N - 1))];
  };
  auto load_rows = [&](long grp) {
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int idx = tid + WG * e;
      long b = grp * FPW + (idx >> LOGN);
      b = b < nframes ? b : nframes - 1;   // ragged last group: clamped, straight-line
      raw[e] = stft_ld<A8>(sig + stft_frame_off((unsigned)b, (unsigned)F, stride, hop) + 2 * (idx & (N - 1)));
    }
  };
  load_rows(g);
  __syncthreads();
#pragma unroll 1
  for (; g < groups; g += gridDim.x) {
    // the window in registers, fl(w[t] * x[t]) per float, before the first pass
#pragma unroll
    for (int e = 0; e < E; e++) park(e) = mk(wr[e].x * raw[e].x, wr[e].y * raw[e].y);
    {  // the next group's frames fly behind this one's passes
      const long gn = g + gridDim.x;
      load_rows(gn < groups ? gn : groups - 1);
    }
    __syncthreads();
#include "stft_spectrum.inc"   // the pass chain, the scale by 1 / N, the r2c pair map: the spectra are in the slots
    const long base = g * CHUNK, total = (long)nframes * N;
    if (base + CHUNK <= total) {
#pragma unroll
      for (int e = 0; e < E; e++) st_nt8(out + base + tid + WG * e, park(e));
    } else {
#pragma unroll
      for (int e = 0; e < E; e++)
        if (base + tid + WG * e < total) out[base + tid + WG * e] = park(e);
    }
    __syncthreads();   // the results are out before the next group is parked
  }
}

// Work item = a run [s, e) of consecutive frames of one channel; it owns the output samples [s hop, e hop) (the
// channel's last run: up to L).  The frames before s that reach into the run's first sample are transformed again
// (ceil(size / hop) - 1 of them), so every sample is summed by ONE workgroup, over its frames in ascending order, from
// zero: no atomics, no partial sums to combine, bit-identical across calls, streams and graph replay.  The sums live
// in a ring of RL = FPW * size floats in LDS (sample p at p mod RL): after a group of frames [a, a + nv) has been added,
// the samples below (a + nv) hop are complete, are written out (divided by the window envelope if asked) and their
// slots zeroed for the samples size later.
template <int LOGN> constexpr bool stft_synth_tab_lds() { return LOGN <= 12; }   // n = 8192: tables from L1/L2 (LDS budget)
template <int LOGN>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_stft_synth(const cpx *__restrict__ spec, int F, int runs, int nf,
                                                                  int hop, long L, const float *__restrict__ win,
                                                                  const double *__restrict__ cum, int normalize,
                                                                  float *__restrict__ out, long stride, long items,
                                                                  const cpx *__restrict__ tab_g,
                                                                  const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW, CHUNK = FPW * N, SIZE = 2 * N;
  constexpr int RL = 2 * CHUNK;   // ring length in floats = FPW * size >= (FPW - 1) hop + size
  constexpr bool TL = stft_synth_tab_lds<LOGN>();
  static_assert(CHUNK == WG * E, "one chunk = E rows of WG elements");
  static_assert(FPW == stft_fpw(SIZE), "stft_plan.hpp restates FPW for the host");
  __shared__ cpx s_tab[TL ? G::HALF : 1];
  __shared__ cpx s_w2[TL ? N / 2 : 1];
  __shared__ cpx s_x[FPW * G::PADN];
  __shared__ float s_ring[RL];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  if constexpr (TL) {
    for (int i = tid; i < N / 2; i += WG) {
      s_tab[i] = tab_g[i];
      s_w2[i] = w2_g[i];
    }
  }
  const cpx *tab = TL ? s_tab : tab_g, *w2 = TL ? s_w2 : w2_g;
  cpx *xb = s_x + f * G::PADN;
  const float *xf = reinterpret_cast<const float *>(s_x);
  // the synthesis window of the lane's output positions p = t + T e (floats 2p, 2p + 1), in registers
  cpx wr[E];
#pragma unroll
  for (int e = 0; e < E; e++) wr[e] = mk(win[2 * (t + T * e)], win[2 * (t + T * e) + 1]);
  auto park = [&](int e) -> cpx & {
    const int idx = tid + WG * e;
    return s_x[(idx >> LOGN) * G::PADN + lds_pad(idx & (N - 1))];
  };
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const long c = item / runs;
    const int r = (int)(item - c * runs);
    const StftRun run = stft_run(r, nf, F, SIZE, hop);   // (stft_plan.hpp)
    const int e_end = run.e_end, fw = run.fw;            // fw: the first frame that reaches sample s hop
    const bool last = e_end == F;
    const long own_lo = run.own_lo;
    const cpx *sp = spec + (long)c * F * N;
    float *orow = out + c * stride;
    for (int i = tid; i < RL; i += WG) s_ring[i] = 0.f;
    // (the ring's zeroing and the first park are ordered by the barrier after the park)
#pragma unroll 1
    for (int a = fw; a < e_end; a += FPW) {
      const int nv = e_end - a < FPW ? e_end - a : FPW;
      cpx raw[E];
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int idx = tid + WG * e, fr = idx >> LOGN;
        raw[e] = sp[(long)(a + (fr < nv ? fr : nv - 1)) * N + (idx & (N - 1))];
      }
#pragma unroll
      for (int e = 0; e < E; e++) park(e) = raw[e];
      __syncthreads();
      // reference `iconv` (cl_fft.cpp:192-205) on the natural-order copy
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        const int i = t + T * k, j = i == 0 ? N / 2 : N - i;
        const cpx ci = xb[lds_pad(i)], cj = xb[lds_pad(j)];
        cpx oi, oj;
        c2r_pair(ci, cj, w2[i], oi, oj);
        const bool z = i == 0;
        oi = mk(z ? ci.x + ci.y : oi.x, z ? ci.x - ci.y : oi.y);
        oj = mk(z ? cj.x : oj.x, z ? cj.y : oj.y);
        xb[lds_pad(i)] = oi;
        xb[lds_pad(j)] = oj;
      }
      __syncthreads();
      cpx v[E];
      pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
      wg_passes<LOGN, G::LOGE, 0, false>(v, t, tab, xb);
      // synthesis window, fl(w[t] * r[t]), in registers
#pragma unroll
      for (int e = 0; e < E; e++) v[e] = mk(wr[e].x * v[e].x, wr[e].y * v[e].y);
      __syncthreads();
      dif_scatter_padded<LOGN, G::LOGE>(v, t, xb);
      __syncthreads();
      // overlap-add of the group's frames into the ring: sample a hop + q takes frames j_lo .. j_hi in ascending order
      const long p0 = (long)a * hop;
      const int span = (nv - 1) * hop + SIZE;
      for (int q = tid; q < span; q += WG) {
        const int jh = q / hop < nv - 1 ? q / hop : nv - 1;
        const int jl = q < SIZE ? 0 : (q - SIZE) / hop + 1;
        float *slot = s_ring + ((p0 + q) & (RL - 1));
        float acc = *slot;
        for (int j = jl; j <= jh; j++) {
          const int d = q - j * hop;
          acc += xf[2 * (j * G::PADN + lds_pad(d >> 1)) + (d & 1)];
        }
        *slot = acc;
      }
      __syncthreads();
      // complete samples out: [a hop, (a + nv) hop), or to the row's end after the channel's last frame
      const long hi = (last && a + nv == e_end) ? L : p0 + (long)nv * hop;
      for (long p = p0 + tid; p < hi; p += WG) {
        float *slot = s_ring + (p & (RL - 1));
        float y = *slot;
        *slot = 0.f;
        if (p >= own_lo) {
          if (normalize) {
            // env[p], the float64 sum of w^2 over the covering frames rounded once (stft_plan.hpp)
            const float en = stft_env_at(cum, SIZE, hop, F, p);
            if (en > 1e-11f) y = y / en;
          }
          orow[p] = y;
        }
      }
      __syncthreads();
    }
  }
}

template <int LOGN>
static int stft_occupancy(const void *k, int wg) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, wg, 0) != hipSuccess || nb < 1) {
    (void)hipGetLastError();
    nb = 1;
  }
  return nb;
}

template <int LOGN>
static hipError_t launch_stft_analyze_n(const StftArgs &a, const DeviceInfo &di, hipStream_t s) {
  using G = LdsGeom<LOGN>;
  const long groups = (a.nframes + G::FPW - 1) / G::FPW;
  static int occ8 = 0, occ4 = 0;
  if (!occ8) occ8 = stft_occupancy<LOGN>((const void *)k_stft_analyze<LOGN, true>, G::WG);
  if (!occ4) occ4 = stft_occupancy<LOGN>((const void *)k_stft_analyze<LOGN, false>, G::WG);
  const long cap = (long)di.num_cus * (a.aligned8 ? occ8 : occ4);
  int grid = (int)(groups < cap ? groups : cap);
  if (a.grid_max > 0 && grid > a.grid_max) grid = a.grid_max;   // CLFA_STFT_GRID_MAX
  if (a.aligned8)
    hipLaunchKernelGGL((k_stft_analyze<LOGN, true>), dim3(grid), dim3(G::WG), 0, s, a.signal, a.stride, a.hop, a.F,
                       (int)a.nframes, a.window, a.spec_out, a.half, a.w2);
  else
    hipLaunchKernelGGL((k_stft_analyze<LOGN, false>), dim3(grid), dim3(G::WG), 0, s, a.signal, a.stride, a.hop, a.F,
                       (int)a.nframes, a.window, a.spec_out, a.half, a.w2);
  return hipGetLastError();
}

template <int LOGN>
static hipError_t launch_stft_synth_n(const StftArgs &a, const DeviceInfo &di, hipStream_t s) {
  using G = LdsGeom<LOGN>;
  static int occ = 0;
  if (!occ) occ = stft_occupancy<LOGN>((const void *)k_stft_synth<LOGN>, G::WG);
  const long slots = (long)di.num_cus * occ;
  const int size = 2 * G::N;
  // the runs (stft_plan.hpp) depend on the device's slots alone, never on the cap of the grid
  const int nf = stft_run_frames(a.nframes, slots, size, a.hop, G::FPW, a.F);
  const int runs = stft_runs(a.F, nf);
  const long items = a.channels * runs;
  int grid = (int)(items < slots ? items : slots);
  if (a.grid_max > 0 && grid > a.grid_max) grid = a.grid_max;   // CLFA_STFT_GRID_MAX
  const long L = (long)(a.F - 1) * a.hop + size;
  hipLaunchKernelGGL((k_stft_synth<LOGN>), dim3(grid), dim3(G::WG), 0, s, a.spec_in, a.F, runs, nf, a.hop,
                     L, a.window, a.cum, a.normalize, a.out, a.stride, items, a.half, a.w2);
  return hipGetLastError();
}

hipError_t launch_stft(const StftArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.nframes <= 0) return hipSuccess;
  switch (a.logn) {
#define CLFA_N(L) \
  case L: return a.forward ? launch_stft_analyze_n<L>(a, di, s) : launch_stft_synth_n<L>(a, di, s);
    CLFA_N(5) CLFA_N(6) CLFA_N(7) CLFA_N(8) CLFA_N(9) CLFA_N(10) CLFA_N(11) CLFA_N(12) CLFA_N(13)
#undef CLFA_N
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace clfa
