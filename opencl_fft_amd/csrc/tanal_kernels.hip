// tanal_kernels.hip — the phase-vocoder analysis of a STORED signal at any time points (clfa_pvoc_tanal_dev,
// include/clfft_amd.h; Csound's pvstanal / mincer).
//
//   k_pvoc_tanal   one launch per call.  Output frame (c, g) is windowed twice straight from the signal: A at
//                  starts[g] - hop and B at starts[g] (samples outside the row are +0: a clamped address and a select,
//                  no branch per element).  Each goes through stft_spectrum.inc (the pass chain, the
//                  scale and the pair map of k_stft_analyze), z of A is kept in a second LDS buffer of FPW x (N + 1) bins
//                  (as k_pvoc_formant keeps its frames), and pvoc_analysis_bin.inc (the per-bin conversion
//                  of k_pvoc_analyze) turns the pair into (amp, freq).  Rows of consecutive bins go out, 8 bytes per lane,
//                  non-temporal.  No spectra in memory, no gathered copy of the signal, no state, no atomics.
//
// A workgroup holds FPW = LdsGeom::FPW output frames at once (frame index b = c * Fout + g) and walks the groups
// grid-stride.  One register buffer of E samples per lane is always one transform ahead: B's rows fly behind A's passes,
// the next group's A rows behind B's.  LDS: the exchange buffer (FPW x PADN), z of A (FPW x (N + 1)) and, up to n = 4096,
// the two twiddle tables; at n = 8192 the tables come from L1/L2, as in k_stft_synth and k_pvoc_formant (70 + 64 KiB of
// buffers leave no room for 64 KiB of tables).
#include "pvoc_analysis.hpp"
#include "fft_wg.hpp"
#include "tanal_launch.hpp"

namespace clfa {

namespace {

template <int LOGN> constexpr bool tanal_tab_lds() { return LOGN <= 12; }

// float t of a window whose floats [lo, hi) lie in the row (`none`: no float does), +0 for the others: the address is
// clamped to a float of the window that does lie in the row (base = the window's first sample; the row's where none), the
// value selected.  Offsets of 32 bits from one base per window: no 64-bit arithmetic per float.
__device__ __forceinline__ float tanal_ld(const float *__restrict__ base, int t, int lo, int hi, bool none) {
  const bool in = t >= lo && t < hi;
  const int tc = t < lo ? lo : (t < hi ? t : hi - 1);
  const float v = base[none ? 0 : tc];
  return in ? v : 0.f;
}

__device__ __forceinline__ void tanal_st_nt8(cpx *p, cpx v) {
  __builtin_nontemporal_store(*reinterpret_cast<unsigned long long *>(&v), reinterpret_cast<unsigned long long *>(p));
}

}  // namespace

template <int LOGN>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_pvoc_tanal(const float *__restrict__ sig, long stride, long samples,
                                                                  int hop, const int *__restrict__ starts, unsigned Fout,
                                                                  long nframes, const float *__restrict__ win,
                                                                  cpx *__restrict__ out, const cpx *__restrict__ etab,
                                                                  float sh, float srs, const cpx *__restrict__ tab_g,
                                                                  const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW, B = N + 1;   // M = N, B bins per frame
  constexpr bool TL = tanal_tab_lds<LOGN>();
  static_assert(FPW * N == WG * E, "one chunk = E rows of WG elements");
  __shared__ cpx s_tab_l[TL ? G::HALF : 1];
  __shared__ cpx s_w2_l[TL ? N / 2 : 1];
  __shared__ cpx s_x[FPW * G::PADN];   // the exchange buffer: the windowed frames, then their packed spectra
  __shared__ cpx s_za[FPW * B];        // z of the earlier windows
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  if constexpr (TL) {
    for (int i = tid; i < N / 2; i += WG) {
      s_tab_l[i] = tab_g[i];
      s_w2_l[i] = w2_g[i];
    }
  }
  const cpx *s_tab = TL ? s_tab_l : tab_g, *s_w2 = TL ? s_w2_l : w2_g;   // the names stft_spectrum.inc reads
  cpx *xb = s_x + f * G::PADN;
  const long groups = (nframes + FPW - 1) / FPW;
  long g = blockIdx.x;
  if (g >= groups) return;
  // element tid + WG e of a chunk: frame (tid + WG e) >> LOGN of the group, complex position (tid + WG e) & (N - 1) — the
  // same positions for every group, so the lane's window values are loaded once and stay in registers
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
  // the windows of group grp that start `back` samples before starts[g]: hop for A, 0 for B
  auto load_rows = [&](long grp, int back) {
    const long b0 = grp * FPW, c0 = b0 / (long)Fout;
    const unsigned g0 = (unsigned)(b0 - c0 * (long)Fout);
    const int last = nframes - 1 - b0 < FPW - 1 ? (int)(nframes - 1 - b0) : FPW - 1;   // ragged last group: clamped
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int idx = tid + WG * e;
      const int fr = (idx >> LOGN) < last ? (idx >> LOGN) : last;
      const unsigned q = g0 + (unsigned)fr, dc = q / Fout, gi = q - dc * Fout;   // frame b0 + fr = (c0 + dc) Fout + gi
      const float *row = sig + (c0 + (long)dc) * stride;
      const long n0 = (long)starts[gi] - back, lo64 = -n0, hi64 = samples - n0;   // the window's first sample; its floats
      const int lo = lo64 < 0 ? 0 : (lo64 > 2 * N ? 2 * N : (int)lo64);           // [lo, hi) lie in the row
      const int hi = hi64 < 0 ? 0 : (hi64 > 2 * N ? 2 * N : (int)hi64);
      const bool none = hi <= lo;
      const float *base = none ? row : row + n0;
      const int t0 = 2 * (idx & (N - 1));
      raw[e] = mk(tanal_ld(base, t0, lo, hi, none), tanal_ld(base, t0 + 1, lo, hi, none));
    }
  };
  load_rows(g, hop);
  __syncthreads();
#pragma unroll 1
  for (; g < groups; g += gridDim.x) {
    const long b0 = g * FPW;
    const int live = (nframes - b0 < FPW ? (int)(nframes - b0) : FPW) * B;
    // A: fl(w[t] * x[s - hop + t]) per float, before the first pass; B's rows fly behind A's passes
#pragma unroll
    for (int e = 0; e < E; e++) park(e) = mk(wr[e].x * raw[e].x, wr[e].y * raw[e].y);
    load_rows(g, 0);
    __syncthreads();
    {
#include "stft_spectrum.inc"
    }
    for (int idx = tid; idx < live; idx += WG) {
      const int fi = idx / B, k = idx - fi * B;
      s_za[idx] = pvoc_bin_of(s_x[fi * G::PADN + lds_pad(k == N ? 0 : k)], k, N);
    }
    __syncthreads();   // zA is kept before B is parked over A's spectrum
    // B: fl(w[t] * x[s + t]); the next group's A rows fly behind B's passes
#pragma unroll
    for (int e = 0; e < E; e++) park(e) = mk(wr[e].x * raw[e].x, wr[e].y * raw[e].y);
    {
      const long gn = g + gridDim.x;
      load_rows(gn < groups ? gn : groups - 1, hop);
    }
    __syncthreads();
    {
#include "stft_spectrum.inc"
    }
    for (int idx = tid; idx < live; idx += WG) {
      const int fi = idx / B, k = idx - fi * B;
      const cpx z = pvoc_bin_of(s_x[fi * G::PADN + lds_pad(k == N ? 0 : k)], k, N), zp = s_za[idx], e = etab[k];
#include "pvoc_analysis_bin.inc"
      tanal_st_nt8(out + b0 * B + idx, mk(amp, freq));
    }
    __syncthreads();   // the results are out before the next group is parked
  }
}

template <int LOGN>
static hipError_t launch_pvoc_tanal_n(const PvocTanalArgs &a, const DeviceInfo &di, hipStream_t s) {
  using G = LdsGeom<LOGN>;
  static int occ = 0;
  if (!occ) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_pvoc_tanal<LOGN>, G::WG, 0) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    occ = nb;
  }
  const long nframes = (long)a.channels * a.Fout;
  const long groups = (nframes + G::FPW - 1) / G::FPW;
  long cap = (long)di.num_cus * occ;
  if (a.grid_max > 0 && cap > a.grid_max) cap = a.grid_max;   // CLFA_PVOC_OPS_GRID_MAX
  const int grid = (int)(groups < cap ? groups : cap);
  hipLaunchKernelGGL((k_pvoc_tanal<LOGN>), dim3(grid), dim3(G::WG), 0, s, a.signal, a.stride, a.samples, a.hop, a.starts,
                     (unsigned)a.Fout, nframes, a.window, a.out, a.etab, a.sh, a.srs, a.half, a.w2);
  return hipGetLastError();
}

hipError_t launch_pvoc_tanal(const PvocTanalArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.Fout <= 0 || a.channels <= 0) return hipSuccess;
  switch (a.logn) {
#define CLFA_N(L) \
  case L: return launch_pvoc_tanal_n<L>(a, di, s);
    CLFA_N(5) CLFA_N(6) CLFA_N(7) CLFA_N(8) CLFA_N(9) CLFA_N(10) CLFA_N(11) CLFA_N(12) CLFA_N(13)
#undef CLFA_N
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace clfa
