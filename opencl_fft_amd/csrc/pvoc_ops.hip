// pvoc_ops.hip — operations on the (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): pitch scale, frequency shift
// and timed read.  All three are stateless, one launch per call, deterministic (gathers: no atomics).  The tile kernels'
// prologue and launch (pvoc_bin, pvoc_tiles) are pvoc_device.hpp's, as in the other Pvoc kernel files; the envelope
// kernel's launch and size dispatch (launch_pvoc_env, pvoc_env_dispatch) are pvoc_env.hpp's.
//
//   k_pvoc_map      scale and shift without keepform: a lane takes output bin j of one frame, finds its source bin and
//                   writes the pair; rows of consecutive bins, 8 bytes per lane, no LDS.
//   k_pvoc_read     the frame sequence read at the positions pos[g]: a copy of frame i or the interpolation of frames
//                   i and i + 1; rows of consecutive bins, 8 bytes per lane.
//   k_pvoc_formant  scale and shift with keepform.  A workgroup holds FPW = LdsGeom::FPW frames: each frame is read once
//                   into LDS (the pairs, and the logs of its amps as the even extension Lext), the packed forward real
//                   transform of Lext runs on the pass chain of k_stft_analyze, the pair step lifters (forward pair map,
//                   zeros above coefs, inverse pair map in one visit of the pair), the inverse runs on the chain of
//                   k_stft_synth, expf turns the first M + 1 samples into env in place (these stages are
//                   pvoc_envelope of pvoc_env.hpp, which k_pvoc_vocode shares), and the map gathers amp, freq
//                   and the two envelope values from LDS.  One read and one write of the frame, no workspace.  n = 8192
//                   reads its twiddle tables from L1/L2 (k_stft_synth's LDS budget: here 70 KiB of exchange buffer and
//                   64 KiB of frame leave no room for 48 KiB of tables).
//
// Every float32 step of the definitions is rounded on its own: the device functions below switch contraction off, as
// pvoc_inc does (pvoc_kernels.hip).  tests/pvoc_ops_model.py restates them.
#include "pvoc_device.hpp"
#include "pvoc_env.hpp"

namespace clfa {

namespace {

constexpr int kOpsWG = 256;            // lanes = bins per workgroup tile (k_pvoc_map, k_pvoc_read)

// source bin of output bin j: k in 1..M-1, kSrcEmpty, or kSrcCopy (the bin is handed over unchanged).  The scale map's
// gather is pvoc_scale_source (pvoc_device.hpp).
__device__ __forceinline__ int pvoc_source(int op, int j, int M, int lowest, float par, float bpf) {
#pragma clang fp contract(off)
  if (j == 0 || j == M) return kSrcCopy;
  if (op == PVOC_SCALE) return pvoc_scale_source(j, M, par);
  if (j < lowest) return kSrcCopy;
  const float t = par * bpf;
  if (!(fabsf(t) <= (float)M)) return kSrcEmpty;   // past every bin, or not a number
  const int k = j - (int)rintf(t);
  return (k >= lowest && k <= M - 1) ? k : kSrcEmpty;
}

// (amp, freq) of a bin that takes source sv; amp is the finished amplitude
__device__ __forceinline__ cpx pvoc_moved(int op, cpx sv, float par, float amp) {
#pragma clang fp contract(off)
  return mk(amp, op == PVOC_SCALE ? sv.y * par : sv.y + par);
}

__device__ __forceinline__ float pvoc_gain(float gain, float amp) {
#pragma clang fp contract(off)
  return gain * amp;
}

__device__ __forceinline__ float pvoc_keepform(float gain, float amp, float env_k, float env_j) {
#pragma clang fp contract(off)
  const float g = gain * amp;
  const float w = g / env_k;
  return w * env_j;
}

__device__ __forceinline__ cpx pvoc_lerp(cpx x0, cpx x1, float a) {
#pragma clang fp contract(off)
  const float dx = x1.x - x0.x, dy = x1.y - x0.y;
  const float px = a * dx, py = a * dy;
  return mk(x0.x + px, x0.y + py);
}

}  // namespace

// item -> (channel, frame f, bin tile), the tile fastest
__global__ __launch_bounds__(kOpsWG) void k_pvoc_map(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                     const float *__restrict__ par, long F, int M, int tiles, long items,
                                                     int op, int lowest, float gain, float cf, float bpf) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int j;
    long f, c;
    if (!pvoc_bin<kOpsWG>(item, tiles, F, M, j, f, c)) continue;
    const long b = c * F + f;
    const float s = par[f];
    const cpx *row = in + b * (M + 1);
    const int src = pvoc_source(op, j, M, lowest, s, bpf);
    cpx o;
    if (src == kSrcCopy) o = row[j];
    else if (src == kSrcEmpty) o = pvoc_empty(j, cf);
    else {
      const cpx sv = row[src];
      o = pvoc_moved(op, sv, s, pvoc_gain(gain, sv.x));
    }
    out[b * (M + 1) + j] = o;
  }
}

// item -> (channel, output frame g, bin tile), the tile fastest
__global__ __launch_bounds__(kOpsWG) void k_pvoc_read(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                      const float *__restrict__ pos, long Fin, long Fout, int M,
                                                      int tiles, long items) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int j;
    long g, c;
    if (!pvoc_bin<kOpsWG>(item, tiles, Fout, M, j, g, c)) continue;
    const long b = c * Fout + g;
    const float p = fminf(fmaxf(pos[g], 0.f), (float)(Fin - 1));   // fmaxf(NaN, 0) = 0
    const long i = (long)floorf(p);
    const float a = p - (float)i;
    const long i1 = i + 1 < Fin ? i + 1 : Fin - 1;
    const cpx x0 = in[(c * Fin + i) * (M + 1) + j];
    cpx o = x0;
    if (a != 0.f) o = pvoc_lerp(x0, in[(c * Fin + i1) * (M + 1) + j], a);   // a == 0: frame i1 is not read at all
    out[b * (M + 1) + j] = o;
  }
}

// grid-stride over groups of FPW consecutive frames (frame index b = c * F + f; the frames are contiguous)
template <int LOGN>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_pvoc_formant(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                                    const float *__restrict__ par, long F, long nframes,
                                                                    int op, int lowest, int coefs, float gain, float cf,
                                                                    float bpf, const cpx *__restrict__ tab_g,
                                                                    const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  using P = PvocEnv<LOGN>;
  constexpr int N = G::N, WG = G::WG, FPW = G::FPW, B = N + 1;   // M = N, B bins per frame
  constexpr bool TL = pvoc_env_tab_lds<LOGN>();
  __shared__ cpx s_tab[TL ? G::HALF : 1];
  __shared__ cpx s_w2[TL ? N / 2 : 1];
  __shared__ cpx s_x[FPW * G::PADN];   // the exchange buffer: Lext, its spectrum, logE, env
  __shared__ cpx s_fr[FPW * B];        // the group's frames as read
  const int tid = threadIdx.x;
  if constexpr (TL) {
    for (int i = tid; i < N / 2; i += WG) {
      s_tab[i] = tab_g[i];
      s_w2[i] = w2_g[i];
    }
  }
  const cpx *tab = TL ? s_tab : tab_g, *w2 = TL ? s_w2 : w2_g;
  auto sample = [&](int fi, int n) -> float & { return P::sample(s_x, fi, n); };
  const long groups = (nframes + FPW - 1) / FPW;
#pragma unroll 1
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const PvocEnvGroup<LOGN> grp(g, nframes);
    const long b0 = grp.b0;
    const int live = grp.live;
    // the frames in, once: the pairs stay in s_fr, the envelope of their amps lands in s_x (pvoc_env.hpp)
    pvoc_envelope<LOGN>(s_x, tab, w2, coefs, live, [&](int idx) {
      const cpx af = in[b0 * B + idx];
      s_fr[idx] = af;
      return af.x;
    });
    for (int idx = tid; idx < live; idx += WG) {
      const int fi = idx / B, j = idx - fi * B;
      const float s = par[(b0 + fi) % F];
      const int src = pvoc_source(op, j, N, lowest, s, bpf);
      cpx o;
      if (src == kSrcCopy) o = s_fr[idx];
      else if (src == kSrcEmpty) o = pvoc_empty(j, cf);
      else {
        const cpx sv = s_fr[fi * B + src];
        o = pvoc_moved(op, sv, s, pvoc_keepform(gain, sv.x, sample(fi, src), sample(fi, j)));
      }
      out[b0 * B + idx] = o;
    }
    __syncthreads();   // the group is out before the next one lands in s_fr and s_x
  }
}

hipError_t launch_pvoc_ops(const PvocOpsArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.op != PVOC_READ && a.keepform) {
    const long nframes = (long)a.channels * a.F;
    return pvoc_env_dispatch(a.logn, [&](auto L) {
      constexpr int LOGN = decltype(L)::value;
      return launch_pvoc_env<LOGN, k_pvoc_formant<LOGN>>(nframes, a.grid_max, di, s, a.in, a.out, a.par, a.F, nframes, a.op,
                                                         a.lowest, a.coefs, a.gain, a.cf, a.bpf, a.half, a.w2);
    });
  }
  const PvocTiles t = pvoc_tiles(a.M, kOpsWG, (long)a.channels * a.F, di, 16, a.grid_max);
  if (a.op == PVOC_READ)
    hipLaunchKernelGGL(k_pvoc_read, dim3(t.grid), dim3(kOpsWG), 0, s, a.in, a.out, a.par, a.Fin, a.F, a.M, t.tiles, t.items);
  else
    hipLaunchKernelGGL(k_pvoc_map, dim3(t.grid), dim3(kOpsWG), 0, s, a.in, a.out, a.par, a.F, a.M, t.tiles, t.items, a.op,
                       a.lowest, a.gain, a.cf, a.bpf);
  return hipGetLastError();
}

}  // namespace clfa
