// pvoc_shape.hip — operations that reshape ONE stream of (amp, freq) frames of clfa_pvoc along the bins
// (include/clfft_amd.h): band pass / reject, table mask, stencil, arpeggiator, peak frequency lock and the warp of the
// spectral envelope.  Stateless, one launch per call, no atomics; the tile kernels' prologue and launch (pvoc_bin,
// pvoc_tiles) and the pitch scale's source map are pvoc_device.hpp's, the warp's launch and size dispatch
// (launch_pvoc_env, pvoc_env_dispatch) pvoc_env.hpp's.  par: F rows of 4 floats, one per frame.
//
//   k_pvoc_shape  band, mask, stencil, arp: a lane takes bin k of one frame, reads its pair and writes one pair; rows of
//                 consecutive bins, 8 bytes in and 8 out per lane, no LDS.  The op is a kernel argument: every lane of a
//                 launch takes the same branch.
//   k_pvoc_lock   the same items.  A locked frame's tile of 256 pairs goes through LDS with a halo of 3 bins on either
//                 side (lanes 0..5 fetch it), so that a lane finds the amps j-3..j+3 and the freqs j-1..j+1 of its row
//                 there, across tile boundaries; the halo's 48 bytes per 2 KiB tile are the only bytes read twice, and
//                 they hit in L2.  A frame with lock == 0 is copied bin by bin, without LDS and without a barrier (the
//                 frame belongs to the item, so the branch is the workgroup's).
//   k_pvoc_warp   a workgroup holds FPW = LdsGeom::FPW frames: the envelope stages of k_pvoc_formant (pvoc_envelope,
//                 pvoc_env.hpp), the pairs staying in LDS, then the rule bin by bin from the pairs and the envelope
//                 samples.  One read and one write of the frame, no workspace; LDS is k_pvoc_formant's (n = 8192 reads
//                 its twiddle tables from L1/L2).
//
// Every float32 step of the definitions is rounded on its own: the device functions below switch contraction off.
// tests/pvoc_shape_model.py restates them.
#include "pvoc_device.hpp"
#include "pvoc_env.hpp"

namespace clfa {

namespace {

constexpr int kShapeWG = 256;   // lanes = bins per workgroup tile (k_pvoc_shape, k_pvoc_lock)
constexpr int kLockHalo = 3;    // bins on either side of a tile that k_pvoc_lock's lanes look at

// the band's gain at |freq| = x; (lc, lf, hf, hc): the row
__device__ __forceinline__ float pvoc_band_gain(float x, float lc, float lf, float hf, float hc, int reject) {
#pragma clang fp contract(off)
  float g = 0.f;
  if (lc <= lf && lf <= hf && hf <= hc && x >= lc && x <= hc) {   // a comparison with a NaN is false
    if (x < lf) {
      const float n = x - lc, d = lf - lc;
      g = n / d;
    } else if (x <= hf) {
      g = 1.f;
    } else {
      const float n = hc - x, d = hc - hf;
      g = n / d;
    }
  }
  return reject ? 1.f - g : g;
}

// one bin of ops 0..3; r: the frame's row, tab: table[k] (0 where the op reads no table)
__device__ __forceinline__ cpx pvoc_shape_bin(int op, cpx v, const float *r, float tab, int k, int M, int reject) {
#pragma clang fp contract(off)
  if (op == PVOC_BAND) {
    const float g = pvoc_band_gain(fabsf(v.y), r[0], r[1], r[2], r[3], reject);
    const float x = v.x * g;
    return mk(g == 1.f ? v.x : (g == 0.f ? 0.f : x), v.y);   // g == 0: the input is not used
  }
  if (op == PVOC_MASK) {
    const float d = pvoc_clamp01(r[0]);
    const float u = 1.f - d, w = d * tab;
    const float m = u + w;
    const float x = v.x * m;
    return mk(d == 0.f ? v.x : x, v.y);
  }
  if (op == PVOC_STENCIL) {
    const float thr = tab * r[1];
    const float x = v.x * r[0];
    return mk(v.x < thr ? x : v.x, v.y);   // a comparison with a NaN is false
  }
  // PVOC_ARP
  const float pos = pvoc_clamp01(r[0]) * (float)M;
  const int t = (int)floorf(pos);
  const float m = 1.f - pvoc_clamp01(r[1]);
  const float x = v.x * r[2], y = v.x * m;
  return mk(k == t ? x : (m == 1.f ? v.x : y), v.y);
}

// the lock's freq of bin j given the freq Fc of the peak next to it
__device__ __forceinline__ float pvoc_lock_freq(float fj, float Fc, float tol) {
#pragma clang fp contract(off)
  const float d = tol * fabsf(Fc);
  const float e = fj - Fc;
  return fabsf(e) < d ? Fc : fj;
}

// the warp's source of bin j, lowest <= j <= M-1: the scale map's source of bin j - d, or kSrcEmpty (the frame is not
// warped, j - d is no bin 1..M-1 of the scale map, or no k reaches it)
__device__ __forceinline__ int pvoc_warp_source(int j, int M, float s, float shift, float bpf) {
#pragma clang fp contract(off)
  const float t = shift * bpf;
  if (!(s >= 0.25f && s <= 4.f) || !(fabsf(t) <= (float)M)) return kSrcEmpty;   // a NaN fails either test
  const int jj = j - (int)rintf(t);
  if (jj < 1 || jj > M - 1) return kSrcEmpty;
  return pvoc_scale_source(jj, M, s);
}

__device__ __forceinline__ float pvoc_warp_amp(float gain, float amp, bool moved, float env_j, float env_k) {
#pragma clang fp contract(off)
  const float g = gain * amp;
  const float w = g / env_j;
  const float x = w * env_k;
  return moved ? x : g;
}

}  // namespace

// item -> (channel, frame f, bin tile), the tile fastest.  table: NULL for the ops that read none
__global__ __launch_bounds__(kShapeWG) void k_pvoc_shape(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                         const float *__restrict__ par, const float *__restrict__ table,
                                                         long F, int M, int tiles, long items, int op, int reject) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long f, c;
    if (!pvoc_bin<kShapeWG>(item, tiles, F, M, k, f, c)) continue;
    const long e = (c * F + f) * (M + 1) + k;
    float r[4] = {0.f, 0.f, 0.f, 0.f};   // the columns the op names
    const int cols = op == PVOC_BAND ? 4 : (op == PVOC_MASK ? 1 : (op == PVOC_STENCIL ? 2 : 3));
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < cols) r[i] = par[4 * f + i];
    const float tab = (op == PVOC_MASK || op == PVOC_STENCIL) ? table[k] : 0.f;
    out[e] = pvoc_shape_bin(op, in[e], r, tab, k, M, reject);
  }
}

// item -> (channel, frame f, bin tile), the tile fastest.  s_t[i] is bin k0 - kLockHalo + i of the item's row
__global__ __launch_bounds__(kShapeWG) void k_pvoc_lock(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                        const float *__restrict__ par, long F, int M, int tiles,
                                                        long items) {
  __shared__ cpx s_t[kShapeWG + 2 * kLockHalo];
  const int tid = threadIdx.x;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int tile;
    long f, c;
    pvoc_item(item, tiles, F, tile, f, c);   // not pvoc_bin: the lanes past bin M fetch the halo and keep the barriers
    const int k0 = tile * kShapeWG, j = k0 + tid;
    const cpx *row = in + (c * F + f) * (M + 1);
    cpx *orow = out + (c * F + f) * (M + 1);
    const float lock = par[4 * f], tol = par[4 * f + 1];
    if (!(lock != 0.f)) {   // the whole workgroup: the frame is the item's.  A NaN locks
      if (j <= M) orow[j] = row[j];
      continue;
    }
    cpx v = mk(0.f, 0.f);
    if (j <= M) v = row[j];
    s_t[tid + kLockHalo] = v;
    if (tid < 2 * kLockHalo) {   // the halo; what lies outside the row is never looked at (a peak is 2..M-2)
      const bool left = tid < kLockHalo;
      const int h = left ? k0 - kLockHalo + tid : k0 + kShapeWG + tid - kLockHalo;
      s_t[left ? tid : kShapeWG + tid] = (h >= 0 && h <= M) ? row[h] : mk(0.f, 0.f);
    }
    __syncthreads();
    if (j <= M) {
      // bin c is a peak: 2 <= c <= M-2 and its amp strictly above the two on either side (a NaN: false)
      auto peak = [&](int cc) {
        if (cc < 2 || cc > M - 2) return false;
        const int i = cc - k0 + kLockHalo;
        const float a = s_t[i].x;
        return a > s_t[i - 2].x && a > s_t[i - 1].x && a > s_t[i + 1].x && a > s_t[i + 2].x;
      };
      if (j >= 1 && j <= M - 1) {
        const int cand = peak(j + 1) ? j + 1 : (peak(j - 1) ? j - 1 : -1);
        if (cand >= 0) v.y = pvoc_lock_freq(v.y, s_t[cand - k0 + kLockHalo].y, tol);
      }
      orow[j] = v;
    }
    __syncthreads();   // the tile is done with before the next item lands in s_t
  }
}

// grid-stride over groups of FPW consecutive frames (frame index b = c * F + f; the frames are contiguous)
template <int LOGN>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_pvoc_warp(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                                 const float *__restrict__ par, long F, long nframes,
                                                                 int lowest, int coefs, float bpf,
                                                                 const cpx *__restrict__ tab_g,
                                                                 const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  using P = PvocEnv<LOGN>;
  constexpr int N = G::N, WG = G::WG, FPW = G::FPW, B = P::B;   // M = N, B bins per frame
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
  const long groups = (nframes + FPW - 1) / FPW;
#pragma unroll 1
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const PvocEnvGroup<LOGN> grp(g, nframes);
    const long b0 = grp.b0;
    const int live = grp.live;
    pvoc_envelope<LOGN>(s_x, tab, w2, coefs, live, [&](int idx) {
      const cpx af = in[b0 * B + idx];
      s_fr[idx] = af;
      return af.x;
    });
    for (int idx = tid; idx < live; idx += WG) {
      const int fi = idx / B, j = idx - fi * B;
      cpx o = s_fr[idx];
      if (j >= lowest && j < N) {   // lowest >= 1; bins 0, M and those below lowest are copies
        const float *r = par + 4 * ((b0 + fi) % F);
        const int src = pvoc_warp_source(j, N, r[0], r[1], bpf);
        const bool moved = src != kSrcEmpty;
        o.x = pvoc_warp_amp(r[2], o.x, moved, P::sample(s_x, fi, j), P::sample(s_x, fi, moved ? src : j));
      }
      out[b0 * B + idx] = o;
    }
    __syncthreads();   // the group is out before the next one lands in s_fr and s_x
  }
}

hipError_t launch_pvoc_shape(const PvocShapeArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.op == PVOC_WARP) {
    const long nframes = (long)a.channels * a.F;
    return pvoc_env_dispatch(a.logn, [&](auto L) {
      constexpr int LOGN = decltype(L)::value;
      return launch_pvoc_env<LOGN, k_pvoc_warp<LOGN>>(nframes, a.grid_max, di, s, a.in, a.out, a.par, a.F, nframes, a.lowest,
                                                      a.coefs, a.bpf, a.half, a.w2);
    });
  }
  if (a.op < PVOC_BAND || a.op > PVOC_LOCK) return hipErrorInvalidValue;
  const PvocTiles t = pvoc_tiles(a.M, kShapeWG, (long)a.channels * a.F, di, 16, a.grid_max);
  if (a.op == PVOC_LOCK)
    hipLaunchKernelGGL(k_pvoc_lock, dim3(t.grid), dim3(kShapeWG), 0, s, a.in, a.out, a.par, a.F, a.M, t.tiles, t.items);
  else
    hipLaunchKernelGGL(k_pvoc_shape, dim3(t.grid), dim3(kShapeWG), 0, s, a.in, a.out, a.par, a.table, a.F, a.M, t.tiles,
                       t.items, a.op, a.reject);
  return hipGetLastError();
}

}  // namespace clfa
