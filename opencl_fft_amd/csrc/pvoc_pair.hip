// pvoc_pair.hip — operations on two streams of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): cross-synthesis,
// morph, spectral filter, spectral maximum and the channel vocoder.  Stateless, one launch per call, no atomics; the tile
// kernel's prologue and launch (pvoc_bin, pvoc_tiles) are pvoc_device.hpp's, the vocoder's launch and size dispatch
// (launch_pvoc_env, pvoc_env_dispatch) pvoc_env.hpp's.
//
//   k_pvoc_pair    cross, morph, filter, mix: a lane takes bin k of one frame, reads the pair of a and the pair of b and
//                  writes one pair; rows of consecutive bins, 8 bytes per lane and stream (16 in, 8 out), no LDS.  The
//                  op is a kernel argument: every lane of a launch takes the same branch.
//   k_pvoc_vocode  a workgroup holds FPW = LdsGeom::FPW frames.  The a-frames go through the envelope stages of
//                  k_pvoc_formant (pvoc_envelope, pvoc_env.hpp) and every lane picks up envA of its own bins (element
//                  tid + i WG, i < 17: 17 floats in registers); the b-frames then go through the same stages in the same
//                  slots, their pairs staying in LDS as k_pvoc_formant's do; the rule is applied bin by bin, each lane
//                  on the bins whose envA it holds.  Each input frame is read once, the output written once, no
//                  workspace.  LDS is k_pvoc_formant's (exchange buffer + one frame copy, 132 KiB at n = 8192, where the
//                  twiddle tables come from L1/L2).
//
// Every float32 step of the definitions is rounded on its own: the device functions below switch contraction off.
// tests/pvoc_pair_model.py restates them.
#include "pvoc_device.hpp"
#include "pvoc_env.hpp"

namespace clfa {

namespace {

constexpr int kPairWG = 256;   // lanes = bins per workgroup tile (k_pvoc_pair)

// one bin of ops 0..3
__device__ __forceinline__ cpx pvoc_pair_bin(int op, cpx a, cpx b, float P, float Q) {
#pragma clang fp contract(off)
  if (op == PVOC_CROSS) {
    const float x = a.x * P, y = b.x * Q;
    return mk(x + y, a.y);
  }
  if (op == PVOC_MORPH) return mk(pvoc_morph(a.x, b.x, pvoc_clamp01(P)), pvoc_morph(a.y, b.y, pvoc_clamp01(Q)));
  if (op == PVOC_FILTER) {
    const float d = pvoc_clamp01(P);
    const float u = 1.f - d, w = d * b.x;
    const float m = d == 0.f ? 1.f : u + w;
    const float x = a.x * m;
    return mk(Q * x, a.y);
  }
  return b.x > a.x ? b : a;   // PVOC_MIX: a comparison with a NaN is false
}

// one bin of the vocoder: b = the excitation's pair
__device__ __forceinline__ cpx pvoc_vocode_bin(cpx b, float envA, float envB, float P, float Q) {
#pragma clang fp contract(off)
  const float d = pvoc_clamp01(P);
  const float r = envA / envB;
  const float u = 1.f - d, w = d * r;
  const float m = u + w;
  const float x = b.x * m;
  return mk(Q * x, b.y);
}

}  // namespace

// item -> (channel, frame f, bin tile), the tile fastest.  p, q: NULL for PVOC_MIX, which reads neither
__global__ __launch_bounds__(kPairWG) void k_pvoc_pair(const cpx *a, const cpx *b, cpx *__restrict__ out,
                                                       const float *p, const float *q, long F, int M, int tiles,
                                                       long items, int op) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long f, c;
    if (!pvoc_bin<kPairWG>(item, tiles, F, M, k, f, c)) continue;
    const long e = (c * F + f) * (M + 1) + k;
    float P = 0.f, Q = 0.f;
    if (op != PVOC_MIX) {
      P = p[f];
      Q = q[f];
    }
    out[e] = pvoc_pair_bin(op, a[e], b[e], P, Q);
  }
}

// grid-stride over groups of FPW consecutive frames (frame index c * F + f; the frames are contiguous)
template <int LOGN>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG) void k_pvoc_vocode(const cpx *a, const cpx *b, cpx *__restrict__ out,
                                                                   const float *p, const float *q, long F, long nframes,
                                                                   int coefs, const cpx *__restrict__ tab_g,
                                                                   const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGN>;
  using P = PvocEnv<LOGN>;
  constexpr int N = G::N, WG = G::WG, FPW = G::FPW, B = P::B, ITERS = P::ITERS;
  constexpr bool TL = pvoc_env_tab_lds<LOGN>();
  __shared__ cpx s_tab[TL ? G::HALF : 1];
  __shared__ cpx s_w2[TL ? N / 2 : 1];
  __shared__ cpx s_x[FPW * G::PADN];   // the exchange buffer, first of the a-frames, then of the b-frames
  __shared__ cpx s_fr[FPW * B];        // the group's b-frames as read
  __shared__ cpx s_pq[FPW];            // (p, q) of the group's frames
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
    if (tid < grp.nv) {   // the frames' (p, q); the barriers of the envelope stages stand between this and their use
      const long f = (b0 + tid) % F;
      s_pq[tid] = mk(p[f], q[f]);
    }
    pvoc_envelope<LOGN>(s_x, tab, w2, coefs, live, [&](int idx) { return a[b0 * B + idx].x; });
    float ea[ITERS];   // envA of the lane's own bins: element idx = tid + i WG
#pragma unroll
    for (int i = 0; i < ITERS; i++) {
      const int idx = tid + i * WG, fi = idx / B;
      if (idx < live) ea[i] = P::sample(s_x, fi, idx - fi * B);
    }
    __syncthreads();   // envA is out of s_x before the b-frames land there
    pvoc_envelope<LOGN>(s_x, tab, w2, coefs, live, [&](int idx) {
      const cpx bf = b[b0 * B + idx];
      s_fr[idx] = bf;
      return bf.x;
    });
#pragma unroll
    for (int i = 0; i < ITERS; i++) {
      const int idx = tid + i * WG, fi = idx / B;
      if (idx < live)
        out[b0 * B + idx] = pvoc_vocode_bin(s_fr[idx], ea[i], P::sample(s_x, fi, idx - fi * B), s_pq[fi].x, s_pq[fi].y);
    }
    __syncthreads();   // the group is out before the next one lands in s_x, s_fr and s_pq
  }
}

hipError_t launch_pvoc_pair(const PvocPairArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.op == PVOC_VOCODE) {
    const long nframes = (long)a.channels * a.F;
    return pvoc_env_dispatch(a.logn, [&](auto L) {
      constexpr int LOGN = decltype(L)::value;
      return launch_pvoc_env<LOGN, k_pvoc_vocode<LOGN>>(nframes, a.grid_max, di, s, a.a, a.b, a.out, a.p, a.q, a.F, nframes,
                                                        a.coefs, a.half, a.w2);
    });
  }
  const PvocTiles t = pvoc_tiles(a.M, kPairWG, (long)a.channels * a.F, di, 16, a.grid_max);
  hipLaunchKernelGGL(k_pvoc_pair, dim3(t.grid), dim3(kPairWG), 0, s, a.a, a.b, a.out, a.p, a.q, a.F, a.M, t.tiles, t.items,
                     a.op);
  return hipGetLastError();
}

}  // namespace clfa
