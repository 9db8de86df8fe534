// pconv_chain.hip — uniformly partitioned overlap-add convolution for gfx950 (MI355X), batched over independent
// channels: the launch chain (restates cl_conv.cpp:393-458 and cl_conv_kernels.h:46-124).
//
// The reference runs 26 launches per block and channel (cl_conv.cpp:393-458:
// reorder, 10 x fft, r2c, convol with float CAS atomics, c2r, reorder, 10 x fft,
// olap).  Here a block is three launches for ALL channels:
//   k_pconv_fwd  real block -> zero-padded real FFT -> packed frame in the ring
//                (reorder + fft + r2c fused; the transform lives in VGPRs + LDS)
//   k_pconv_mac  acc[n] = sum_p A[(wp+p) % nparts][n] (.) B[p][n]; one lane owns
//                two bins and walks the partitions in registers: no atomics,
//                deterministic order, 16-byte coalesced streaming of both rings
//   k_pconv_inv  c2r + inverse FFT + overlap-add + 1/bins scaling fused
// The rings are channels x nparts x bins complex64, resident in HBM.
// The same block in fewer launches, and the direct convolution, one file per kernel family:
//   pconv_fused.inc  k_pconv_fused: one launch per block, one workgroup per channel (enough channels to fill the chip).
//                    Part of THIS translation unit (included at the end) because of the compiler, like the families of
//                    fft_kernels.hip: compiled apart, k_pconv_fwd<9..12> and k_pconv_inv<9..12> — the sizes both
//                    families instantiate — come out with other address arithmetic (profiles/conv_split_same.txt)
//   pconv_coop.hip   k_pconv_coop: one launch per block for a few channels, workgroups meet through handover.hpp
//   dconv_block.hip  k_dconv_block: the direct convolution (cl_dconv.cpp), same hand-over
//   handover.hpp     the inter-workgroup hand-over of pconv_coop.hip and dconv_block.hip
#include <cstdlib>

#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// forward: in (channels x pts floats) -> ring frame
// ---------------------------------------------------------------------------------
template <int LOGB>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_pconv_fwd(const float *__restrict__ in, long in_stride,
                                                                cpx *__restrict__ ring, int frame, int nparts,
                                                                int channels, const cpx *__restrict__ tab_g,
                                                                const cpx *__restrict__ w2_g,
                                                                const float *__restrict__ in_b, cpx *__restrict__ ring_b,
                                                                int frame_b) {
  // blockIdx.y = 1: the second input of a time-varying block (its own ring and frame), same launch
  if (blockIdx.y == 1) {
    in = in_b;
    ring = ring_b;
    frame = frame_b;
  }
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW;
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();
  cpx *xb = s_x + f * G::PADN;
  const int groups = (channels + FPW - 1) / FPW;
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    const int ch = g * FPW + f;
    const bool active = ch < channels;
    // the real block reinterpreted as N/2 complex values, upper half zero
    // (cl_conv.cpp:399: only bytes>>1 of in1 are written; the rest is zero)
    const cpx *src = reinterpret_cast<const cpx *>(in + (long)(active ? ch : 0) * in_stride);
    cpx v[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int p = t + T * e;
      v[e] = (active && p < N / 2) ? src[p] : mk(0.f, 0.f);
    }
    wg_passes<LOGB, G::LOGE, 0, true>(v, t, s_tab, xb);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; e++) xb[lds_pad(t + T * e)] = v[e];
    __syncthreads();
    if (active) {
      cpx *x = ring + ((long)ch * nparts + frame) * N;
      for (int i = t; i < N / 2; i += T) {
        if (i == 0) {
          cpx z = xb[0];
          x[0] = mk((z.x + z.y) * .5f, (z.x - z.y) * .5f);
          x[N / 2] = xb[lds_pad(N / 2)];
        } else {
          cpx oi, oj;
          r2c_pair(xb[lds_pad(i)], xb[lds_pad(N - i)], w2_g[i], oi, oj);
          x[i] = oi;
          x[N - i] = oj;
        }
      }
    }
  }
}

template <int LOGB>
static hipError_t launch_fwd_one(const PconvGeom &g, const float *in, long in_stride, cpx *ring, int frame,
                                 const cpx *half, const cpx *w2f, hipStream_t s, const float *in_b, cpx *ring_b,
                                 int frame_b) {
  using G = LdsGeom<LOGB>;
  int groups = (g.channels + G::FPW - 1) / G::FPW;
  const int grid = grid_clamp(groups, 4096);
  hipLaunchKernelGGL((k_pconv_fwd<LOGB>), dim3(grid, in_b ? 2 : 1), dim3(G::WG), 0, s, in, in_stride, ring, frame,
                     g.nparts, g.channels, half, w2f, in_b, ring_b, frame_b);
  return hipGetLastError();
}

hipError_t launch_pconv_forward(const PconvGeom &g, const float *in, long in_stride, cpx *ring, int frame,
                                const cpx *half, const cpx *w2f, hipStream_t s, const float *in_b, cpx *ring_b,
                                int frame_b) {
  return dispatch_logb<1, 13>(g.logb, [&](auto L) {
    return launch_fwd_one<decltype(L)::value>(g, in, in_stride, ring, frame, half, w2f, s, in_b, ring_b, frame_b);
  });
}

// ---------------------------------------------------------------------------------
// multiply-accumulate over partitions (reference convol, cl_conv_kernels.h:102-118)
// ---------------------------------------------------------------------------------
// one lane = two adjacent bins (16 B) of one channel; loops the partitions of its segment.
// blockIdx.y = segment of the partition axis (1 segment when there are enough channels to fill
// the chip; few channels with long filters are split and summed by k_pconv_reduce in fixed order)
template <int UNROLL>
__global__ __launch_bounds__(256) void k_pconv_mac(const cpx *__restrict__ A, const cpx *__restrict__ B,
                                                   cpx *__restrict__ acc, int wp, int bins, int nparts,
                                                   long total /* channels * bins/2 */, int chunk) {
  const int hb = bins >> 1;
  const int p_begin = blockIdx.y * chunk;
  const int p_end = p_begin + chunk < nparts ? p_begin + chunk : nparts;
  cpx *dst = acc + (long)blockIdx.y * total * 2;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long ch = g / hb;
    const int i2 = (int)(g % hb);
    const cpx2 *a = reinterpret_cast<const cpx2 *>(A + ch * (long)nparts * bins) + i2;
    const cpx2 *b = reinterpret_cast<const cpx2 *>(B + ch * (long)nparts * bins) + i2;
    cpx s0 = mk(0.f, 0.f), s1 = mk(0.f, 0.f);
    int fr = wp + p_begin;  // ring frame of partition p_begin (wp = frame of the oldest input block)
    fr = fr < nparts ? fr : fr - nparts;
    int p = p_begin;
    for (; p + UNROLL <= p_end; p += UNROLL) {
      cpx2 av[UNROLL], bv[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; u++) {
        int f = fr + u;
        f = f < nparts ? f : f - nparts;
        av[u] = ld_nt(a + (long)f * hb);
        bv[u] = ld_nt(b + (long)(p + u) * hb);
      }
#pragma unroll
      for (int u = 0; u < UNROLL; u++) mac_term(s0, s1, av[u], bv[u], i2 == 0);
      fr += UNROLL;
      fr = fr < nparts ? fr : fr - nparts;
    }
    // (not on mac_term: with the select form hipcc emits other arithmetic for this loop — v_mul + v_sub where it fuses today)
    for (; p < p_end; p++) {
      cpx2 av = a[(long)fr * hb], bv = b[(long)p * hb];
      if (i2 == 0) {
        s0.x += av.a.x * bv.a.x;
        s0.y += av.a.y * bv.a.y;
      } else {
        s0 = cadd(s0, cmul_plain(av.a, bv.a));
      }
      s1 = cadd(s1, cmul_plain(av.b, bv.b));
      fr = fr + 1 < nparts ? fr + 1 : 0;
    }
    cpx2 o;
    o.a = s0;
    o.b = s1;
    reinterpret_cast<cpx2 *>(dst)[g] = o;
  }
}

// partial accumulators k = base, base + stride, ..., (count of them, base = blockIdx.y * count * stride, as far as
// nsplit goes) summed in ascending order into accumulator `base`: deterministic.  One launch with count = nsplit sums
// everything; many segments (a single channel with a long filter) are summed as a two-level tree so that the sum is
// not one workgroup's serial walk over hundreds of strided loads.  MAXC > 0: count <= MAXC, all loads are issued
// before the first add (one memory latency instead of `count`).
template <int MAXC>
__global__ __launch_bounds__(256) void k_pconv_reduce(cpx *__restrict__ acc, long total2, int nsplit, int count, int stride) {
  const int base = blockIdx.y * count * stride;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total2; g += (long)gridDim.x * 256) {
    if constexpr (MAXC > 0) {
      cpx v[MAXC];
#pragma unroll
      for (int k = 0; k < MAXC; k++) {
        const bool ok = k < count && base + k * stride < nsplit;
        v[k] = acc[(long)(ok ? base + k * stride : base) * total2 + g];   // clamped: straight-line loads
        if (!ok) v[k] = mk(0.f, 0.f);
      }
      cpx s = v[0];
#pragma unroll
      for (int k = 1; k < MAXC; k++) s = cadd(s, v[k]);
      acc[(long)base * total2 + g] = s;
    } else {
      cpx s = acc[(long)base * total2 + g];
      for (int k = 1; k < count && base + k * stride < nsplit; k++) s = cadd(s, acc[(long)(base + k * stride) * total2 + g]);
      acc[(long)base * total2 + g] = s;
    }
  }
}

int pconv_mac_split(const PconvGeom &g) {
  // split only when channels x bins/2 gives fewer than ~64K lanes (config 4 has 131072: no split).  A single
  // channel with a long filter — the reference harness' own case, csound/tests.py — has to put the whole chip on
  // the partition axis to stream its rings at HBM speed: up to 512 segments of at least 4 partitions
  // (CLFA_PCONV_SPLIT_MAX: tuning switch, read once).
  static const int cap = [] {
    const char *e = getenv("CLFA_PCONV_SPLIT_MAX");
    const int v = e ? atoi(e) : 512;
    return v < 1 ? 1 : (v > 2048 ? 2048 : v);   // the two-level sum holds 64 groups of 32 partial accumulators
  }();
  long lanes = (long)g.channels * (g.bins / 2);
  const long target = lanes <= 1024 ? 128L * 1024 : 64L * 1024;   // measured: the finer split pays up to pts = 2048
  long want = (target + lanes - 1) / lanes;
  if (lanes >= 64L * 1024) want = 1;
  if (want > cap) want = cap;
  if (want > g.nparts / 4) want = g.nparts / 4;   // (segments of 1 or 2 partitions: measured, mixed — not kept)
  return want < 1 ? 1 : (int)want;
}

hipError_t launch_pconv_mac(const PconvGeom &g, const cpx *ringA, const cpx *ringB, int wp, cpx *acc,
                            hipStream_t s, bool reduce) {
  long total = (long)g.channels * (g.bins / 2);
  long grid = (total + 255) / 256;
  if (grid > 256 * 64) grid = 256 * 64;
  const int nsplit = pconv_mac_split(g);
  const int chunk = (g.nparts + nsplit - 1) / nsplit;
  hipLaunchKernelGGL((k_pconv_mac<4>), dim3((int)grid, nsplit), dim3(256), 0, s, ringA, ringB, acc, wp, g.bins,
                     g.nparts, total, chunk);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || nsplit == 1 || !reduce) return e;
  long total2 = total * 2, rgrid = (total2 + 255) / 256;
  if (rgrid > 4096) rgrid = 4096;
  auto sum = [&](int groups, int count, int stride) -> hipError_t {   // the smallest unrolled form that holds `count`
    const dim3 grid((int)rgrid, groups), block(256);
    if (count > 64) return hipErrorInvalidValue;   // (cannot happen below the 2048 cap: a dropped partial sum must not pass silently)
    if (count <= 2) hipLaunchKernelGGL(k_pconv_reduce<2>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    else if (count <= 4) hipLaunchKernelGGL(k_pconv_reduce<4>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    else if (count <= 8) hipLaunchKernelGGL(k_pconv_reduce<8>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    else if (count <= 16) hipLaunchKernelGGL(k_pconv_reduce<16>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    else if (count <= 32) hipLaunchKernelGGL(k_pconv_reduce<32>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    else hipLaunchKernelGGL(k_pconv_reduce<64>, grid, block, 0, s, acc, total2, nsplit, count, stride);
    return hipGetLastError();
  };
  if (nsplit > 64) {   // groups of 32, then the group sums
    const int groups = (nsplit + 31) / 32;
    if ((e = sum(groups, 32, 1)) != hipSuccess) return e;
    return sum(1, groups, 32);
  }
  return sum(1, nsplit, 1);
}

// ---------------------------------------------------------------------------------
// inverse: acc -> c2r -> inverse FFT -> overlap-add (reference c2r + reorder +
// fft + olap, cl_conv_kernels.h:87-100, 120-124)
// ---------------------------------------------------------------------------------
template <int LOGB>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_pconv_inv(const cpx *__restrict__ acc,
                                                                float *__restrict__ tail,
                                                                float *__restrict__ out, int channels,
                                                                const cpx *__restrict__ tab_g,
                                                                const cpx *__restrict__ w2_g, int nsplit) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW;
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();
  cpx *xb = s_x + f * G::PADN;
  const int groups = (channels + FPW - 1) / FPW;
  const long part = (long)channels * N;   // one partial accumulator (MAC split over the partition axis)
  for (int g = blockIdx.x; g < groups; g += gridDim.x) {
    const int ch = g * FPW + f;
    const bool active = ch < channels;
    const cpx *x0 = acc + (long)(active ? ch : 0) * N;
    // sum of the partial accumulators, ascending (the order k_pconv_reduce uses): no separate launch
    auto x = [&](int i) {
      cpx sum = x0[i];
      for (int k = 1; k < nsplit; k++) sum = cadd(sum, x0[k * part + i]);
      return sum;
    };
    __syncthreads();
    if (active) {
      for (int i = t; i < N / 2; i += T)
        c2r_unpack<N>(i, x, [&](int k) { return w2_g[k]; }, [&](int p, cpx val) { xb[lds_pad(p)] = val; });
    }
    __syncthreads();
    cpx v[E];
    pass_gather<LOGB, G::LOGE>(v, t, [&](int p) { return xb[lds_pad(p)]; });
    wg_passes<LOGB, G::LOGE, 0, false>(v, t, s_tab, xb);
    if (active) {
      // v[e] holds real samples 2p, 2p+1 of the 2*bins-point block, p = t + T*e.
      // p < N/2: output half (+ old tail, / bins); p >= N/2: the new tail, unscaled.
      constexpr float inv = 1.0f / (float)N;
      cpx *o = reinterpret_cast<cpx *>(out + (long)ch * N);
      cpx *tl = reinterpret_cast<cpx *>(tail + (long)ch * N);
      if constexpr (E >= 2) {
#pragma unroll
        for (int e = 0; e < E / 2; e++) {
          const int p = t + T * e;
          cpx old = tl[p];
          o[p] = mk((v[e].x + old.x) * inv, (v[e].y + old.y) * inv);
          tl[p] = v[e + E / 2];
        }
      }
    }
  }
}

template <int LOGB>
static hipError_t launch_inv_one(const PconvGeom &g, const cpx *acc, float *tail, float *out, const cpx *half,
                                 const cpx *w2i, hipStream_t s, int nsplit) {
  using G = LdsGeom<LOGB>;
  int groups = (g.channels + G::FPW - 1) / G::FPW;
  const int grid = grid_clamp(groups, 4096);
  hipLaunchKernelGGL((k_pconv_inv<LOGB>), dim3(grid), dim3(G::WG), 0, s, acc, tail, out, g.channels, half, w2i, nsplit);
  return hipGetLastError();
}

hipError_t launch_pconv_inverse(const PconvGeom &g, const cpx *acc, float *tail, float *out, const cpx *half,
                                const cpx *w2i, hipStream_t s, int nsplit) {
  return dispatch_logb<1, 13>(g.logb, [&](auto L) {
    return launch_inv_one<decltype(L)::value>(g, acc, tail, out, half, w2i, s, nsplit);
  });
}

// ---------------------------------------------------------------------------------
// partitions above the LDS sizes (pts = 16384, 32768): the same chain composed from the
// large-N FFT kernel; these two kernels are its zero-padding and overlap-add ends
// ---------------------------------------------------------------------------------
// work[ch][p] = p < bins/2 ? (in[ch][2p], in[ch][2p+1]) : 0   (cl_conv.cpp:399: half of in1 is written)
__global__ __launch_bounds__(256) void k_pconv_pad(const float *__restrict__ in, long in_stride,
                                                   cpx *__restrict__ work, int bins, long total) {
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long ch = g / bins;
    const int p = (int)(g % bins);
    work[g] = p < bins / 2 ? reinterpret_cast<const cpx *>(in + ch * in_stride)[p] : mk(0.f, 0.f);
  }
}
// reference olap (cl_conv_kernels.h:120-124) on work viewed as 2*bins floats per channel
__global__ __launch_bounds__(256) void k_pconv_olap(const float *__restrict__ work, float *__restrict__ tail,
                                                    float *__restrict__ out, int bins, long total) {
  const float inv = 1.0f / (float)bins;
  for (long g = blockIdx.x * 256L + threadIdx.x; g < total; g += (long)gridDim.x * 256) {
    const long ch = g / bins;
    const int n = (int)(g % bins);
    const float *t = work + ch * 2L * bins;
    out[g] = (t[n] + tail[g]) * inv;
    tail[g] = t[bins + n];
  }
}
hipError_t launch_pconv_pad(const float *in, long in_stride, cpx *work, int bins, int channels, hipStream_t s) {
  long total = (long)channels * bins, grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_pconv_pad, dim3((int)grid), dim3(256), 0, s, in, in_stride, work, bins, total);
  return hipGetLastError();
}
hipError_t launch_pconv_olap(const float *work, float *tail, float *out, int bins, int channels, hipStream_t s) {
  long total = (long)channels * bins, grid = (total + 255) / 256;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_pconv_olap, dim3((int)grid), dim3(256), 0, s, work, tail, out, bins, total);
  return hipGetLastError();
}

}  // namespace clfa

#include "pconv_fused.inc"
