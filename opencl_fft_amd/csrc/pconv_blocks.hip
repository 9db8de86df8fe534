// pconv_blocks.hip — many consecutive blocks of a partitioned convolution in a fixed number of launches
// (clfa_pconv_process_blocks_dev), partitions of 32..4096 samples.
//
// A call of K blocks equals K calls of clfa_pconv_process_dev.  Per sub-batch of K blocks:
//   k_pconvb_fwd     spectra of all K x channels new blocks (and second inputs) -> workspace X (and XB)
//   k_pconvb_mac     Y_j = sum_p F(j, p) (.) H(j, p) for a tile of KT consecutive outputs j: the ring frame of
//                    partition p is loaded ONCE for the KT outputs, and their input frames — consecutive blocks —
//                    slide through a register window by one per partition
//   k_pconvb_inv     c2r + inverse transform + overlap-add, a run of consecutive blocks per transform slot
//   k_pconvb_commit  the last nparts spectra, the new second-input frames and the last tail go into the object's state
// The rings are read by the MAC as they stood before the call; they are written only by the commit launch, after
// every read.  Frame algebra (block j of the sub-batch, w = wp and w2 = wp2 before it, nparts partitions):
//   input of partition p for output j:  m = j - (nparts - 1) + p;  m >= 0: X[m], m < 0: ring A frame (w + m) mod nparts
//   response of partition p for output j (time-varying): k_p = (w2 - p) mod nparts; k_p <= j: XB[k_p], else ring B[p]
// Every output bin is one accumulator summed over p = 0, 1, ... nparts - 1 with the products of k_pconv_mac, whatever
// the tile, the sub-batch or the split of the signal into calls: results are bit-identical across splits.
#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

namespace {

__device__ __forceinline__ void st_pair(float *p, cpx v, bool aligned) {
  if (aligned) {
    *reinterpret_cast<cpx *>(p) = v;
  } else {
    p[0] = v.x;
    p[1] = v.y;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------
// forward: rows (channel, block j) of in -> X[(ch * cap + j) * N]; blockIdx.y = 1: in_b -> XB
// ---------------------------------------------------------------------------------
template <int LOGB>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_pconvb_fwd(const float *__restrict__ in, const float *__restrict__ in_b,
                                                                 long in_stride, cpx *__restrict__ X, cpx *__restrict__ XB,
                                                                 int K, int cap, int channels, int aligned,
                                                                 const cpx *__restrict__ tab_g, const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, T = G::T, WG = G::WG, FPW = G::FPW;
  if (blockIdx.y == 1) {
    in = in_b;
    X = XB;
  }
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();
  cpx *xb = s_x + f * G::PADN;
  const long rows = (long)channels * K;
  const long groups = (rows + FPW - 1) / FPW;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long r = g * FPW + f;
    const bool active = r < rows;
    const int ch = active ? (int)(r / K) : 0, j = active ? (int)(r % K) : 0;
    const float *src = in + (long)ch * in_stride + (long)j * N;
    fwd_row<LOGB>(src, aligned, active, X + ((long)ch * cap + j) * N, t, s_tab, xb, w2_g, [](int, cpx) {});
  }
}

// ---------------------------------------------------------------------------------
// multiply-accumulate with reuse: one wave = (16-byte item slice, tile of KT outputs, channel)
// ---------------------------------------------------------------------------------
template <int KT, bool TV>
__global__ __launch_bounds__(64) void k_pconvb_mac(const cpx *__restrict__ ringA, const cpx *__restrict__ ringB,
                                                   const cpx *__restrict__ X, const cpx *__restrict__ XB, cpx *__restrict__ Y,
                                                   int K, int cap, int w, int w2, int bins, int nparts) {
  const int hb = bins >> 1;
  const int item = blockIdx.x * 64 + threadIdx.x;
  const int it = item < hb ? item : hb - 1;   // (clamped: straight-line loads; the store is guarded)
  const int ch = blockIdx.z;
  const int j0 = blockIdx.y * KT;
  const cpx2 *ra = reinterpret_cast<const cpx2 *>(ringA + (long)ch * nparts * bins) + it;
  const cpx2 *rb = reinterpret_cast<const cpx2 *>(ringB + (long)ch * nparts * bins) + it;
  const cpx2 *xs = reinterpret_cast<const cpx2 *>(X + (long)ch * cap * bins) + it;
  const cpx2 *xbs = reinterpret_cast<const cpx2 *>(XB + (long)ch * cap * bins) + it;
  // input frame m of the sub-batch: m >= 0 this call's spectrum X[m]; m < 0 the ring's frame (w + m) mod nparts.
  // m > K - 1 only feeds outputs past the sub-batch (never stored): clamped
  auto frame = [&](int m) -> const cpx2 * {
    if (m >= 0) return xs + (long)(m < K ? m : K - 1) * hb;
    int f = w + m;
    f = f < 0 ? f + nparts : f;
    return ra + (long)f * hb;
  };
  const bool dc = item == 0;   // packed DC / Nyquist bin: (re*re, im*im)
  cpx s0[KT], s1[KT];
  cpx2 win[KT];
#pragma unroll
  for (int t = 0; t < KT; t++) {
    s0[t] = s1[t] = mk(0.f, 0.f);
    win[t] = ld_nt(frame(j0 + t - (nparts - 1)));
  }
  // (the lambda stays: with mac_term called straight from the unrolled loop hipcc emits another code object)
  auto mac = [&](int t, const cpx2 &a, const cpx2 &b) {
    mac_term(s0[t], s1[t], a, b, dc);
  };
  // one partition: the response frame(s) of p, then the next input frame of the window
  cpx2 bq = ld_nt(rb), bnq = bq, xq = win[0];
  int kq = 0;
  auto load = [&](int p) {
    bq = ld_nt(rb + (long)p * hb);
    if constexpr (TV) {
      int k = w2 - p;
      kq = k < 0 ? k + nparts : k;
      bnq = ld_nt(xbs + (long)(kq < K ? kq : 0) * hb);
    }
    xq = ld_nt(frame(j0 + KT - (nparts - 1) + p));   // enters the window after partition p
  };
  load(0);
  for (int p = 0; p < nparts; p++) {
    const cpx2 b = bq, bn = bnq, xn = xq;
    const int k = kq;
    if (p + 1 < nparts) load(p + 1);   // next partition's loads are in flight under this one's arithmetic
#pragma unroll
    for (int t = 0; t < KT; t++) {
      if constexpr (TV) {
        // output j0 + t sees the new second-input frame once block k_p (<= j) has filed it
        mac(t, win[t], (k < K && k <= j0 + t) ? bn : b);
      } else {
        mac(t, win[t], b);
      }
    }
    window_shift(win, xn);
  }
  if (item < hb) {
#pragma unroll
    for (int t = 0; t < KT; t++) {
      const int j = j0 + t;
      if (j < K) {
        cpx2 o;
        o.a = s0[t];
        o.b = s1[t];
        reinterpret_cast<cpx2 *>(Y + ((long)ch * cap + j) * bins)[item] = o;
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// inverse + overlap-add: rows (channel, run of R blocks); the run's first block takes the previous block's second
// half from the object's tail (run 0) or from the transform of the block before the run
// ---------------------------------------------------------------------------------
template <int LOGB>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_pconvb_inv(const cpx *__restrict__ Y, const float *__restrict__ tail,
                                                                 float *__restrict__ tail_out, float *__restrict__ out,
                                                                 long out_stride, int K, int cap, int R, int channels,
                                                                 int aligned, const cpx *__restrict__ tab_g,
                                                                 const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW;
  static_assert(E >= 2, "16 points per lane");
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();
  cpx *xb = s_x + f * G::PADN;
  const int nruns = (K + R - 1) / R;
  const long rows = (long)channels * nruns;
  const long groups = (rows + FPW - 1) / FPW;
  constexpr float inv = 1.0f / (float)N;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long r = g * FPW + f;
    const bool active = r < rows;
    const int ch = active ? (int)(r / nruns) : 0, run = active ? (int)(r % nruns) : 0;
    const int j0 = run * R, j1 = j0 + R < K ? j0 + R : K;
    cpx prev[E / 2];
    if (j0 == 0) {
      const cpx *tl = reinterpret_cast<const cpx *>(tail + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E / 2; e++) prev[e] = tl[t + T * e];
    }
    // iteration q transforms block j0 - 1 + q (q = 0 only for its second half); all slots walk R + 1 iterations
    for (int q = 0; q <= R; q++) {
      const int j = j0 - 1 + q;
      const bool live = active && j < j1 && (q > 0 || j0 > 0);
      const cpx *y = Y + ((long)ch * cap + (j < 0 ? 0 : (j < K ? j : K - 1))) * N;
      __syncthreads();
      if (live) {
        for (int i = t; i < N / 2; i += T)
          c2r_unpack<N>(i, [&](int p) { return y[p]; }, [&](int k) { return w2_g[k]; }, [&](int p, cpx val) { xb[lds_pad(p)] = val; });
      }
      __syncthreads();
      cpx v[E];
      pass_gather<LOGB, G::LOGE>(v, t, [&](int p) { return xb[lds_pad(p)]; });
      wg_passes<LOGB, G::LOGE, 0, false>(v, t, s_tab, xb);
      if (live) {
        // v[e] holds real samples 2p, 2p+1 of the 2*bins-point block, p = t + T*e: the first half is this block's output
        // (+ the previous block's second half, / bins), the second half carries on
        if (q > 0) {
          float *o = out + (long)ch * out_stride + (long)j * N;
#pragma unroll
          for (int e = 0; e < E / 2; e++) {
            const int p = t + T * e;
            st_pair(o + 2 * p, mk((v[e].x + prev[e].x) * inv, (v[e].y + prev[e].y) * inv), aligned);
          }
        }
#pragma unroll
        for (int e = 0; e < E / 2; e++) prev[e] = v[e + E / 2];
      }
    }
    if (active && j1 == K) {
      cpx *tl = reinterpret_cast<cpx *>(tail_out + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E / 2; e++) tl[t + T * e] = prev[e];
    }
  }
}

// ---------------------------------------------------------------------------------
// commit: y = 0 the last min(K, nparts) spectra -> ring A; y = 1 the new tail; y = 2 (time-varying) XB[k] -> ring B frame
// (w2 - k) mod nparts, k < K <= nparts
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pconvb_commit(cpx *__restrict__ ringA, cpx *__restrict__ ringB, float *__restrict__ tail,
                                                       const cpx *__restrict__ X, const cpx *__restrict__ XB,
                                                       const float *__restrict__ tail_new, int K, int cap, int w, int w2,
                                                       int bins, int nparts, int channels) {
  const int hb = bins >> 1;
  if (blockIdx.y == 1) return commit_tail(tail, tail_new, (long)channels * bins);
  const bool b = blockIdx.y == 2;
  commit_spectra(b ? ringB : ringA, b ? XB : X, b ? 0 : commit_first(K, nparts), K, cap, hb, nparts, channels, [&](int m) {
    if (b) {
      const int fr = w2 - m;
      return fr < 0 ? fr + nparts : fr;
    }
    return ring_a_frame(w, m, nparts);
  });
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
int pconv_blocks_tile(const PconvGeom &g, const DeviceInfo &di) {
  // enough waves on the item x channel axes alone: long tiles (each ring frame feeds 16 outputs); a few channels: short
  // tiles, so that the tile axis fills the chip.  Fixed per object: an output's arithmetic never depends on the tile.
  const long slices = g.bins / 2 >= 64 ? g.bins / 128 : 1;
  return (long)g.channels * slices >= di.num_cus ? 16 : 4;
}

template <int LOGB>
static hipError_t fwd_one(const float *in, const float *in_b, long in_stride, cpx *X, cpx *XB, int K, int cap, int channels,
                          int aligned, const cpx *half, const cpx *w2f, hipStream_t s) {
  using G = LdsGeom<LOGB>;
  long groups = ((long)channels * K + G::FPW - 1) / G::FPW;
  const int grid = grid_clamp(groups, 8192);
  hipLaunchKernelGGL((k_pconvb_fwd<LOGB>), dim3(grid, in_b ? 2 : 1), dim3(G::WG), 0, s, in, in_b, in_stride, X, XB, K, cap,
                     channels, aligned, half, w2f);
  return hipGetLastError();
}

template <int LOGB>
static hipError_t inv_one(const cpx *Y, const float *tail, float *tail_out, float *out, long out_stride, int K, int cap, int R,
                          int channels, int aligned, const cpx *half, const cpx *w2i, hipStream_t s) {
  using G = LdsGeom<LOGB>;
  const int nruns = (K + R - 1) / R;
  long groups = ((long)channels * nruns + G::FPW - 1) / G::FPW;
  const int grid = grid_clamp(groups, 8192);
  hipLaunchKernelGGL((k_pconvb_inv<LOGB>), dim3(grid), dim3(G::WG), 0, s, Y, tail, tail_out, out, out_stride, K, cap, R,
                     channels, aligned, half, w2i);
  return hipGetLastError();
}

template <int LOGB>
static hipError_t launch_blocks_one(const PconvBlocks &a, hipStream_t s) {
  const PconvGeom &g = a.g;
  {
    // a second input with rows of its own (another stride or alignment) takes a launch of its own
    const long stride2 = a.in2_stride ? a.in2_stride : a.in_stride;
    const int aligned2 = a.aligned_in2 < 0 ? a.aligned_in : a.aligned_in2;
    const bool own = a.in2 && (stride2 != a.in_stride || aligned2 != a.aligned_in);
    hipError_t e = fwd_one<LOGB>(a.in1, own ? nullptr : a.in2, a.in_stride, a.X, a.XB, a.K, a.cap, g.channels, a.aligned_in, a.half,
                                 a.w2f, s);
    if (e == hipSuccess && own)
      e = fwd_one<LOGB>(a.in2, nullptr, stride2, a.XB, nullptr, a.K, a.cap, g.channels, aligned2, a.half, a.w2f, s);
    if (e != hipSuccess) return e;
  }
  {
    const int hb = g.bins / 2;
    dim3 grid((hb + 63) / 64, (a.K + a.kt - 1) / a.kt, g.channels);
#define CLFA_MAC(KT, TVF)                                                                                                   \
  hipLaunchKernelGGL((k_pconvb_mac<KT, TVF>), grid, dim3(64), 0, s, (const cpx *)a.ringA, (const cpx *)a.ringB, (const cpx *)a.X, \
                     (const cpx *)a.XB, a.Y, a.K, a.cap, a.w, a.w2, g.bins, g.nparts)
    if (a.kt == 16) {
      if (a.in2) CLFA_MAC(16, true);
      else CLFA_MAC(16, false);
    } else {
      if (a.in2) CLFA_MAC(4, true);
      else CLFA_MAC(4, false);
    }
#undef CLFA_MAC
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  {
    hipError_t e = inv_one<LOGB>((const cpx *)a.Y, (const float *)a.tail, a.tail_ws, a.out, a.out_stride, a.K, a.cap, a.run,
                                 g.channels, a.aligned_out, a.half, a.w2i, s);
    if (e != hipSuccess) return e;
  }
  {
    long n = (long)g.channels * g.bins;
    const int grid = grid_clamp((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_pconvb_commit, dim3(grid, a.in2 ? 3 : 2), dim3(256), 0, s, a.ringA, a.ringB, a.tail, (const cpx *)a.X,
                       (const cpx *)a.XB, (const float *)a.tail_ws, a.K, a.cap, a.w, a.w2, g.bins, g.nparts, g.channels);
  }
  return hipGetLastError();
}

hipError_t launch_pconv_blocks(const PconvBlocks &a, hipStream_t s) {
  if (a.K < 1 || a.K > a.cap || (a.in2 && a.K > a.g.nparts) || (a.kt != 4 && a.kt != 16) || a.run < 1)
    return hipErrorInvalidValue;
  return dispatch_logb<kPconvBlocksMinLog, kPconvBlocksMaxLog>(a.g.logb,
                                                               [&](auto L) { return launch_blocks_one<decltype(L)::value>(a, s); });
}

// the forward and inverse launches on their own, for the convolution matrix (pconv_matrix.hip)
hipError_t launch_pconvb_forward(int logb, const float *in, long in_stride, cpx *X, int K, int cap, int channels, int aligned,
                                 const cpx *half, const cpx *w2f, hipStream_t s) {
  return dispatch_logb<kPconvBlocksMinLog, kPconvBlocksMaxLog>(logb, [&](auto L) {
    return fwd_one<decltype(L)::value>(in, nullptr, in_stride, X, nullptr, K, cap, channels, aligned, half, w2f, s);
  });
}

hipError_t launch_pconvb_inverse(int logb, const cpx *Y, const float *tail, float *tail_out, float *out, long out_stride, int K,
                                 int cap, int R, int channels, int aligned, const cpx *half, const cpx *w2i, hipStream_t s) {
  return dispatch_logb<kPconvBlocksMinLog, kPconvBlocksMaxLog>(logb, [&](auto L) {
    return inv_one<decltype(L)::value>(Y, tail, tail_out, out, out_stride, K, cap, R, channels, aligned, half, w2i, s);
  });
}

}  // namespace clfa
