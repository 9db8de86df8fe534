// dconv_blocks.hip — direct convolution of whole signals for many channels (clfa_dconv_process_blocks_dev, static form):
//   out_c[t] = sum_{k < irsize} coef_c[k] x_c[t - 1 - k],   0 <= t < L = nblocks * vsize
// where x_c[tau] is the call's input for tau >= 0 and the delay ring at (wp + tau) mod end for -irsize <= tau < 0.
//
// Two or three launches per sub-batch, for ALL channels:
//   k_dconvb_fir     grid (tile of consecutive outputs, channel, tap segment).  Tiles ignore the block boundaries: a
//                    channel's signal is contiguous.  A lane owns R consecutive outputs and keeps the 2 R - 1 samples
//                    they meet over R consecutive taps in registers; per group of R taps it takes R new samples from an
//                    LDS copy of the tile's window (one aligned 16-byte read per four of them) and R coefficients that are
//                    uniform across the workgroup (scalar loads): R multiply-adds per LDS dword where k_dconv_block gets
//                    one.  The window is staged per chunk of kDconvbChunk taps, R + 1 clamped loads per lane in flight.
//   k_dconvb_reduce  only with more than one tap segment (responses longer than kDconvbSeg): the segments' partial sums
//                    added in ascending segment order.
//   k_dconvb_commit  files the last `end` input samples in the delay rings.  The compute launch reads the rings, this one
//                    writes them; the stream orders the two.
//
// Order of every output's sum (the contract of include/clfft_amd.h): taps in ascending k, one fused multiply-add each,
// into an accumulator that starts at zero with every chunk of kDconvbChunk taps (counted from the segment's first tap);
// the chunks' sums added in ascending order, then the segments' in ascending order.  Nothing in it depends on which tile
// or lane an output lands in or on R, so results do not depend on nblocks, on the split into calls and sub-batches, or
// on the R the launcher picks.  No atomics.
#include "dconv_launch.hpp"
#include "pconv_device.hpp"

namespace clfa {

DconvBlocksPlan dconv_blocks_plan(int irsize) {
  DconvBlocksPlan pl;
  long segs = ((long)irsize + kDconvbSeg - 1) / kDconvbSeg;
  segs = segs > kDconvbMaxSegs ? kDconvbMaxSegs : segs;
  long len = ((long)irsize + segs - 1) / segs;
  len = (len + kDconvbChunk - 1) / kDconvbChunk * kDconvbChunk;   // whole chunks: every segment starts a fresh accumulator
  pl.seg_len = len > 0x7fffff00L ? 0x7fffff00 : (int)len;
  pl.segs = (int)(((long)irsize + pl.seg_len - 1) / pl.seg_len);
  return pl;
}

template <int R>
__global__ __launch_bounds__(256) void k_dconvb_fir(float *__restrict__ out, long out_stride, const float *__restrict__ in1,
                                                    long in_stride, const float *__restrict__ del,
                                                    const float *__restrict__ coefs, float *__restrict__ part,
                                                    long part_stride, int irsize, int end, int wp, long L, int seg_len) {
  constexpr int T = 256 * R, W = T + kDconvbChunk;   // outputs per tile; samples of the window a chunk of taps meets
  static_assert(kDconvbChunk % R == 0 && W % 256 == 0, "aligned blocks of R samples; whole staging rounds");
  __shared__ __attribute__((aligned(16))) float s_x[W];
  const int tid = threadIdx.x, c = blockIdx.y, sg = blockIdx.z;
  const long t0 = (long)blockIdx.x * T;
  const long ka = (long)sg * seg_len;
  const long kb = ka + seg_len < irsize ? ka + seg_len : irsize;
  const float *x = in1 + (long)c * in_stride;
  const float *ring = del + (long)c * end;
  const float *cf = coefs + (long)c * end;
  float tot[R];
#pragma unroll
  for (int i = 0; i < R; i++) tot[i] = 0.f;
  for (long kc = ka; kc < kb; kc += kDconvbChunk) {
    const int nt = (int)(kb - kc < kDconvbChunk ? kb - kc : kDconvbChunk);
    // s_x[j] = x[t0 - kc - kDconvbChunk + j]: history from the ring, the rest from the input; indices clamped instead of
    // branched around, all of a lane's loads in flight (as k_dconv_block stages); zero outside [-irsize, L)
    const long tau0 = t0 - kc - kDconvbChunk;
    float v[W / 256];
    bool inside[W / 256];
#pragma unroll
    for (int u = 0; u < W / 256; u++) {
      const long tau = tau0 + tid + 256 * u;
      const long tc = tau < -(long)irsize ? -(long)irsize : (tau > L - 1 ? L - 1 : tau);
      long r = wp + tc;   // tc < 0: ring index (wp + tau) mod end, wp + tau >= -irsize > -end
      r = r < 0 ? r + end : r;
      const float *src = tc >= 0 ? x + tc : ring + r;
      v[u] = *src;
      inside[u] = tc == tau;
    }
    __syncthreads();   // the previous chunk's readers are done
#pragma unroll
    for (int u = 0; u < W / 256; u++) s_x[tid + 256 * u] = inside[u] ? v[u] : 0.f;
    __syncthreads();
    // taps kc + g R + q, q < R: output i of this lane meets s[R - 1 + i - q] of the 2 R - 1 samples s = (lo | hi), the
    // aligned blocks R (tid - g - 1) and R (tid - g) past s_x[kDconvbChunk]; the next group's hi is this one's lo
    auto block = [&](int b, float (&d)[R]) {
      const float *p = s_x + kDconvbChunk + R * b;
      if constexpr (R % 4 == 0) {
#pragma unroll
        for (int m = 0; m < R; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4 *>(p + m);
          d[m] = q4.x, d[m + 1] = q4.y, d[m + 2] = q4.z, d[m + 3] = q4.w;
        }
      } else if constexpr (R % 2 == 0) {
#pragma unroll
        for (int m = 0; m < R; m += 2) {
          const float2 q2 = *reinterpret_cast<const float2 *>(p + m);
          d[m] = q2.x, d[m + 1] = q2.y;
        }
      } else {
#pragma unroll
        for (int m = 0; m < R; m++) d[m] = p[m];
      }
    };
    float acc[R], hi[R], lo[R];
#pragma unroll
    for (int i = 0; i < R; i++) acc[i] = 0.f;
    block(tid, hi);
    const int full = nt / R;
#pragma unroll 2
    for (int g = 0; g < full; g++) {
      block(tid - g - 1, lo);
      const float *ck = cf + kc + g * R;   // uniform across the workgroup
#pragma unroll
      for (int q = 0; q < R; q++) {
        const float cq = ck[q];
#pragma unroll
        for (int i = 0; i < R; i++) {
          const int m = R - 1 + i - q;
          acc[i] = __builtin_fmaf(cq, m < R ? lo[m] : hi[m - R], acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < R; i++) hi[i] = lo[i];
    }
    // the last taps of a response that is no multiple of R: same order, samples straight from LDS
    for (int q = 0; q < nt - full * R; q++) {
      const float cq = cf[kc + full * R + q];
      const float *p = s_x + kDconvbChunk - 1 + R * (tid - full) - q;
#pragma unroll
      for (int i = 0; i < R; i++) acc[i] = __builtin_fmaf(cq, p[i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < R; i++) tot[i] += acc[i];
  }
  float *dst = gridDim.z == 1 ? out + (long)c * out_stride : part + ((long)sg * gridDim.y + c) * part_stride;
#pragma unroll
  for (int i = 0; i < R; i++) {
    const long t = t0 + (long)tid * R + i;
    if (t < L) dst[t] = tot[i];
  }
}

// out_c[t] = the segments' partial sums in ascending segment order (as k_pconvm_reduce: every load issued, then the adds)
__global__ __launch_bounds__(256) void k_dconvb_reduce(float *__restrict__ out, long out_stride, const float *__restrict__ part,
                                                       long part_stride, int segs, long L) {
  const int c = blockIdx.y, channels = gridDim.y;
  for (long t = blockIdx.x * 256L + threadIdx.x; t < L; t += (long)gridDim.x * 256) {
    float sum = part[(long)c * part_stride + t];
    int s = 1;
    for (; s + 8 <= segs; s += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = part[((long)(s + u) * channels + c) * part_stride + t];
#pragma unroll
      for (int u = 0; u < 8; u++) sum += v[u];
    }
    for (; s < segs; s++) sum += part[((long)s * channels + c) * part_stride + t];
    out[(long)c * out_stride + t] = sum;
  }
}

// the call's last n = min(L, end) input samples into the delay rings at (wp + tau) mod end
__global__ __launch_bounds__(256) void k_dconvb_commit(float *__restrict__ del, const float *__restrict__ in1, long in_stride,
                                                       int end, int wp, long L, long n) {
  const int c = blockIdx.y;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long tau = L - n + i;
    del[(long)c * end + (wp + tau) % end] = in1[(long)c * in_stride + tau];
  }
}

hipError_t launch_dconv_blocks(const DconvBlocksArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.L < 1 || a.channels < 1 || a.channels > 65535 || a.plan.segs < 1 || a.plan.segs > kDconvbMaxSegs ||
      (long)a.plan.segs * a.plan.seg_len < a.irsize || (a.plan.segs > 1 && (!a.part || a.part_stride < a.L)))
    return hipErrorInvalidValue;
  // outputs per lane: 8 once that still gives every CU two workgroups, else 2 (more, smaller tiles; the same bits)
  const long tiles8 = (a.L + 256 * 8 - 1) / (256 * 8), tiles2 = (a.L + 256 * 2 - 1) / (256 * 2);
  const bool wide = a.plan.force_r ? a.plan.force_r == 8 : tiles8 * a.channels * a.plan.segs >= 2L * di.num_cus;
  const long tiles = wide ? tiles8 : tiles2;
  if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles, a.channels, a.plan.segs);
  if (wide)
    hipLaunchKernelGGL(k_dconvb_fir<8>, grid, dim3(256), 0, s, a.out, a.out_stride, a.in1, a.in_stride, a.del, a.coefs, a.part,
                       a.part_stride, a.irsize, a.end, a.wp, a.L, a.plan.seg_len);
  else
    hipLaunchKernelGGL(k_dconvb_fir<2>, grid, dim3(256), 0, s, a.out, a.out_stride, a.in1, a.in_stride, a.del, a.coefs, a.part,
                       a.part_stride, a.irsize, a.end, a.wp, a.L, a.plan.seg_len);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.plan.segs > 1) {
    hipLaunchKernelGGL(k_dconvb_reduce, dim3(grid_clamp((a.L + 255) / 256, 4096), a.channels), dim3(256), 0, s, a.out,
                       a.out_stride, a.part, a.part_stride, a.plan.segs, a.L);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const long n = a.L < a.end ? a.L : a.end;
  hipLaunchKernelGGL(k_dconvb_commit, dim3(grid_clamp((n + 255) / 256, 4096), a.channels), dim3(256), 0, s, a.del, a.in1,
                     a.in_stride, a.end, a.wp, a.L, n);
  return hipGetLastError();
}

}  // namespace clfa
