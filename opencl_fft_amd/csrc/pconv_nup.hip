// pconv_nup.hip — the kernels of the non-uniformly partitioned convolution (clfa_nupconv, nupconv_host.cpp): a head of small
// partitions (pts0) gives the latency; the long tail runs in large partitions (pts1 = m * pts0), and each tail block's
// multiply-accumulate is spread in m slices of its bins over the m head blocks that pass while its output is not yet needed.
//   k_nupc_stage   the call's input rows -> the tail's input row (channels x pts1 floats) at the stream's position
//   k_nupc_stage2  the same for two sets of rows in one launch: x and the time-varying second input
//   k_nupc_fwd     a time-varying block's forward transforms of one level, two jobs in one launch (x and the second
//                  input, each with its own rows and destination frame); a job may also file its samples in a stage row
//   k_nupc_mac     Y = sum_p A[(w - (nparts - 1) + p) mod nparts] (.) B[p] of ONE block of a level over a range of its
//                  16-byte items: one accumulator per bin over p = 0, 1, ... nparts - 1 with mac_term, the order and the
//                  products of k_pconvb_mac — the bits of Clpconv's blocks route, however the bins are cut into slices.
//                  A single-block call runs the head's block and the tail's slice in one launch of it
//   k_nupc_mix     out = head + pending tail output at the stream's position, one float32 addition, the head first
//   k_nupc_fade_mix  a block of a timed crossfade (clfft_amd.h): both paths' head + pending sums, then a + g * (b - a)
// The forward and inverse transforms are launch_pconvb_forward / launch_pconvb_inverse with K = 1 (a time-varying block's
// forward transforms: k_nupc_fwd, the same row transform); calls of several blocks
// run the head through launch_pconv_blocks.  A new block's spectrum goes straight into ring frame w, the one frame the
// multiply-accumulate of the block before it does not read; committing it is the host's w + 1.
#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

// rows of n floats (a multiple of 32) as units of V floats: V = 4 where every row start is 16-byte aligned
template <int V> struct RowUnit;
template <> struct RowUnit<1> { typedef float type; };
template <> struct RowUnit<4> { typedef v4f type; };

}  // namespace

// ---------------------------------------------------------------------------------
// stage: in[ch][0 .. n) -> stage[ch][off .. off + n)
// ---------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_nupc_stage(const float *__restrict__ in, long in_stride, float *__restrict__ stage,
                                                    int pts1, int off, int n, int channels) {
  typedef typename RowUnit<V>::type U;
  const int nu = n / V;
  const long total = (long)channels * nu;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i / nu), k = (int)(i % nu) * V;
    *reinterpret_cast<U *>(stage + (long)ch * pts1 + off + k) = *reinterpret_cast<const U *>(in + (long)ch * in_stride + k);
  }
}

// ... two sets of rows in one launch: blockIdx.y = 1 copies in_b -> stage_b
template <int V>
__global__ __launch_bounds__(256) void k_nupc_stage2(const float *__restrict__ in, long in_stride, float *__restrict__ stage,
                                                     const float *__restrict__ in_b, long in_b_stride, float *__restrict__ stage_b,
                                                     int pts1, int off, int n, int channels) {
  typedef typename RowUnit<V>::type U;
  if (blockIdx.y == 1) {
    in = in_b;
    in_stride = in_b_stride;
    stage = stage_b;
  }
  const int nu = n / V;
  const long total = (long)channels * nu;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i / nu), k = (int)(i % nu) * V;
    *reinterpret_cast<U *>(stage + (long)ch * pts1 + off + k) = *reinterpret_cast<const U *>(in + (long)ch * in_stride + k);
  }
}

// ---------------------------------------------------------------------------------
// forward transforms of one level for a time-varying block: blockIdx.y picks the job, one row per channel.  The row's
// transform is k_pconvb_fwd's (fwd_row): the bits of launch_pconvb_forward.  A job with a copy destination stores the
// pairs it loads there (the stage launch folded in); one without a frame only copies.
// ---------------------------------------------------------------------------------
template <int LOGB>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_nupc_fwd(NupcFwdJob j0, NupcFwdJob j1, int channels,
                                                               const cpx *__restrict__ tab_g, const cpx *__restrict__ w2_g) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, T = G::T, WG = G::WG, FPW = G::FPW;
  const NupcFwdJob &job = blockIdx.y ? j1 : j0;
  const float *src0 = job.src;
  const long stride = job.stride, copy_stride = job.copy_stride;
  const int aligned = job.aligned;
  cpx *frame = job.frame;
  float *copy = job.copy;
  const long fstride = (long)job.frames * N;
  const int tid = threadIdx.x;
  if (!frame) {   // (the whole launch row of workgroups: no barrier is skipped by a part of one)
    if (copy) {
      const long total = (long)channels * (N / 2);
      for (long i = (long)blockIdx.x * WG + tid; i < total; i += (long)gridDim.x * WG) {
        const int ch = (int)(i / (N / 2)), p = (int)(i % (N / 2));
        *reinterpret_cast<cpx *>(copy + ch * copy_stride + 2 * p) = ld_pair(src0 + ch * stride + 2 * p, aligned);
      }
    }
    return;
  }
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[FPW * G::PADN];
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();
  cpx *xb = s_x + f * G::PADN;
  const long groups = ((long)channels + FPW - 1) / FPW;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long r = g * FPW + f;
    const bool active = r < channels;
    const long ch = active ? r : 0;
    float *cp = copy ? copy + ch * copy_stride : nullptr;
    fwd_row<LOGB>(src0 + ch * stride, aligned, active, frame + ch * fstride, t, s_tab, xb, w2_g, [&](int p, cpx v) {
      if (cp) *reinterpret_cast<cpx *>(cp + 2 * p) = v;
    });
  }
}

// ---------------------------------------------------------------------------------
// mix: out[ch][0 .. n) = out[ch][0 .. n) + pend[ch][off .. off + n)   (out holds the head's samples)
// ---------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_nupc_mix(float *out, long out_stride, const float *__restrict__ pend, int pts1, int off,
                                                  int n, int channels) {
  typedef typename RowUnit<V>::type U;
  const int nu = n / V;
  const long total = (long)channels * nu;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i / nu), k = (int)(i % nu) * V;
    U *o = reinterpret_cast<U *>(out + (long)ch * out_stride + k);
    *o = *o + *reinterpret_cast<const U *>(pend + (long)ch * pts1 + off + k);
  }
}

// ---------------------------------------------------------------------------------
// fade mix: a = out + pendA (the first path, as k_nupc_mix), b = headB + pendB (the second), out = a + g * (b - a) with
// g = (float)n / N, n = n0 + the sample's index in the row: a division, a subtraction, a multiplication and an addition,
// each rounded on its own
// ---------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_nupc_fade_mix(float *out, long out_stride, const float *__restrict__ headB,
                                                       const float *__restrict__ pendA, const float *__restrict__ pendB, int pts1,
                                                       int off, int n, int channels, long n0, float N) {
#pragma clang fp contract(off)
  typedef typename RowUnit<V>::type U;
  const int nu = n / V;
  const long total = (long)channels * nu;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i / nu), k = (int)(i % nu) * V;
    U *o = reinterpret_cast<U *>(out + (long)ch * out_stride + k);
    const U a = *o + *reinterpret_cast<const U *>(pendA + (long)ch * pts1 + off + k);
    const U b = *reinterpret_cast<const U *>(headB + (long)ch * n + k) + *reinterpret_cast<const U *>(pendB + (long)ch * pts1 + off + k);
    U g;
    if constexpr (V == 1) {
      g = (float)(n0 + k) / N;
    } else {
#pragma unroll
      for (int v = 0; v < V; v++) g[v] = (float)(n0 + k + v) / N;
    }
    const U d = b - a;
    const U gd = g * d;
    *o = a + gd;
  }
}

// ---------------------------------------------------------------------------------
// multiply-accumulate of ONE block of a level over items [item0, item0 + nitems) of every channel: one lane = (channel,
// item), the lanes laid over both together, so that a slice of 16 items still fills its waves.  The partitions are one
// serial chain per lane (the order is the result's bits), so what hides the memory latency is depth: the loads of D
// partitions are in flight together.  blockIdx.y picks the job: a single-block call runs the head's block (all its items)
// and the tail's slice side by side in one launch (NJ = 2); a fade's block runs both under both response sets (NJ = 4).
// ---------------------------------------------------------------------------------
template <int NJ> struct NupcMacJobs { NupcMacJob j[NJ]; };

template <int D, int NJ>
__global__ __launch_bounds__(64) void k_nupc_mac(NupcMacJobs<NJ> jobs, int channels) {
  static_assert(NJ == 2 || NJ == kNupcMacJobs, "two jobs, or a fade's four");
  const NupcMacJob &job = NJ > 2 && blockIdx.y >= 2 ? (blockIdx.y == 3 ? jobs.j[NJ - 1] : jobs.j[NJ - 2]) : (blockIdx.y ? jobs.j[1] : jobs.j[0]);
  const cpx *__restrict__ ringA = job.ringA;
  const cpx *__restrict__ ringB = job.ringB;
  cpx *__restrict__ Y = job.Y;
  const int w = job.w, bins = job.bins, nparts = job.nparts, ring = job.ring, item0 = job.item0, nitems = job.nitems;
  if (blockIdx.x * 64L >= (long)channels * nitems) return;   // (the grid is the larger job's)
  const int hb = bins >> 1;
  const long total = (long)channels * nitems;
  const long gid = blockIdx.x * 64L + threadIdx.x;
  const long g = gid < total ? gid : total - 1;   // (clamped: straight-line loads; the store is guarded)
  const int ch = (int)(g / nitems), item = item0 + (int)(g % nitems);
  const cpx2 *ra = reinterpret_cast<const cpx2 *>(ringA + (long)ch * ring * bins) + item;
  const cpx2 *rb = reinterpret_cast<const cpx2 *>(ringB + (long)ch * nparts * bins) + item;
  // input frame of partition p: block (p - (nparts - 1)) counted from the new one, ring frame (w + that) mod ring; the
  // new block's own spectrum is frame w (p = nparts - 1).  Past the last partition: clamped, never used
  auto frame = [&](int p) -> const cpx2 * {
    p = p < nparts ? p : nparts - 1;
    int f = w - (nparts - 1) + p;
    f = f < 0 ? f + ring : f;
    return ra + (long)f * hb;
  };
  auto resp = [&](int p) -> const cpx2 * { return rb + (long)(p < nparts ? p : nparts - 1) * hb; };
  const bool dc = item == 0;   // packed DC / Nyquist bin: (re*re, im*im)
  cpx s0 = mk(0.f, 0.f), s1 = mk(0.f, 0.f);
  cpx2 xq[D], hq[D];
#pragma unroll
  for (int d = 0; d < D; d++) {
    xq[d] = ld_nt(frame(d));
    hq[d] = ld_nt(resp(d));
  }
  for (int p0 = 0; p0 < nparts; p0 += D) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      const cpx2 x = xq[d], h = hq[d];
      xq[d] = ld_nt(frame(p0 + d + D));
      hq[d] = ld_nt(resp(p0 + d + D));
      // past the last partition the term is dropped by a select on the sums, not by a branch: a branch in the body ends
      // the overlap of the loads with the arithmetic
      cpx t0 = s0, t1 = s1;
      mac_term(t0, t1, x, h, dc);
      const bool live = p0 + d < nparts;
      s0 = mk(live ? t0.x : s0.x, live ? t0.y : s0.y);
      s1 = mk(live ? t1.x : s1.x, live ? t1.y : s1.y);
    }
  }
  if (gid < total) {
    cpx2 o;
    o.a = s0;
    o.b = s1;
    reinterpret_cast<cpx2 *>(Y + (long)ch * bins)[item] = o;
  }
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
static bool rows_16(const void *p, long stride) { return ((uintptr_t)p & 15) == 0 && (stride & 3) == 0; }

hipError_t launch_nupc_stage(const float *in, long in_stride, float *stage, int pts1, int off, int n, int channels,
                             hipStream_t s) {
  if (n < 1 || (n & 31) || (off & 31) || off + n > pts1) return hipErrorInvalidValue;
  const bool v4 = rows_16(in, in_stride);   // (the stage row itself: hipMalloc'ed, pts1 and off multiples of 32)
  const int grid = grid_clamp(((long)channels * (n / (v4 ? 4 : 1)) + 255) / 256, 4096);
  if (v4) hipLaunchKernelGGL(k_nupc_stage<4>, dim3(grid), dim3(256), 0, s, in, in_stride, stage, pts1, off, n, channels);
  else hipLaunchKernelGGL(k_nupc_stage<1>, dim3(grid), dim3(256), 0, s, in, in_stride, stage, pts1, off, n, channels);
  return hipGetLastError();
}

hipError_t launch_nupc_stage2(const float *in, long in_stride, float *stage, const float *in_b, long in_b_stride, float *stage_b,
                              int pts1, int off, int n, int channels, hipStream_t s) {
  if (n < 1 || (n & 31) || (off & 31) || off + n > pts1) return hipErrorInvalidValue;
  const bool v4 = rows_16(in, in_stride) && rows_16(in_b, in_b_stride);
  const int grid = grid_clamp(((long)channels * (n / (v4 ? 4 : 1)) + 255) / 256, 4096);
  if (v4)
    hipLaunchKernelGGL(k_nupc_stage2<4>, dim3(grid, 2), dim3(256), 0, s, in, in_stride, stage, in_b, in_b_stride, stage_b, pts1, off, n, channels);
  else
    hipLaunchKernelGGL(k_nupc_stage2<1>, dim3(grid, 2), dim3(256), 0, s, in, in_stride, stage, in_b, in_b_stride, stage_b, pts1, off, n, channels);
  return hipGetLastError();
}

hipError_t launch_nupc_fwd(int logb, const NupcFwdJob *jobs, int njobs, int channels, const cpx *half, const cpx *w2f, hipStream_t s) {
  if (njobs < 1 || njobs > 2 || channels < 1) return hipErrorInvalidValue;
  for (int i = 0; i < njobs; i++) {
    const NupcFwdJob &j = jobs[i];
    if (!j.src || (!j.frame && !j.copy) || (j.frame && j.frames < 1) || ((uintptr_t)j.copy & 7) || (j.copy_stride & 1))
      return hipErrorInvalidValue;
  }
  return dispatch_logb<kPconvBlocksMinLog, kPconvBlocksMaxLog>(logb, [&](auto L) {
    using G = LdsGeom<decltype(L)::value>;
    const int grid = grid_clamp(((long)channels + G::FPW - 1) / G::FPW, 8192);
    hipLaunchKernelGGL((k_nupc_fwd<decltype(L)::value>), dim3(grid, njobs), dim3(G::WG), 0, s, jobs[0], jobs[njobs - 1], channels, half, w2f);
    return hipGetLastError();
  });
}

hipError_t launch_nupc_mix(float *out, long out_stride, const float *pend, int pts1, int off, int n, int channels,
                           hipStream_t s) {
  if (n < 1 || (n & 31) || (off & 31) || off + n > pts1) return hipErrorInvalidValue;
  const bool v4 = rows_16(out, out_stride);
  const int grid = grid_clamp(((long)channels * (n / (v4 ? 4 : 1)) + 255) / 256, 4096);
  if (v4) hipLaunchKernelGGL(k_nupc_mix<4>, dim3(grid), dim3(256), 0, s, out, out_stride, pend, pts1, off, n, channels);
  else hipLaunchKernelGGL(k_nupc_mix<1>, dim3(grid), dim3(256), 0, s, out, out_stride, pend, pts1, off, n, channels);
  return hipGetLastError();
}

hipError_t launch_nupc_fade_mix(float *out, long out_stride, const float *headB, const float *pendA, const float *pendB, int pts1,
                                int off, int n, int channels, long n0, float N, hipStream_t s) {
  if (n < 1 || (n & 31) || (off & 31) || off + n > pts1 || n0 < 0 || !(N > 0.f)) return hipErrorInvalidValue;
  const bool v4 = rows_16(out, out_stride) && rows_16(headB, n);   // (the pending rows: as launch_nupc_mix's)
  const int grid = grid_clamp(((long)channels * (n / (v4 ? 4 : 1)) + 255) / 256, 4096);
  if (v4)
    hipLaunchKernelGGL(k_nupc_fade_mix<4>, dim3(grid), dim3(256), 0, s, out, out_stride, headB, pendA, pendB, pts1, off, n, channels, n0, N);
  else
    hipLaunchKernelGGL(k_nupc_fade_mix<1>, dim3(grid), dim3(256), 0, s, out, out_stride, headB, pendA, pendB, pts1, off, n, channels, n0, N);
  return hipGetLastError();
}

hipError_t launch_nupc_mac(const NupcMacJob *jobs, int njobs, int channels, hipStream_t s) {
  if (njobs < 1 || njobs > kNupcMacJobs) return hipErrorInvalidValue;
  long blocks = 0;
  for (int i = 0; i < njobs; i++) {
    const NupcMacJob &j = jobs[i];
    if (j.item0 < 0 || j.nitems < 1 || j.item0 + j.nitems > j.bins / 2 || j.nparts < 1 || j.ring < j.nparts || j.w < 0 || j.w >= j.ring)
      return hipErrorInvalidValue;
    const long b = ((long)channels * j.nitems + 63) / 64;
    blocks = b > blocks ? b : blocks;
  }
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  // (jobs past njobs repeat the last one: blockIdx.y never picks them)
  if (njobs > 2) {
    NupcMacJobs<kNupcMacJobs> a;
    for (int i = 0; i < kNupcMacJobs; i++) a.j[i] = jobs[i < njobs ? i : njobs - 1];
    hipLaunchKernelGGL((k_nupc_mac<kNupcMacDepth, kNupcMacJobs>), dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, channels);
  } else {
    const NupcMacJobs<2> a = {{jobs[0], jobs[njobs - 1]}};
    hipLaunchKernelGGL((k_nupc_mac<kNupcMacDepth, 2>), dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, channels);
  }
  return hipGetLastError();
}

}  // namespace clfa
