// pconv_matrix.hip — convolution matrix: `inputs` signals mixed into `outputs` signals through an outputs x inputs matrix of
// partitioned responses, y_o = sum_i x_i * h_{o,i} (clfa_pconv_matrix), partitions of 32..4096 samples.
//
// Per sub-batch of K blocks, whatever K:
//   k_pconvb_fwd      spectra of the inputs x K new blocks -> workspace X (pconv_blocks.hip, channels = inputs)
//   k_pconvm_mac      Y_{o,j} = sum_i sum_p F_i(j, p) (.) H_{o,i}(nparts - 1 - p) over one segment of the sequence
//                     r = i * nparts + p: the response frame (o, i, p) is loaded ONCE for a tile of KT consecutive
//                     outputs j, and input i's frames slide through a register window by one per partition
//   k_pconvm_reduce   (segs > 1) Y += P[0], Y += P[1], ... in ascending segment order
//   k_pconvb_inv      c2r + inverse transform + overlap-add of Y into the output rows, one tail per output
//   k_pconvm_commit   the last nparts spectra of every input -> ring A, the new tails -> the object
// Frame algebra (block j of the sub-batch, w = the object's ring position before it): the input frame of partition p for
// output j is m = j - (nparts - 1) + p; m >= 0: X_i[m], m < 0: ring A_i frame (w + m) mod nparts.
// Every output bin of segment s is one accumulator over its r in ascending order; the segments are fixed per object
// (pconv_matrix_plan), and so is the order in which they are added: results do not depend on K, the sub-batch, the split
// of a signal into calls, the stream or graph replay.
//
// A sub-batch inside a timed crossfade (launch_pconv_matrix_fade; contract in clfft_amd.h) runs a second path over the same
// X and ring A: k_pconvm_mac_fade reads each input frame once against the frames of both response sets (H -> Y / P, H2 ->
// Y2 / P2), reduce and inverse run per path (the second with its own tails, into a scratch of samples), k_pconvm_mix forms
// a + g * (b - a) in place, and the commit also takes the second tails.  launch_pconv_matrix_prime starts the second path's
// tails at the push: the block before the next one under H2, whose nparts input frames are exactly what ring A holds.
#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

namespace {

__device__ __forceinline__ long seg_start(long total, int s, int segs) { return total * s / segs; }

}  // namespace

// ---------------------------------------------------------------------------------
// multiply-accumulate: one wave = (64 items of two bins, tile of KT outputs, output o, segment s), flattened into x
// ---------------------------------------------------------------------------------
template <int KT>
__global__ __launch_bounds__(64) void k_pconvm_mac(const cpx *__restrict__ ringA, const cpx *__restrict__ H,
                                                   const cpx *__restrict__ X, cpx *__restrict__ Y, cpx *__restrict__ P, int K,
                                                   int cap, int w, int bins, int nparts, int inputs, int outputs, int segs) {
  const int hb = bins >> 1;
  const int slices = (hb + 63) / 64, tiles = (K + KT - 1) / KT;
  long b = blockIdx.x;
  const int slice = (int)(b % slices);
  b /= slices;
  const int tile = (int)(b % tiles);
  b /= tiles;
  const int o = (int)(b % outputs);
  const int s = (int)(b / outputs);
  const int item = slice * 64 + threadIdx.x;
  const int it = item < hb ? item : hb - 1;   // (clamped: straight-line loads; the store is guarded)
  const int j0 = tile * KT;
  const long total = (long)inputs * nparts;
  const long r0 = seg_start(total, s, segs), r1 = seg_start(total, s + 1, segs);
  const bool dc = item == 0;   // packed DC / Nyquist bin: (re*re, im*im)
  cpx s0[KT], s1[KT];
#pragma unroll
  for (int t = 0; t < KT; t++) s0[t] = s1[t] = mk(0.f, 0.f);
  // (the lambda stays: with mac_term called straight from the unrolled loop hipcc emits another code object)
  auto mac = [&](int t, const cpx2 &x, const cpx2 &h) {
    mac_term(s0[t], s1[t], x, h, dc);
  };
  for (int i = (int)(r0 / nparts); (long)i * nparts < r1; i++) {
    const long ib = (long)i * nparts;
    const int pa = r0 > ib ? (int)(r0 - ib) : 0;
    const int pb = r1 - ib < nparts ? (int)(r1 - ib) : nparts;
    const cpx2 *ra = reinterpret_cast<const cpx2 *>(ringA + ib * bins) + it;
    const cpx2 *xs = reinterpret_cast<const cpx2 *>(X + (long)i * cap * bins) + it;
    // partition q of response (o, i); step p of the walk uses q = nparts - 1 - p
    const cpx2 *hp = reinterpret_cast<const cpx2 *>(H + ((long)o * inputs + i) * nparts * bins) + it;
    // input frame m of the sub-batch: m >= 0 this call's spectrum X_i[m]; m < 0 ring A_i frame (w + m) mod nparts.
    // m > K - 1 only feeds outputs past the sub-batch (never stored): clamped
    auto frame = [&](int m) -> const cpx2 * {
      if (m >= 0) return xs + (long)(m < K ? m : K - 1) * hb;
      int f = w + m;
      f = f < 0 ? f + nparts : f;
      return ra + (long)f * hb;
    };
    cpx2 win[KT];
#pragma unroll
    for (int t = 0; t < KT; t++) win[t] = ld_nt(frame(j0 + t - (nparts - 1) + pa));
    cpx2 hq, xq;
    auto load = [&](int p) {
      hq = ld_nt(hp + (long)(nparts - 1 - p) * hb);
      xq = ld_nt(frame(j0 + KT - (nparts - 1) + p));   // enters the window after partition p
    };
    load(pa);
    for (int p = pa; p < pb; p++) {
      const cpx2 h = hq, xn = xq;
      if (p + 1 < pb) load(p + 1);   // next partition's loads are in flight under this one's arithmetic
#pragma unroll
      for (int t = 0; t < KT; t++) mac(t, win[t], h);
      window_shift(win, xn);
    }
  }
  if (item < hb) {
    cpx2 *dst = reinterpret_cast<cpx2 *>(s == 0 ? Y + (long)o * cap * bins : P + ((long)(s - 1) * outputs + o) * cap * bins);
#pragma unroll
    for (int t = 0; t < KT; t++) {
      const int j = j0 + t;
      if (j < K) {
        cpx2 v;
        v.a = s0[t];
        v.b = s1[t];
        dst[(long)j * hb + item] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// the same walk for a fade.  SETS = 2: every input frame also meets the frame of a second response set H2, in a second set
// of accumulators written to Y2 / P2; per accumulator the terms and their order are those of k_pconvm_mac, so each set has
// that kernel's bits.  shift: the outputs are the blocks j + shift of the sub-batch (-1 with K = 1: the block before it,
// from ring A alone, for the second tails).  (A kernel of its own: k_pconvm_mac keeps its text, because every way of
// sharing this walk with it, a wave function or template flags, gave it another code object: tools/check_isa.py --same.)
// ---------------------------------------------------------------------------------
template <int KT, int SETS>
__global__ __launch_bounds__(64) void k_pconvm_mac_fade(const cpx *__restrict__ ringA, const cpx *__restrict__ H,
                                                        const cpx *__restrict__ H2, const cpx *__restrict__ X,
                                                        cpx *__restrict__ Y, cpx *__restrict__ P, cpx *__restrict__ Y2,
                                                        cpx *__restrict__ P2, int K, int cap, int w, int shift, int bins,
                                                        int nparts, int inputs, int outputs, int segs) {
  const int hb = bins >> 1;
  const int slices = (hb + 63) / 64, tiles = (K + KT - 1) / KT;
  long b = blockIdx.x;
  const int slice = (int)(b % slices);
  b /= slices;
  const int tile = (int)(b % tiles);
  b /= tiles;
  const int o = (int)(b % outputs);
  const int s = (int)(b / outputs);
  const int item = slice * 64 + threadIdx.x;
  const int it = item < hb ? item : hb - 1;   // (clamped: straight-line loads; the store is guarded)
  const int j0 = tile * KT;
  const long total = (long)inputs * nparts;
  const long r0 = seg_start(total, s, segs), r1 = seg_start(total, s + 1, segs);
  const bool dc = item == 0;   // packed DC / Nyquist bin: (re*re, im*im)
  cpx s0[KT], s1[KT], u0[KT], u1[KT];   // (u0, u1: the second set's)
#pragma unroll
  for (int t = 0; t < KT; t++) s0[t] = s1[t] = mk(0.f, 0.f);
  if (SETS > 1) {
#pragma unroll
    for (int t = 0; t < KT; t++) u0[t] = u1[t] = mk(0.f, 0.f);
  }
  // (the lambda stays: with mac_term called straight from the unrolled loop hipcc emits another code object)
  auto mac = [&](int t, const cpx2 &x, const cpx2 &h) {
    mac_term(s0[t], s1[t], x, h, dc);
  };
  auto mac2 = [&](int t, const cpx2 &x, const cpx2 &h) {
    mac_term(u0[t], u1[t], x, h, dc);
  };
  for (int i = (int)(r0 / nparts); (long)i * nparts < r1; i++) {
    const long ib = (long)i * nparts;
    const int pa = r0 > ib ? (int)(r0 - ib) : 0;
    const int pb = r1 - ib < nparts ? (int)(r1 - ib) : nparts;
    const cpx2 *ra = reinterpret_cast<const cpx2 *>(ringA + ib * bins) + it;
    const cpx2 *xs = reinterpret_cast<const cpx2 *>(X + (long)i * cap * bins) + it;
    // partition q of response (o, i); step p of the walk uses q = nparts - 1 - p
    const cpx2 *hp = reinterpret_cast<const cpx2 *>(H + ((long)o * inputs + i) * nparts * bins) + it;
    const cpx2 *hp2 = SETS > 1 ? reinterpret_cast<const cpx2 *>(H2 + ((long)o * inputs + i) * nparts * bins) + it : hp;
    // input frame m of the sub-batch: m >= 0 this call's spectrum X_i[m]; m < 0 ring A_i frame (w + m) mod nparts
    // (m >= -nparts).  m > K - 1 only feeds outputs past the sub-batch (never stored): clamped
    auto frame = [&](int m) -> const cpx2 * {
      if (m >= 0) return xs + (long)(m < K ? m : K - 1) * hb;
      int f = w + m;
      f = f < 0 ? f + nparts : f;
      return ra + (long)f * hb;
    };
    cpx2 win[KT];
#pragma unroll
    for (int t = 0; t < KT; t++) win[t] = ld_nt(frame(j0 + shift + t - (nparts - 1) + pa));
    cpx2 hq, hq2{}, xq;
    auto load = [&](int p) {
      hq = ld_nt(hp + (long)(nparts - 1 - p) * hb);
      if (SETS > 1) hq2 = ld_nt(hp2 + (long)(nparts - 1 - p) * hb);
      xq = ld_nt(frame(j0 + shift + KT - (nparts - 1) + p));   // enters the window after partition p
    };
    load(pa);
    for (int p = pa; p < pb; p++) {
      const cpx2 h = hq, h2 = hq2, xn = xq;
      if (p + 1 < pb) load(p + 1);   // next partition's loads are in flight under this one's arithmetic
#pragma unroll
      for (int t = 0; t < KT; t++) mac(t, win[t], h);
      if (SETS > 1) {
#pragma unroll
        for (int t = 0; t < KT; t++) mac2(t, win[t], h2);
      }
      window_shift(win, xn);
    }
  }
  if (item < hb) {
    cpx2 *dst = reinterpret_cast<cpx2 *>(s == 0 ? Y + (long)o * cap * bins : P + ((long)(s - 1) * outputs + o) * cap * bins);
#pragma unroll
    for (int t = 0; t < KT; t++) {
      const int j = j0 + t;
      if (j < K) {
        cpx2 v;
        v.a = s0[t];
        v.b = s1[t];
        dst[(long)j * hb + item] = v;
      }
    }
    if (SETS > 1) {
      dst = reinterpret_cast<cpx2 *>(s == 0 ? Y2 + (long)o * cap * bins : P2 + ((long)(s - 1) * outputs + o) * cap * bins);
#pragma unroll
      for (int t = 0; t < KT; t++) {
        const int j = j0 + t;
        if (j < K) {
          cpx2 v;
          v.a = u0[t];
          v.b = u1[t];
          dst[(long)j * hb + item] = v;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// the segments' partial sums, added in ascending segment order: Y = ((Y_0 + P_1) + P_2) + ...
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pconvm_reduce(cpx *__restrict__ Y, const cpx *__restrict__ P, int K, int cap, int bins,
                                                       int outputs, int segs) {
  const int hb = bins >> 1;
  const long n = (long)outputs * K * hb;
  const long pstride = (long)outputs * cap * hb;   // one segment's partials, in cpx2
  cpx2 *y = reinterpret_cast<cpx2 *>(Y);
  const cpx2 *q = reinterpret_cast<const cpx2 *>(P);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int item = (int)(i % hb);
    const long rest = i / hb;
    const int j = (int)(rest % K), o = (int)(rest / K);
    const long at = ((long)o * cap + j) * hb + item;
    cpx2 v = y[at];
    for (int s = 1; s < segs; s++) {
      const cpx2 u = q[(long)(s - 1) * pstride + at];
      v.a = cadd(v.a, u.a);
      v.b = cadd(v.b, u.b);
    }
    y[at] = v;
  }
}

// ---------------------------------------------------------------------------------
// commit: y = 0 the last min(K, nparts) spectra of every input -> ring A frame (w + m) mod nparts; y = 1 the new tails
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pconvm_commit(cpx *__restrict__ ringA, float *__restrict__ tail, const cpx *__restrict__ X,
                                                       const float *__restrict__ tail_new, int K, int cap, int w, int bins,
                                                       int nparts, int inputs, int outputs) {
  const int hb = bins >> 1;
  if (blockIdx.y == 1) return commit_tail(tail, tail_new, (long)outputs * bins);
  commit_spectra(ringA, X, commit_first(K, nparts), K, cap, hb, nparts, inputs,
                 [&](int m) { return ring_a_frame(w, m, nparts); });
}

// ... and the second tails of a fade
__global__ __launch_bounds__(256) void k_pconvm_commit_tail(float *__restrict__ tail, const float *__restrict__ tail_new, long n) {
  commit_tail(tail, tail_new, n);
}

// ---------------------------------------------------------------------------------
// crossfade: out = a + g * (b - a) in place, a = the first path's sample in `out`, b = the second path's in `mix`,
// g = (float)n / (float)N for sample n of the fade (n0 = that of the sub-batch's first sample), each operation rounded
// on its own
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pconvm_mix(float *__restrict__ out, long out_stride, const float *__restrict__ mix,
                                                    long mix_stride, long len, int outputs, long n0, float N) {
#pragma clang fp contract(off)
  const long n = (long)outputs * len;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long o = i / len, k = i % len;
    const float g = (float)(n0 + k) / N;
    float *dst = out + o * out_stride + k;
    const float a = *dst, d = mix[o * mix_stride + k] - a;
    *dst = a + g * d;
  }
}

// ---------------------------------------------------------------------------------
// plan and launchers
// ---------------------------------------------------------------------------------
PconvMatrixPlan pconv_matrix_plan(int bins, int nparts, int inputs, int outputs, const DeviceInfo &di) {
  // The (input, partition) reduction is split until one tile of outputs has about eight waves per CU: with few outputs and
  // bins the item x output axes alone give a handful of waves (16 -> 2 at 512 bins: 8), and each wave's chain of dependent
  // loads is as long as its segment, so short segments hide the latency (profiles/pconv_matrix_r07.txt: 64 x 64 at 256
  // bins, K = 1, 218 us per block with 4 segments, 125 with 16).  A segment keeps at least 16 steps, so the window refills
  // and the partial sums stay small against the response traffic.  Long tiles once the segments alone fill the chip.
  // Fixed per object: the order of every output bin's sums never depends on K.
  PconvMatrixPlan pl;
  const long slices = (bins / 2 + 63) / 64;
  const long base = slices * outputs;
  const long total = (long)inputs * nparts;
  long segs = (8L * di.num_cus + base - 1) / base;
  const long most = total / 16 > 1 ? total / 16 : 1;
  segs = segs < most ? segs : most;
  segs = segs < 256 ? segs : 256;
  pl.segs = (int)(segs < 1 ? 1 : segs);
  pl.kt = base * pl.segs >= di.num_cus ? 16 : 4;
  return pl;
}

namespace {

bool args_ok(const PconvMatrixArgs &a) {
  const PconvMatrixPlan &pl = a.plan;
  return !(a.K < 1 || a.K > a.cap || (pl.kt != 4 && pl.kt != 16) || pl.segs < 1 || a.run < 1 || a.logb < kPconvBlocksMinLog ||
           a.logb > kPconvBlocksMaxLog || (pl.segs > 1 && !a.P));
}

// grid of a MAC launch at a tile of kt outputs; 0: too large
long mac_grid(const PconvMatrixArgs &a, int kt) {
  const long slices = (a.bins / 2 + 63) / 64, tiles = (a.K + kt - 1) / kt;
  const long grid = slices * tiles * a.outputs * a.plan.segs;
  return grid > 0x7fffffffL ? 0 : grid;
}

hipError_t launch_mac(const PconvMatrixArgs &a, const cpx *H, cpx *Y, cpx *P, hipStream_t s) {
  const long grid = mac_grid(a, a.plan.kt);
  if (!grid) return hipErrorInvalidValue;
#define CLFA_MAC(KT)                                                                                                    \
  hipLaunchKernelGGL((k_pconvm_mac<KT>), dim3((unsigned)grid), dim3(64), 0, s, (const cpx *)a.ringA, H, (const cpx *)a.X, Y, P, \
                     a.K, a.cap, a.w, a.bins, a.nparts, a.inputs, a.outputs, a.plan.segs)
  if (a.plan.kt == 16) CLFA_MAC(16);
  else CLFA_MAC(4);
#undef CLFA_MAC
  return hipGetLastError();
}

hipError_t launch_reduce(const PconvMatrixArgs &a, cpx *Y, const cpx *P, hipStream_t s) {
  if (a.plan.segs == 1) return hipSuccess;
  const long n = (long)a.outputs * a.K * (a.bins / 2);
  const int grid = grid_clamp((n + 255) / 256, 8192);
  hipLaunchKernelGGL(k_pconvm_reduce, dim3(grid), dim3(256), 0, s, Y, P, a.K, a.cap, a.bins, a.outputs, a.plan.segs);
  return hipGetLastError();
}

hipError_t launch_commit(const PconvMatrixArgs &a, hipStream_t s) {
  const long n = (long)(a.inputs > a.outputs ? a.inputs : a.outputs) * a.bins;
  const int grid = grid_clamp((n + 255) / 256, 4096);
  hipLaunchKernelGGL(k_pconvm_commit, dim3(grid, 2), dim3(256), 0, s, a.ringA, a.tail, (const cpx *)a.X, (const float *)a.tail_ws,
                     a.K, a.cap, a.w, a.bins, a.nparts, a.inputs, a.outputs);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_pconv_matrix(const PconvMatrixArgs &a, hipStream_t s) {
  if (!args_ok(a)) return hipErrorInvalidValue;
  hipError_t e = launch_pconvb_forward(a.logb, a.in, a.in_stride, a.X, a.K, a.cap, a.inputs, a.aligned_in, a.half, a.w2f, s);
  if (e != hipSuccess) return e;
  if ((e = launch_mac(a, a.H, a.Y, a.P, s)) != hipSuccess) return e;
  if ((e = launch_reduce(a, a.Y, a.P, s)) != hipSuccess) return e;
  e = launch_pconvb_inverse(a.logb, a.Y, a.tail, a.tail_ws, a.out, a.out_stride, a.K, a.cap, a.run, a.outputs, a.aligned_out,
                            a.half, a.w2i, s);
  if (e != hipSuccess) return e;
  return launch_commit(a, s);
}

// ---------------------------------------------------------------------------------
// a sub-batch inside a fade: forward, both paths' MAC (one launch, or two of the plain kernel), reduce and inverse per path,
// mix, commit.  The first path's launches are those of launch_pconv_matrix on the same arguments.
// ---------------------------------------------------------------------------------
static bool fade_args_ok(const PconvMatrixArgs &a) {
  return args_ok(a) && a.H2 && a.tail2 && a.Y2 && a.tail_ws2 && a.mix && (a.plan.segs == 1 || a.P2);
}

hipError_t launch_pconv_matrix_fade(const PconvMatrixArgs &a, hipStream_t s) {
  if (!fade_args_ok(a) || a.fade_pos < 0 || a.K > a.fade_len - a.fade_pos || a.fade_len > 0x7fffffffL / a.bins)
    return hipErrorInvalidValue;
  hipError_t e = launch_pconvb_forward(a.logb, a.in, a.in_stride, a.X, a.K, a.cap, a.inputs, a.aligned_in, a.half, a.w2f, s);
  if (e != hipSuccess) return e;
  if (a.two_mac) {
    if ((e = launch_mac(a, a.H, a.Y, a.P, s)) != hipSuccess || (e = launch_mac(a, a.H2, a.Y2, a.P2, s)) != hipSuccess) return e;
  } else {
    // always at a tile of 4 outputs (the tile enters no sum): two accumulator sets at a tile of 16 need 362 registers per
    // lane, one wave per SIMD, and were slower in five of six cases (profiles/pconv_matrix_fade_r10.txt)
    const long grid = mac_grid(a, 4);
    if (!grid) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_pconvm_mac_fade<4, 2>), dim3((unsigned)grid), dim3(64), 0, s, (const cpx *)a.ringA, a.H, a.H2,
                       (const cpx *)a.X, a.Y, a.P, a.Y2, a.P2, a.K, a.cap, a.w, 0, a.bins, a.nparts, a.inputs, a.outputs,
                       a.plan.segs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = launch_reduce(a, a.Y, a.P, s)) != hipSuccess || (e = launch_reduce(a, a.Y2, a.P2, s)) != hipSuccess) return e;
  e = launch_pconvb_inverse(a.logb, a.Y, a.tail, a.tail_ws, a.out, a.out_stride, a.K, a.cap, a.run, a.outputs, a.aligned_out,
                            a.half, a.w2i, s);
  if (e != hipSuccess) return e;
  const long mix_stride = (long)a.cap * a.bins;
  e = launch_pconvb_inverse(a.logb, a.Y2, a.tail2, a.tail_ws2, a.mix, mix_stride, a.K, a.cap, a.run, a.outputs, 1, a.half,
                            a.w2i, s);
  if (e != hipSuccess) return e;
  {
    const long len = (long)a.K * a.bins;
    const int grid = grid_clamp((a.outputs * len + 255) / 256, 8192);
    hipLaunchKernelGGL(k_pconvm_mix, dim3(grid), dim3(256), 0, s, a.out, a.out_stride, (const float *)a.mix, mix_stride, len,
                       a.outputs, a.fade_pos * a.bins, (float)(a.fade_len * a.bins));
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if ((e = launch_commit(a, s)) != hipSuccess) return e;
  const long n = (long)a.outputs * a.bins;
  hipLaunchKernelGGL(k_pconvm_commit_tail, dim3(grid_clamp((n + 255) / 256, 4096)), dim3(256), 0, s, a.tail2,
                     (const float *)a.tail_ws2, n);
  return hipGetLastError();
}

// the second tails at the push: the block before the next one, evaluated under H2 from ring A alone (its nparts input
// frames are exactly the ring's), through reduce and a one-block inverse whose samples are dropped
hipError_t launch_pconv_matrix_prime(const PconvMatrixArgs &a0, hipStream_t s) {
  PconvMatrixArgs a = a0;
  a.K = 1;
  if (!fade_args_ok(a) || !a.X) return hipErrorInvalidValue;
  const long grid = mac_grid(a, 4);
  if (!grid) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_pconvm_mac_fade<4, 1>), dim3((unsigned)grid), dim3(64), 0, s, (const cpx *)a.ringA, a.H2,
                     (const cpx *)nullptr, (const cpx *)a.X, a.Y2, a.P2, (cpx *)nullptr, (cpx *)nullptr, 1, a.cap, a.w, -1, a.bins,
                     a.nparts, a.inputs, a.outputs, a.plan.segs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || (e = launch_reduce(a, a.Y2, a.P2, s)) != hipSuccess) return e;
  return launch_pconvb_inverse(a.logb, a.Y2, a.tail, a.tail2, a.mix, (long)a.cap * a.bins, 1, a.cap, a.run, a.outputs, 1,
                               a.half, a.w2i, s);
}

}  // namespace clfa
