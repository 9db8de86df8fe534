// pconv_fused.inc (part of the translation unit pconv_chain.hip) — one block of the partitioned convolution in ONE launch,
// one workgroup per channel (k_pconv_fused); restates cl_conv.cpp:393-458 / 460-548 and cl_conv_kernels.h:46-124.  It
// replaces the launch chain of pconv_chain.hip when there are enough channels to fill the chip.
#include "pconv_device.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// fused block: forward FFT -> MAC over all partitions -> inverse FFT + overlap-add, one
// workgroup per channel, ONE launch per block (used when there are enough channels to fill the
// chip).  Everything a channel needs stays inside its workgroup, so the only synchronisation is
// __syncthreads(): the new spectrum frame is stored to the ring and re-read by the same
// workgroup (workgroup-scope visibility), the accumulator lives in LDS.
// ---------------------------------------------------------------------------------
template <int LOGB, bool TV, bool DEEP = false>
__global__ __launch_bounds__(256) void k_pconv_fused(const float *__restrict__ in1, const float *__restrict__ in2,
                                                     cpx *__restrict__ ringA, cpx *__restrict__ ringB,
                                                     float *__restrict__ tail, float *__restrict__ out, int frame1,
                                                     int frame2, int wp, int nparts, const cpx *__restrict__ tab_g,
                                                     const cpx *__restrict__ w2f_g, const cpx *__restrict__ w2i_g) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T;   // N = bins; T = N/16 lanes run the FFTs
  static_assert(T <= 256 && N / 2 >= 256, "fused block kernel covers bins 512..4096");
  constexpr int HB = N / 2, IPT = HB / 256;     // 16-byte items (two bins) per lane in the MAC
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[G::PADN];
  __shared__ cpx s_acc[N];
  const int tid = threadIdx.x;
  const int ch = blockIdx.x;
  for (int i = tid; i < N / 2; i += 256) s_tab[i] = tab_g[i];
  __syncthreads();

  // ---- forward chain(s): reference reorder + fft + r2c (cl_conv.cpp:399-419 / 465-513) ----------
  auto forward_load = [&](const float *in, cpx (&v)[E]) {
    if (tid < T) {
      const cpx *src = reinterpret_cast<const cpx *>(in + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int p = tid + T * e;
        v[e] = p < N / 2 ? src[p] : mk(0.f, 0.f);
      }
    }
  };
  auto forward_rest = [&](cpx (&v)[E], cpx *ring, int frame) {
    // all 256 lanes walk the barriers; lanes >= T carry dummies and touch no LDS slot of the transform
    if (tid < T) pass_compute<LOGB, G::LOGE, 0, true>(v, tid, s_tab);
    constexpr int LOGR0 = pass_logr(LOGB, G::LOGE, 0);
    static_assert(LOGR0 == 4, "16 points per lane");
    // unrolled pass chain with workgroup-wide barriers
    __syncthreads();
    if (tid < T) pass_scatter<LOGB, G::LOGE, 0>(v, tid, [&](int p, cpx val) { s_x[lds_pad(p)] = val; });
    __syncthreads();
    if (tid < T) {
      pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
      pass_compute<LOGB, G::LOGE, 4, true>(v, tid, s_tab);
    }
    if constexpr (LOGB > 8) {
      __syncthreads();
      if (tid < T) pass_scatter<LOGB, G::LOGE, 4>(v, tid, [&](int p, cpx val) { s_x[lds_pad(p)] = val; });
      __syncthreads();
      if (tid < T) {
        pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
        pass_compute<LOGB, G::LOGE, 8, true>(v, tid, s_tab);
      }
    }
    __syncthreads();
    if (tid < T) {
#pragma unroll
      for (int e = 0; e < E; e++) s_x[lds_pad(tid + T * e)] = v[e];
    }
    __syncthreads();
    cpx *x = ring + ((long)ch * nparts + frame) * N;
    for (int i = tid; i < N / 2; i += 256) {
      const int j = i == 0 ? N / 2 : N - i;
      const cpx ci = s_x[lds_pad(i)], cj = s_x[lds_pad(j)];
      cpx oi, oj;
      r2c_pack_pair(ci, cj, w2f_g[i], i == 0, oi, oj);
      x[i] = oi;
      x[j] = oj;
    }
  };
  // Fewer channels than CUs (DEEP), static response: the MAC needs the frame stored below only for its LAST partition (the ring
  // position frame1 = wp - 1 pairs with partition nparts - 1, clfa_pconv_process_dev), so the first kPre partitions are
  // requested in front of the forward chain — behind the block's own samples: the counter of outstanding loads is in order —
  // and land while it runs: a workgroup that is alone with its latency starts its MAC with a full queue (160 channels:
  // 51.2-52.1 -> 46.0-46.5 us per block).  Same products, same order of the sums.  With a workgroup on every CU it buys
  // nothing (256 channels 67.3-68.2 -> 68.7-69.5), profiles/pconv_prefetch_r05.txt.
  constexpr int kPre = (TV || !DEEP || IPT > 2) ? 0 : 8;
  const cpx2 *const mac_a = reinterpret_cast<const cpx2 *>(ringA + (long)ch * nparts * N);
  const cpx2 *const mac_b = reinterpret_cast<const cpx2 *>(ringB + (long)ch * nparts * N);
  [[maybe_unused]] cpx2 pa[kPre ? kPre : 1][IPT], pb[kPre ? kPre : 1][IPT];
  [[maybe_unused]] const bool pre = kPre > 0 && nparts >= 4 * kPre;   // uniform (9 .. 12 partitions: +3 %, 40 and more: 0 .. -12 %)
  cpx vin[E];
  forward_load(in1, vin);
  if constexpr (kPre > 0) {
    if (pre) {
#pragma unroll
      for (int q = 0; q < kPre; q++) {
        const int fq = wp + q < nparts ? wp + q : wp + q - nparts;
#pragma unroll
        for (int k = 0; k < IPT; k++) {
          pa[q][k] = ld_nt(mac_a + (long)fq * HB + tid + 256 * k);
          pb[q][k] = ld_nt(mac_b + (long)q * HB + tid + 256 * k);
        }
      }
    }
  }
  forward_rest(vin, ringA, frame1);
  if constexpr (TV) {
    forward_load(in2, vin);
    forward_rest(vin, ringB, frame2);
  }
  __syncthreads();   // the frames just stored are re-read below by this workgroup

  // ---- MAC over all partitions (reference convol, cl_conv_kernels.h:102-118) -----------------------
  {
    const cpx2 *a = mac_a;
    const cpx2 *b = mac_b;
    cpx s0[IPT], s1[IPT];
#pragma unroll
    for (int k = 0; k < IPT; k++) s0[k] = s1[k] = mk(0.f, 0.f);
    int fr = wp;
    auto mac = [&](const cpx2 (&av)[IPT], const cpx2 (&bv)[IPT]) {
#pragma unroll
      for (int k = 0; k < IPT; k++) {
        cpx pr = cmul_plain(av[k].a, bv[k].a);
        if (k == 0) {  // lane 0: packed DC / Nyquist bin, (re*re, im*im) — a select, not a branch (a branch
          const bool dc = tid == 0;   // splits the loop body and the streaming loads stop overlapping)
          pr = mk(dc ? av[k].a.x * bv[k].a.x : pr.x, dc ? av[k].a.y * bv[k].a.y : pr.y);
        }
        s0[k] = cadd(s0[k], pr);
        s1[k] = cadd(s1[k], cmul_plain(av[k].b, bv[k].b));
      }
    };
    auto step = [&](int p) {
      cpx2 av[IPT], bv[IPT];
#pragma unroll
      for (int k = 0; k < IPT; k++) {
        av[k] = ld_nt(a + (long)fr * HB + tid + 256 * k);
        bv[k] = ld_nt(b + (long)p * HB + tid + 256 * k);
      }
      mac(av, bv);
      fr = fr + 1 < nparts ? fr + 1 : 0;
    };
    int p0 = 0;
    if constexpr (kPre > 0) {
      if (pre) {
#pragma unroll
        for (int q = 0; q < kPre; q++) mac(pa[q], pb[q]);
        p0 = kPre;
        fr = wp + kPre < nparts ? wp + kPre : wp + kPre - nparts;
      }
    }
    // loads of 4 partitions in flight per lane fill the memory system when every CU has a workgroup; with fewer
    // channels than CUs (DEEP) a workgroup is alone with its latency and 8 pay (160 channels: 55.5 -> 51.8 us)
    if constexpr (DEEP) {
#pragma unroll 8
      for (int p = p0; p < nparts; p++) step(p);
    } else {
#pragma unroll 4
      for (int p = p0; p < nparts; p++) step(p);
    }
#pragma unroll
    for (int k = 0; k < IPT; k++) {
      s_acc[2 * (tid + 256 * k)] = s0[k];
      s_acc[2 * (tid + 256 * k) + 1] = s1[k];
    }
  }
  __syncthreads();

  // ---- inverse chain: c2r + inverse FFT + overlap-add (cl_conv_kernels.h:87-100, 120-124) -------------
  for (int i = tid; i < N / 2; i += 256) {
    if (i == 0) {
      const cpx c0 = s_acc[0];
      s_x[0] = mk(c0.x + c0.y, c0.x - c0.y);
      s_x[lds_pad(N / 2)] = s_acc[N / 2];
    } else {
      cpx oi, oj;
      c2r_pair(s_acc[i], s_acc[N - i], w2i_g[i], oi, oj);
      s_x[lds_pad(i)] = oi;
      s_x[lds_pad(N - i)] = oj;
    }
  }
  __syncthreads();
  {
    cpx v[E];
    if (tid < T) {
      pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
      pass_compute<LOGB, G::LOGE, 0, false>(v, tid, s_tab);
    }
    __syncthreads();
    if (tid < T) pass_scatter<LOGB, G::LOGE, 0>(v, tid, [&](int p, cpx val) { s_x[lds_pad(p)] = val; });
    __syncthreads();
    if (tid < T) {
      pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
      pass_compute<LOGB, G::LOGE, 4, false>(v, tid, s_tab);
    }
    if constexpr (LOGB > 8) {
      __syncthreads();
      if (tid < T) pass_scatter<LOGB, G::LOGE, 4>(v, tid, [&](int p, cpx val) { s_x[lds_pad(p)] = val; });
      __syncthreads();
      if (tid < T) {
        pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
        pass_compute<LOGB, G::LOGE, 8, false>(v, tid, s_tab);
      }
    }
    if (tid < T) {
      constexpr float inv = 1.0f / (float)N;
      cpx *o = reinterpret_cast<cpx *>(out + (long)ch * N);
      cpx *tl = reinterpret_cast<cpx *>(tail + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E / 2; e++) {
        const int p = tid + T * e;
        const cpx old = tl[p];
        o[p] = mk((v[e].x + old.x) * inv, (v[e].y + old.y) * inv);
        tl[p] = v[e + E / 2];
      }
    }
  }
}

bool pconv_fused_ok(const PconvGeom &g, const DeviceInfo &di) {
  // one workgroup per channel: below ~8/15 of the CUs the chip is too empty for it (measured at pts 1024, 94
  // partitions: 128 channels 48 us fused against 46 us on the three-kernel chain, 144 channels 50 against 56)
  return g.logb >= 9 && g.logb <= 12 && g.channels * 15 >= di.num_cus * 8;
}

template <int LOGB>
static hipError_t launch_fused_one(const PconvGeom &g, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                                   float *tail, float *out, int frame1, int frame2, int wp, const cpx *half,
                                   const cpx *w2f, const cpx *w2i, hipStream_t s, bool deep) {
#define CLFA_FUSED(TVF, DP)                                                                                          \
  hipLaunchKernelGGL((k_pconv_fused<LOGB, TVF, DP>), dim3(g.channels), dim3(256), 0, s, in1, in2, ringA, ringB, tail, out, \
                     frame1, frame2, wp, g.nparts, half, w2f, w2i)
  if (in2 && deep) CLFA_FUSED(true, true);
  else if (in2) CLFA_FUSED(true, false);
  else if (deep) CLFA_FUSED(false, true);
  else CLFA_FUSED(false, false);
#undef CLFA_FUSED
  return hipGetLastError();
}

hipError_t launch_pconv_fused(const PconvGeom &g, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                              float *tail, float *out, int frame1, int frame2, int wp, const cpx *half,
                              const cpx *w2f, const cpx *w2i, hipStream_t s, bool deep) {
  return dispatch_logb<9, 12>(g.logb, [&](auto L) {
    return launch_fused_one<decltype(L)::value>(g, in1, in2, ringA, ringB, tail, out, frame1, frame2, wp, half, w2f, w2i, s, deep);
  });
}

}  // namespace clfa
