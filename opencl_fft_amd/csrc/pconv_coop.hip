// pconv_coop.hip — one block of the partitioned convolution in ONE launch for a FEW channels (k_pconv_coop): workgroups
// split the bins and the partitions and meet through the hand-over of handover.hpp; restates cl_conv.cpp:393-458 /
// 460-548 and cl_conv_kernels.h:46-124.  The launch chain it replaces is in pconv_chain.hip.
#include <cstdlib>

#include "handover.hpp"
#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// cooperative block: ONE launch per block for a FEW channels — the single-instance call that the reference's
// opcodes and its own harness make (cl_conv.cpp:393-458 / 460-548 once per ksmps block; csound/tests.py:22-29).
// With one channel the chain above is four or five dependent launches of 5 us each.  Here S workgroups per
// channel split the BIN axis of the multiply-accumulate (no partial sums to add up: a bin's whole sum over the
// partitions is formed inside one workgroup, rows of lanes walking the partitions in parallel and meeting in
// LDS in fixed order), every workgroup transforms the new input block itself (a few microseconds of redundant
// arithmetic instead of a grid-wide hand-over of the new frame; workgroup 0 also files it in the ring for the
// blocks to come), and the only inter-workgroup step is the hand-over of the finished accumulator slices —
// bins x 8 bytes per channel in all — to whichever workgroup arrives LAST at the channel's counter: it runs the
// inverse chain.  No workgroup ever waits for another one: nothing spins.
// The hand-over itself (protocol and primitives): handover.hpp.
// ---------------------------------------------------------------------------------
template <int LOGB, bool TV>
__global__ __launch_bounds__(LdsGeom<LOGB>::WG) void k_pconv_coop(const float *__restrict__ in1, const float *__restrict__ in2,
                                                    cpx *__restrict__ ringA, cpx *__restrict__ ringB,
                                                    float *__restrict__ tail, float *__restrict__ out, int frame1,
                                                    int frame2, int wp, int nparts, const cpx *__restrict__ tab_g,
                                                    const cpx *__restrict__ w2f_g, const cpx *__restrict__ w2i_g,
                                                    cpx *__restrict__ xacc, unsigned *__restrict__ counters, int logs,
                                                    int sparts, int acquire) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T, HB = N / 2;   // N = bins; T = N/16 lanes run the FFTs
  constexpr int WG = G::WG;                                  // 256 lanes; 512 for partitions of 8192 samples
  constexpr int kSliceMax = 512;                             // bins per workgroup (host: logs >= LOGB - 9)
  static_assert(LOGB >= 5 && LOGB <= 13 && T <= WG, "bins 32..8192: slices of 32 bins, 16 points per lane in the transforms");
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_x[G::PADN];
  __shared__ cpx s_fa[kSliceMax];            // this workgroup's slice of the new input block's packed spectrum (frame1 of ring A)
  __shared__ cpx s_fb[TV ? kSliceMax : 1];   // ... of the second input's (frame2 of ring B)
  __shared__ cpx2 s_red[WG];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  // workgroup = (slice sl of the bins, segment ps of the partition axis)
  const int ch = blockIdx.y, S = 1 << logs, sl = blockIdx.x & (S - 1), ps = blockIdx.x >> logs;
  for (int i = tid; i < N / 2; i += WG) s_tab[i] = tab_g[i];
  __syncthreads();

  // ---- this workgroup's part of the multiply-accumulate: slice = N >> logs bins = IW 16-byte items; lane = item li of
  // partition row pr; rows walk p = p_begin + pr, + NR, ...  The first loads of the walk (and the ring operands of the
  // new frames' terms) are issued HERE, before the forward transforms: they need nothing from them, and their memory
  // latency then runs under 1-2 us of butterflies instead of after them.
  const int iw = HB >> logs, nr = WG / iw;
  const int li = tid % iw, pr = tid / iw;
  const int item = sl * iw + li;                       // 16-byte item (bins 2 item, 2 item + 1) of the frame
  const cpx2 *ra = reinterpret_cast<const cpx2 *>(ringA + (long)ch * nparts * N) + item;
  const cpx2 *rb = reinterpret_cast<const cpx2 *>(ringB + (long)ch * nparts * N) + item;
  const int p1 = nparts - 1;                           // (wp + p1) % nparts == frame1: wp = frame1 + 1
  const int chunk = (nparts + sparts - 1) / sparts;    // this workgroup's partitions [p_begin, p_end)
  const int p_begin = ps * chunk, p_end = p_begin + chunk < nparts ? p_begin + chunk : nparts;
  constexpr int UNR = 4;
  cpx2 av0[UNR], bv0[UNR];
  bool live0[UNR];
#pragma unroll
  for (int u = 0; u < UNR; u++) {   // (clamped, not predicated: straight-line loads)
    const int pp = p_begin + pr + u * nr;
    const bool ok = pp < p_end;
    const int pc = ok ? pp : p_end - 1;
    int fr = wp + pc;
    fr = fr < nparts ? fr : fr - nparts;
    av0[u] = ld_nt(ra + (long)fr * HB);
    bv0[u] = ld_nt(rb + (long)pc * HB);
    live0[u] = ok && pc != p1 && !(TV && pc == frame2);
  }
  const cpx2 b_p1 = rb[(long)p1 * HB];                 // ring operand of the new A frame's term
  int fr2 = wp + (TV ? frame2 : 0);
  fr2 = fr2 < nparts ? fr2 : fr2 - nparts;
  const cpx2 a_f2 = ra[(long)fr2 * HB];                // ... of the new B frame's term (time-varying blocks)
  // ... and so are the pack / unpack twiddles of the lane's bins and the overlap-add tail: every global load that does
  // not depend on this launch's results leaves at the top of the kernel — a block is a chain of dependent steps of a
  // microsecond each, and every load left in the middle of it is one more
  constexpr int NI = (N / 2 + WG - 1) / WG;
  cpx w2f_r[NI], w2i_r[NI];
#pragma unroll
  for (int q = 0; q < NI; q++) {
    const int i = tid + q * WG;
    w2f_r[q] = w2f_g[i < N / 2 ? i : 0];
    w2i_r[q] = w2i_g[i < N / 2 ? i : 0];
  }
  cpx tail_r[E / 2];
  {
    const cpx *tl = reinterpret_cast<const cpx *>(tail + (long)ch * N);
#pragma unroll
    for (int e = 0; e < E / 2; e++) tail_r[e] = tl[(tid < T ? tid : 0) + T * e];
  }

  // ---- forward chain(s) in every workgroup: reference reorder + fft + r2c (cl_conv.cpp:399-419 / 465-513) ----
  // Time-varying blocks transform both inputs AT ONCE where the lanes allow it (2 T <= 256): lanes [0, T) take in1,
  // lanes [T, 2 T) in2, each group with its own exchange buffer — one pass chain's worth of barriers, not two.
  constexpr bool DUAL = TV && 2 * T <= WG;
  __shared__ cpx s_x2[DUAL ? G::PADN : 1];
  auto forward = [&](const float *inA, const float *inB, bool dual) {
    // inB / ring B only when dual; otherwise one input (inA) by lanes [0, T)
    const int grp = dual ? tid / T : 0, tt = dual ? tid % T : tid;
    const bool work = dual ? tid < 2 * T : tid < T;
    cpx *sx = (DUAL && grp == 1) ? s_x2 : s_x;
    cpx v[E];
    if (work) {
      const cpx *src = reinterpret_cast<const cpx *>((grp == 1 ? inB : inA) + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int p = tt + T * e;
        v[e] = p < N / 2 ? src[p] : mk(0.f, 0.f);
      }
      pass_compute<LOGB, G::LOGE, 0, true>(v, tt, s_tab);
    }
    // (LOGB > 4 always: a second pass of radix 2^min(4, LOGB - 4), a third one above 256 bins)
    __syncthreads();
    if (work) pass_scatter<LOGB, G::LOGE, 0>(v, tt, [&](int p, cpx val) { sx[lds_pad(p)] = val; });
    __syncthreads();
    if (work) {
      pass_gather<LOGB, G::LOGE>(v, tt, [&](int p) { return sx[lds_pad(p)]; });
      pass_compute<LOGB, G::LOGE, 4, true>(v, tt, s_tab);
    }
    if constexpr (LOGB > 8) {
      __syncthreads();
      if (work) pass_scatter<LOGB, G::LOGE, 4>(v, tt, [&](int p, cpx val) { sx[lds_pad(p)] = val; });
      __syncthreads();
      if (work) {
        pass_gather<LOGB, G::LOGE>(v, tt, [&](int p) { return sx[lds_pad(p)]; });
        pass_compute<LOGB, G::LOGE, 8, true>(v, tt, s_tab);
      }
    }
    if constexpr (LOGB > 12) {
      __syncthreads();
      if (work) pass_scatter<LOGB, G::LOGE, 8>(v, tt, [&](int p, cpx val) { sx[lds_pad(p)] = val; });
      __syncthreads();
      if (work) {
        pass_gather<LOGB, G::LOGE>(v, tt, [&](int p) { return sx[lds_pad(p)]; });
        pass_compute<LOGB, G::LOGE, 12, true>(v, tt, s_tab);
      }
    }
    __syncthreads();
    if (work) {
#pragma unroll
      for (int e = 0; e < E; e++) sx[lds_pad(tt + T * e)] = v[e];
    }
    __syncthreads();
  };
  // packed spectrum (reference r2c) of the transform left in `sx` -> sf (LDS) and, by workgroup 0, the ring frame
  const int bw = N >> logs, b0 = sl * bw;   // this workgroup's bins [b0, b0 + bw)
  auto pack = [&](const cpx *sx, cpx *ring, int frame, cpx *sf) {
    cpx *x = ring + ((long)ch * nparts + frame) * N;
#pragma unroll
    for (int q = 0; q < NI; q++) {
      const int i = tid + q * WG;
      if (i >= N / 2) break;
      const int j = i == 0 ? N / 2 : N - i;
      const cpx ci = sx[lds_pad(i)], cj = sx[lds_pad(j)];
      cpx oi, oj;
      r2c_pack_pair(ci, cj, w2f_r[q], i == 0, oi, oj);
      if (i >= b0 && i < b0 + bw) sf[i - b0] = oi;
      if (j >= b0 && j < b0 + bw) sf[j - b0] = oj;
      if (blockIdx.x == 0) {   // filed in the ring for the blocks to come; nobody reads it from there in this launch
        x[i] = oi;
        x[j] = oj;
      }
    }
  };
  if constexpr (DUAL) {
    forward(in1, in2, true);
    pack(s_x, ringA, frame1, s_fa);
    pack(s_x2, ringB, frame2, s_fb);
    __syncthreads();
  } else {
    forward(in1, nullptr, false);
    pack(s_x, ringA, frame1, s_fa);
    __syncthreads();
    if constexpr (TV) {
      forward(in2, nullptr, false);
      pack(s_x, ringB, frame2, s_fb);
      __syncthreads();
    }
  }

  // ---- MAC over all partitions for this workgroup's slice of the bins (reference convol, cl_conv_kernels.h:102-118)
  {
    const cpx2 *a = ra, *b = rb;
    const bool dc = item == 0;                           // packed DC / Nyquist bin: (re*re, im*im)
    cpx s0 = mk(0.f, 0.f), s1 = mk(0.f, 0.f);
    auto term = [&](const cpx2 &av, const cpx2 &bv, bool live) {
      cpx pa = cmul_plain(av.a, bv.a);
      pa = mk(dc ? av.a.x * bv.a.x : pa.x, dc ? av.a.y * bv.a.y : pa.y);
      const cpx pb = cmul_plain(av.b, bv.b);
      s0 = cadd(s0, mk(live ? pa.x : 0.f, live ? pa.y : 0.f));
      s1 = cadd(s1, mk(live ? pb.x : 0.f, live ? pb.y : 0.f));
    };
    // the frames written by THIS launch (frame1 of A; frame2 of B) are taken from LDS below: in the loop their
    // (stale) ring contents are read like any other frame and dropped by a select — no branch in the stream
#pragma unroll
    for (int u = 0; u < UNR; u++) term(av0[u], bv0[u], live0[u]);   // the batch fetched before the transforms
    int p = p_begin + pr + UNR * nr;
    for (; p + (UNR - 1) * nr < p_end; p += UNR * nr) {
      cpx2 av[UNR], bv[UNR];
      bool live[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) {
        const int pp = p + u * nr;
        int fr = wp + pp;
        fr = fr < nparts ? fr : fr - nparts;
        av[u] = ld_nt(a + (long)fr * HB);
        bv[u] = ld_nt(b + (long)pp * HB);
        live[u] = pp != p1 && !(TV && pp == frame2);
      }
#pragma unroll
      for (int u = 0; u < UNR; u++) term(av[u], bv[u], live[u]);
    }
    for (; p < p_end; p += nr) {
      int fr = wp + p;
      fr = fr < nparts ? fr : fr - nparts;
      term(ld_nt(a + (long)fr * HB), ld_nt(b + (long)p * HB), p != p1 && !(TV && p == frame2));
    }
    // the terms of the new frames, by the row that owns their partition
    const cpx2 *fa = reinterpret_cast<const cpx2 *>(s_fa) + li;
    if (p1 >= p_begin && p1 < p_end && pr == (p1 - p_begin) % nr) {
      cpx2 bv;
      if (TV && p1 == frame2) bv = reinterpret_cast<const cpx2 *>(s_fb)[li];
      else bv = b_p1;
      term(*fa, bv, true);
    }
    if constexpr (TV) {
      if (frame2 != p1 && frame2 >= p_begin && frame2 < p_end && pr == (frame2 - p_begin) % nr) {
        term(a_f2, reinterpret_cast<const cpx2 *>(s_fb)[li], true);
      }
    }
    cpx2 mine;
    mine.a = s0;
    mine.b = s1;
    s_red[tid] = mine;
    __syncthreads();
    if (pr == 0) {   // rows summed in ascending order: deterministic
      cpx t0 = s_red[li].a, t1 = s_red[li].b;
      for (int r = 1; r < nr; r++) {
        t0 = cadd(t0, s_red[r * iw + li].a);
        t1 = cadd(t1, s_red[r * iw + li].b);
      }
      cpx *dst = xacc + ((long)ch * sparts + ps) * N + 2 * item;
      st_agent(dst, t0);
      st_agent(dst + 1, t1);
    }
  }
  // ---- hand-over: the last workgroup to arrive at the channel's counter owns the inverse chain
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const unsigned old = handover_arrive(counters + ch);
    s_last = old == (unsigned)(S * sparts - 1);
    if (s_last) {
      __hip_atomic_store(counters + ch, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next block's launch
      handover_acquire(acquire);
    }
  }
  __syncthreads();
  if (!s_last) return;

  // ---- inverse chain: c2r + inverse FFT + overlap-add (cl_conv_kernels.h:87-100, 120-124) -------------
  const cpx *xa = xacc + (long)ch * sparts * N;
  auto xsum = [&](int i) {   // the segments' partial sums in ascending order
    cpx sum = ld_agent(xa + i);
    for (int k = 1; k < sparts; k++) sum = cadd(sum, ld_agent(xa + (long)k * N + i));
    return sum;
  };
#pragma unroll
  for (int q = 0; q < NI; q++) {
    const int i = tid + q * WG;
    if (i >= N / 2) break;
    if (i == 0) {
      const cpx c0 = xsum(0);
      s_x[0] = mk(c0.x + c0.y, c0.x - c0.y);
      s_x[lds_pad(N / 2)] = xsum(N / 2);
    } else {
      cpx oi, oj;
      c2r_pair(xsum(i), xsum(N - i), w2i_r[q], oi, oj);
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
    if constexpr (LOGB > 12) {
      __syncthreads();
      if (tid < T) pass_scatter<LOGB, G::LOGE, 8>(v, tid, [&](int p, cpx val) { s_x[lds_pad(p)] = val; });
      __syncthreads();
      if (tid < T) {
        pass_gather<LOGB, G::LOGE>(v, tid, [&](int p) { return s_x[lds_pad(p)]; });
        pass_compute<LOGB, G::LOGE, 12, false>(v, tid, s_tab);
      }
    }
    if (tid < T) {
      constexpr float inv = 1.0f / (float)N;
      cpx *o = reinterpret_cast<cpx *>(out + (long)ch * N);
      cpx *tl = reinterpret_cast<cpx *>(tail + (long)ch * N);
#pragma unroll
      for (int e = 0; e < E / 2; e++) {
        const int p = tid + T * e;
        const cpx old = tail_r[e];
        o[p] = mk((v[e].x + old.x) * inv, (v[e].y + old.y) * inv);
        tl[p] = v[e + E / 2];
      }
    }
  }
}

// Shape of the cooperative block, or logs = -1 when it does not apply: bins 32..4096; slices of 32 bins (256-byte
// segments of a frame) unless the channels alone would overfill the chip; the partition axis cut into segments until
// a workgroup's share of the two rings is at most CLFA_PCONV_COOP_MAX_KB (tuning switch, read at plan creation; 0 switches the
// kernel off); filters that would need more than half the CUs that way stay with the launch chain above (the split
// MAC + tree sum), which puts the whole chip on the partition axis.
PconvCoop pconv_coop_plan(const PconvGeom &g, const DeviceInfo &di) {
  const char *cap_env = getenv("CLFA_PCONV_COOP_MAX_KB");   // read per plan, like every other tuning switch
  const long cap_kb = cap_env ? atol(cap_env) : 128L;
  PconvCoop c{-1, 1};
  // (partitions of 8192 samples were measured on this kernel with 512-lane workgroups: 27 us static, 36 us time-varying
  // against 29 us on the chain — a workgroup's own 8192-point transforms take 10 us each — so they stay on the chain)
  if (g.logb < 5 || g.logb > 12 || cap_kb <= 0) return c;
  int logs = g.logb - 5;                                  // 32 bins per workgroup
  const int logs_min = g.logb > 9 ? g.logb - 9 : 0;       // at most 256 16-byte items per workgroup (one per lane)
  while (logs > logs_min && ((long)g.channels << logs) > di.num_cus) logs--;
  if (((long)g.channels << logs) > 2L * di.num_cus) return c;
  const long share = 2L * g.nparts * (g.bins >> logs) * 8;   // bytes of the rings one bin slice streams
  long sparts = (share + cap_kb * 1024 - 1) / (cap_kb * 1024);
  // ... as far as HALF the CUs go: a block that needs the whole chip to stream its rings is faster on the chain
  // (measured, real-time ratio of one time-varying channel: M = 512, L = 2^21: 448 here against 482 on the chain,
  // L = 2^22: 384 / 401; M = 2048, L = 2^21: 1761 / 1804 — every workgroup repeats the forward transform, and
  // the last one adds up all the segments)
  const long wgs = (long)g.channels << logs;
  long room = (di.num_cus / 2) / wgs;
  if (room < 1) room = 1;
  if (sparts > g.nparts / 4) sparts = g.nparts / 4;          // segments of at least 4 partitions
  if (sparts < 1) sparts = 1;
  if (sparts > room) {
    // Many channels: their bin slices alone occupy half the chip or more, every workgroup streams its whole share
    // (up to 1 MiB) and nothing is cut or added up.  Measured at pts 1024 x 94 partitions, per block: 24 channels
    // 24.0 (chain) -> 15.5 us, 32: 24.1 -> 16.4, 64: 33.0 -> 24.0, 100: 41.4 -> 32.6, 128: 45.4 -> 40.4, 136: 55.9
    // -> 50.1; from 137 channels on k_pconv_fused takes over (144: 49.7 against 49.7 here, 256: 68.7 against 73.3).
    if (2 * wgs < di.num_cus || share > 1024L * 1024) return c;
    sparts = 1;
  }
  c.logs = logs;
  c.sparts = (int)sparts;
  return c;
}

template <int LOGB>
static hipError_t launch_coop_one(const PconvGeom &g, PconvCoop c, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                                  float *tail, float *out, int frame1, int frame2, int wp, const cpx *half, const cpx *w2f,
                                  const cpx *w2i, cpx *xacc, unsigned *counters, int num_cus, hipStream_t s) {
  const dim3 grid(c.sparts << c.logs, g.channels);
  const int acquire = (long)grid.x * grid.y > num_cus;   // more workgroups than CUs: see handover_acquire()
  if (in2)
    hipLaunchKernelGGL((k_pconv_coop<LOGB, true>), grid, dim3(LdsGeom<LOGB>::WG), 0, s, in1, in2, ringA, ringB, tail, out, frame1, frame2,
                       wp, g.nparts, half, w2f, w2i, xacc, counters, c.logs, c.sparts, acquire);
  else
    hipLaunchKernelGGL((k_pconv_coop<LOGB, false>), grid, dim3(LdsGeom<LOGB>::WG), 0, s, in1, in2, ringA, ringB, tail, out, frame1, frame2,
                       wp, g.nparts, half, w2f, w2i, xacc, counters, c.logs, c.sparts, acquire);
  return hipGetLastError();
}

hipError_t launch_pconv_coop(const PconvGeom &g, PconvCoop c, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                             float *tail, float *out, int frame1, int frame2, int wp, const cpx *half, const cpx *w2f,
                             const cpx *w2i, cpx *xacc, unsigned *counters, int num_cus, hipStream_t s) {
  return dispatch_logb<5, 12>(g.logb, [&](auto L) {
    return launch_coop_one<decltype(L)::value>(g, c, in1, in2, ringA, ringB, tail, out, frame1, frame2, wp, half, w2f, w2i, xacc, counters,
                                               num_cus, s);
  });
}

}  // namespace clfa
