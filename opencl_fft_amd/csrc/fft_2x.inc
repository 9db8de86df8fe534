// fft_2x.inc (part of the translation unit fft_kernels.hip) — transforms as TWO runs of the next smaller
// single-workgroup machinery plus a radix-2 step in registers, for gfx950 (MI355X): one HBM pass where the four-step kernel (plus the stand-alone pack kernel) took two.
//   k_rfft_2x<14>     packed real size 65536 on two 16384-point runs, k_rfft_2x_s<13>: real size 32768 on two 8192-point runs;
//   k_cfft_2x<13>     complex n = 16384 on two 8192-point runs.
#include "fft_xfer.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// packed real size 65536 (n = 32768 complex): two runs of the 16384-point LDS machinery per transform
// ---------------------------------------------------------------------------------
// n = 2 M, M = 16384: the even and odd complex samples z[2j], z[2j+1] — one 16-byte access per lane — go
// through the 16384-point pass chain one after the other (same 1024 lanes, same exchange buffer); the
// radix-2 step that joins them and the reference's pair map (cl_fft.cpp:178-205) meet in registers
// (fft_device.hpp, rfft2x_fwd_slot / rfft2x_inv_slot): one HBM pass, where the four-step kernel plus the
// stand-alone pack kernel took two.  The inverse runs the transposed network.
// Byte offsets (vector part, scalar part) of the four packed bins of slot (u, q) of lane t (rfft2x_pos(i, which),
// i = pair_index<14, 4>(t, u, q)): every one of them is C + j or C - j, j = t + 1024 u, so the lane part is one of TWO
// VGPRs (t * 8, (1024 - t) * 8) and the rest scalar.  With flat addresses each of the 32 accesses of a lane carried
// its own 64-bit address pair — hipcc then issued the inverse kernel's loads four at a time, each group behind a
// full s_waitcnt vmcnt(0): eight exposed memory latencies per transform.  The u = 0 slots carry lane 0's exceptions
// (pair_index, rfft2x_pos) in the vector part.
struct R15Off {
  int v, s;
};
// LOGC: the sub-transforms' length (14: real size 65536, T = 1024 lanes, four pairs per u; 13: real size 32768,
// T = 512 lanes, two pairs per u — pair_index<13, 4>: q = 0 -> i = j, 1 -> 4096 - j)
template <int LOGC, int LOGE> __device__ __forceinline__ R15Off rfft2x_off(const XferBuf &b, int t, int u, int q, int which) {
  constexpr int LOGR = pass_rem_logr(LOGC, LOGE), R = 1 << LOGR, M = 1 << LOGC, NB = M >> LOGR, T = M >> LOGE;
  static_assert(R == 2 || R == 4, "two or four pairs per u");
  if (u == 0) return R15Off{rfft2x_pos<LOGC>(pair_index<LOGC, LOGE>(t, 0, q), which) * 8, 0};
  // i = +j + ci or -j + ci;  position = which 0: i, 1: 2M - i, 2: M - i, 3: M + i
  const bool ineg = q >= R / 2;
  const int ci = R == 4 ? (q == 0 ? 0 : q == 1 ? NB : q == 2 ? 2 * NB : NB) : (q == 0 ? 0 : NB);
  const bool neg = (which == 1 || which == 2) ? !ineg : ineg;                       // sign of j in the position
  const int c = which == 0 ? ci : which == 1 ? 2 * M - ci : which == 2 ? M - ci : M + ci;   // position = c +- j
  return neg ? R15Off{b.vd, (c - u * T - T) * 8} : R15Off{b.va, (c + u * T) * 8};
}
// k_rfft_2x<14>: real size 65536, one 1024-lane workgroup per CU (formerly k_rfft_lds15);
// k_rfft_2x<13>: real size 32768, 512 lanes and 71 KiB of LDS — TWO workgroups per CU, which overlap each other's
// memory phases (k_fft_lds<14> with its pair maps puts one 1024-lane workgroup on a CU)
// (the template also instantiates as <11, true | false, ., 3> — real size 8192 on two 2048-point runs with eight points per
// lane, the half table in LDS; measured slower than k_fft_lds<12> in round 4 and without a launcher since)
template <int LOGC, bool FWD, bool SCALE, int LOGE = 4>
__device__ __forceinline__ void rfft_2x_body(cpx *__restrict__ data, const cpx *__restrict__ tab_g, const cpx *__restrict__ w2_g,
                                             long batch, long out_off) {
  constexpr int LOGN = LOGC, E = 1 << LOGE, M = 1 << LOGC, T = M / E, R = 1 << pass_rem_logr(LOGC, LOGE);
  constexpr bool LANE = kLdsTwoLevel(LOGC);   // lane-addressed tables (8192 / 16384 points) or the half table W_M^k
  constexpr int NTAB = LANE ? kLaneLds : M / 2;
  __shared__ cpx s_tab[NTAB];
  __shared__ cpx s_x[lds_padded_size(M)];
  const int tid = threadIdx.x;
  for (int i = tid; i < (LANE ? kLane13Lds : M / 2); i += T) s_tab[LANE ? lane_lds_index(i) : i] = tab_g[i];
  // lane constants kept across the batch loop: W_M^tid and W_4M^tid only (4 VGPRs; the kernel runs under the 128-VGPR
  // cap) — W_M^(2 tid), ^(3 tid) and W_2M^tid are their products
  const cpx wl0 = LANE ? tab_g[kLane13Lds + tid] : mk(1.f, 0.f);
  const cpx h0 = w2_g[tid];   // W_4M^tid (the plan's sign)
  cpx *xb = s_x;
  __syncthreads();
#pragma unroll 1
  for (long b = blockIdx.x; b < batch; b += gridDim.x) {
    int t = tid;   // opaque per iteration: LDS / global offsets are recomputed, not kept live across the loop
    asm volatile("" : "+v"(t));
    const auto tab = [&]() {
      if constexpr (LOGC == 14) {
        const cpx wl1 = cmul(wl0, wl0);
        return LaneTab14{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl0, wl1, cmul(wl0, wl1)};
      } else if constexpr (LOGC == 13) {
        return LaneTab13{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl0};
      } else {
        return static_cast<const cpx *>(s_tab);
      }
    }();
    const cpx g0 = cmul(h0, h0);   // W_2M^tid
    cpx *x = data + b * (long)(2 * M);
    cpx *xs = x + out_off;   // where the results go (out_off = 0: in place)
    const XferBuf xo{__builtin_amdgcn_make_buffer_rsrc(x, 0, 0x7fffffff, 0x00020000), t * 8, (T - t) * 8};
    cpx va[E], vb[E];
    if constexpr (FWD) {
#pragma unroll
      for (int e = 0; e < E; e++) {
        const f4v q = ld_nt16(x + 2 * (t + T * e));
        va[e] = mk(q.x, q.y);
        vb[e] = mk(q.z, q.w);
      }
      pass_compute<LOGN, LOGE, 0, true>(va, t, tab);
      // staggered: one chain's LDS transfers under the other's passes.  (The middle passes on permuted lanes — fft_wg.hpp,
      // wg_passes_pair_sigma, conflict-free gathers — measured nothing here: size 32768 +1.4 %, 65536 -0.5 %,
      // profiles/ab_lane_sigma_r05.txt; the complex kernel below keeps them for its -0.7 %.)
      wg_passes_pair<LOGN, LOGE, 0, true>(va, vb, t, tab, xb);
      if constexpr (SCALE) {
        constexpr float inv = 1.0f / (float)(2 * M);
#pragma unroll
        for (int e = 0; e < E; e++) {
          va[e] = cscale(va[e], inv);
          vb[e] = cscale(vb[e], inv);
        }
      }
      cpx ai[E / 2], aj[E / 2], bi[E / 2], bj[E / 2];
      pairs_visit<LOGN, LOGE>(va, t, [&](int k, int, cpx ci, cpx cj) {
        ai[k] = ci;
        aj[k] = cj;
      });
      pairs_visit<LOGN, LOGE>(vb, t, [&](int k, int, cpx ci, cpx cj) {
        bi[k] = ci;
        bj[k] = cj;
      });
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        // (flat addresses for the forward kernel's stores: buffer-addressed they were measured 2 % slower)
        rfft2x_fwd_slot<LOGC>(t, k / R, k % R, pair_index<LOGN, LOGE>(t, k / R, k % R), ai[k], aj[k], bi[k], bj[k], g0, h0,
                              [&](int pos, cpx v) { st_nt(xs + pos, v); });
        __builtin_amdgcn_sched_barrier(0);   // slot by slot: hoisted, the eight slots' twiddles spill
      }
    } else {
      cpx oa[E / 2], pa[E / 2], ob[E / 2], pb[E / 2];
      cpx raw[2 * E];   // all 32 loads of the lane are in flight before the first slot is computed
#pragma unroll
      for (int k = 0; k < E / 2; k++)
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const R15Off o = rfft2x_off<LOGC, LOGE>(xo, t, k / R, k % R, w);
          raw[4 * k + w] = ld_buf<false>(xo, o.v, o.s);
        }
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        const int i = pair_index<LOGN, LOGE>(t, k / R, k % R);
        rfft2x_inv_slot<LOGC>(t, k / R, k % R, i, g0, h0, raw[4 * k], raw[4 * k + 1], raw[4 * k + 2], raw[4 * k + 3], oa[k],
                              pa[k], ob[k], pb[k]);
      }
      constexpr int L1 = pass_last_logns(LOGN, LOGE) - LOGE;
      // staggered (fft_wg.hpp, wg_passes_dif_pair): one chain's scatter drains under the other's butterflies
      pass_first_paired<LOGN, LOGE, false>(va, t, oa, pa, tab);
      __syncthreads();
      pass_first_paired_scatter<LOGN, LOGE>(va, t, xb);
      pass_first_paired<LOGN, LOGE, false>(vb, t, ob, pb, tab);
      __syncthreads();
      dif_gather_padded<LOGN, LOGE, L1>(va, t, xb);
      __syncthreads();
      pass_first_paired_scatter<LOGN, LOGE>(vb, t, xb);
      dif_compute<LOGN, LOGE, L1, false>(va, t, tab);
      __syncthreads();
      dif_gather_padded<LOGN, LOGE, L1>(vb, t, xb);
      wg_passes_dif_pair<LOGN, LOGE, L1, false>(va, vb, t, tab, xb);
#pragma unroll
      for (int e = 0; e < E; e++) st_nt16(xs + 2 * (t + T * e), f4v{va[e].x, va[e].y, vb[e].x, vb[e].y});
    }
  }
}

template <int LOGC, bool FWD, bool SCALE, int LOGE = 4>
__global__ __launch_bounds__((1 << LOGC) >> LOGE, 4) void k_rfft_2x(cpx *__restrict__ data, const cpx *__restrict__ tab_g,
                                                                    const cpx *__restrict__ w2_g, long batch, long out_off) {
  rfft_2x_body<LOGC, FWD, SCALE, LOGE>(data, tab_g, w2_g, batch, out_off);
}
// ... with single LDS accesses (real size 32768)
template <int LOGC, bool FWD, bool SCALE, int LOGE = 4>
__global__ __launch_bounds__((1 << LOGC) >> LOGE, 4) CLFA_DS_SINGLE_FN void k_rfft_2x_s(cpx *__restrict__ data, const cpx *__restrict__ tab_g,
                                                                    const cpx *__restrict__ w2_g, long batch, long out_off) {
  rfft_2x_body<LOGC, FWD, SCALE, LOGE>(data, tab_g, w2_g, batch, out_off);
}

hipError_t launch_rfft_lds15(bool fwd, cpx *data, const FftTables &t, long batch, const DeviceInfo &di, hipStream_t s,
                             long out_off) {
  if (batch <= 0) return hipSuccess;
  const int grid = (int)(batch < di.num_cus ? batch : di.num_cus);   // one 1024-lane workgroup per CU
  if (fwd) hipLaunchKernelGGL((k_rfft_2x<14, true, true>), dim3(grid), dim3(1024), 0, s, data, t.half, t.w2, batch, out_off);
  else hipLaunchKernelGGL((k_rfft_2x<14, false, false>), dim3(grid), dim3(1024), 0, s, data, t.half, t.w2, batch, out_off);
  return hipGetLastError();
}
// real size 32768: t.half = the n = 8192 lane tables (kLane13Size), t.w2 = the plan's r2c table (16384 entries)
hipError_t launch_rfft_2x13(bool fwd, cpx *data, const FftTables &t, long batch, const DeviceInfo &di, hipStream_t s,
                            long out_off) {
  if (batch <= 0) return hipSuccess;
  const long cap = 2L * di.num_cus;   // two 512-lane workgroups per CU
  const int grid = (int)(batch < cap ? batch : cap);
  if (fwd) hipLaunchKernelGGL((k_rfft_2x_s<13, true, true>), dim3(grid), dim3(512), 0, s, data, t.half, t.w2, batch, out_off);
  else hipLaunchKernelGGL((k_rfft_2x_s<13, false, false>), dim3(grid), dim3(512), 0, s, data, t.half, t.w2, batch, out_off);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// complex n = 16384 as TWO 8192-point runs (decimation in time: even and odd samples — one 16-byte load per lane
// brings both) through the n = 8192 machinery, staggered through one exchange buffer (wg_passes_pair), and a radix-2
// step in registers: Z[i] = A[i] + W_16384^i B[i], Z[i + 8192] = A[i] - W_16384^i B[i].  512 lanes, 71 KiB of LDS:
// two workgroups share a CU and overlap each other's memory phases — the whole-transform-in-LDS forms (k_fft_lds<14>
// with 1024 lanes, the persistent four-step kernel) put ONE workgroup on a CU, and its load, pass and store phases
// follow one another.  W_16384^(tid + 512 e) = (lane constant W_16384^tid) x (compile-time W_32^e).  (k_cfft_2x<13>.)
// ---------------------------------------------------------------------------------
// (LOGC = 14: n = 32768 on two 16384-point runs, one 1024-lane workgroup per CU — measured against the persistent
// four-step kernel before choosing, see DESIGN.md)
template <int LOGC, bool FWD, bool SCALE>
__global__ __launch_bounds__((1 << LOGC) / 16, 4) void k_cfft_2x(cpx *__restrict__ data, const cpx *__restrict__ tab_g,
                                                                 long batch, long out_off) {
  using G = LdsGeom<LOGC>;
  constexpr int LOGN = LOGC, LOGE = 4, E = 16, M = 1 << LOGC, T = M / E;
  __shared__ cpx s_tab[kLaneLds];
  __shared__ cpx s_x[G::PADN];
  const int tid = threadIdx.x;
  for (int i = tid; i < kLane13Lds; i += T) s_tab[lane_lds_index(i)] = tab_g[i];
  const cpx wl0 = tab_g[kLane13Lds + tid];                                     // W_M^tid
  const cpx h0 = tab_g[(LOGC == 14 ? kLane14Size : kLane13Size) + tid];        // W_2M^tid (forward sign, like every table)
  cpx *xb = s_x;
  __syncthreads();
#pragma unroll 1
  for (long b = blockIdx.x; b < batch; b += gridDim.x) {
    int t = tid;   // opaque per iteration: LDS / global offsets are recomputed, not kept live across the loop
    asm volatile("" : "+v"(t));
    const auto tab_of = [&](int t) {
      if constexpr (LOGC == 14) {
        const cpx wl1 = cmul(wl0, wl0);
        return LaneTab14{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl0, wl1, cmul(wl0, wl1)};
      } else {
        return LaneTab13{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl0};
      }
    };
    const auto tab = tab_of(t);
    cpx *x = data + b * (long)(2 * M);
    cpx va[E], vb[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const f4v q = ld_nt16(x + 2 * (t + T * e));
      va[e] = mk(q.x, q.y);
      vb[e] = mk(q.z, q.w);
    }
    pass_compute<LOGN, LOGE, 0, FWD>(va, t, tab);
    wg_passes_pair_sigma<LOGN, LOGE, 0, FWD, false>(va, vb, t, lane_sigma(t), tab, tab_of(lane_sigma(t)), xb);
    // radix-2 step: position i = t + T e, W_2M^i = W_2M^t W_32^e
    constexpr float c32[16] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
                               0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f,
                               0.19509032201612826785f, 0.0f, -0.19509032201612826785f, -0.38268343236508977173f,
                               -0.55557023301960222474f, -0.70710678118654752440f, -0.83146961230254523708f,
                               -0.92387953251128675613f, -0.98078528040323044913f};
    constexpr float s32[16] = {0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f,
                               0.70710678118654752440f, 0.83146961230254523708f, 0.92387953251128675613f,
                               0.98078528040323044913f, 1.0f, 0.98078528040323044913f, 0.92387953251128675613f,
                               0.83146961230254523708f, 0.70710678118654752440f, 0.55557023301960222474f,
                               0.38268343236508977173f, 0.19509032201612826785f};
    constexpr float inv = SCALE ? 1.0f / (float)(2 * M) : 1.0f;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const cpx w = e == 0 ? h0 : ctw<true>(h0, c32[e], s32[e]);   // W_2M^(t + T e), forward sign
      const cpx p = cmulc<!FWD>(vb[e], w);
      cpx o0 = cadd(va[e], p), o1 = csub(va[e], p);
      if constexpr (SCALE) {
        o0 = cscale(o0, inv);
        o1 = cscale(o1, inv);
      }
      st_nt(x + out_off + t + T * e, o0);
      st_nt(x + out_off + M + t + T * e, o1);
      __builtin_amdgcn_sched_barrier(0);   // element by element: hoisted, the sixteen twiddles spill
    }
  }
}

template <int LOGC>
static hipError_t launch_cfft_2x_n(bool fwd, bool scale, cpx *data, const FftTables &t, long batch, const DeviceInfo &di,
                                   hipStream_t s, long out_off) {
  if (batch <= 0) return hipSuccess;
  constexpr int T = (1 << LOGC) / 16;
  const long cap = (LOGC == 13 ? 2L : 1L) * di.num_cus;   // two 512-lane workgroups per CU, or one of 1024 lanes
  const int grid = (int)(batch < cap ? batch : cap);
  if (fwd && scale) hipLaunchKernelGGL((k_cfft_2x<LOGC, true, true>), dim3(grid), dim3(T), 0, s, data, t.half, batch, out_off);
  else if (fwd) hipLaunchKernelGGL((k_cfft_2x<LOGC, true, false>), dim3(grid), dim3(T), 0, s, data, t.half, batch, out_off);
  else if (!scale) hipLaunchKernelGGL((k_cfft_2x<LOGC, false, false>), dim3(grid), dim3(T), 0, s, data, t.half, batch, out_off);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_cfft_2x13(bool fwd, bool scale, cpx *data, const FftTables &t, long batch, const DeviceInfo &di,
                            hipStream_t s, long out_off) {
  return launch_cfft_2x_n<13>(fwd, scale, data, t, batch, di, s, out_off);
}

}  // namespace clfa
