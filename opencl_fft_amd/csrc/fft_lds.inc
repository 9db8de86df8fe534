// fft_lds.inc (part of the translation unit fft_kernels.hip) — batched 1-D FFTs that one workgroup holds:
// n <= 8192 (packed real size <= 16384), for gfx950 (MI355X).
//
// Replaces the reference's launch chain reorder + log2(N) x fft (+ conv/iconv)
// (cl_fft.cpp:24-41, 138-151, 178-205) by
//   k_fft_lds    one HBM pass: a transform (n <= 8192) lives in VGPRs + LDS of one
//                workgroup; r2c pack / c2r unpack fused (the two bins of a pair meet in
//                one lane's registers where the pass structure allows);
//   k_fft_small  n = 8 .. 64 (packed real: .. 256): the same passes behind workgroup-wide coalesced rows;
//   k_fft_tiny   n = 2 and 4, complex: a copy kernel with a butterfly in it.
#include "fft_xfer.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// single-workgroup LDS FFT
// ---------------------------------------------------------------------------------

// Global loads of one transform into registers, in the order the first stage wants them:
//   C2C / R2C : v[e] = x[t + T*e]                         (coalesced, T apart)
//   C2R       : v[2k] = x[i], v[2k+1] = x[N-i], i = t + T*k (the pairs of the reference's iconv);
//               pair 0 of lane 0 is (x[0], x[N/2])
// The packed real kernels of a whole workgroup address them through a buffer descriptor (fft_xfer.hpp, XferBuf)
// (measured, interleaved A/B against flat addressing: r2c + c2r of size 16384 0.213 -> 0.203-0.208 ms; the complex
// transforms, which have one ascending stream each way, lose 2 % at n = 8192 and stay as they were)
// (buffer addressing for the complex n = 8192 kernels was measured per direction as well: inverse 0.780 -> 0.835 ms,
// forward 0.789 -> 0.827 ms per 2 GiB — both lose, although the inverse instantiation carries a 20-byte spill on flat
// addresses)
template <int LOGN, int MODE, bool FWD = true>
constexpr bool kLdsBufAddr = LdsGeom<LOGN>::FPW == 1 && LOGN >= 12 && MODE != MODE_C2C;
// byte offsets (vector part, scalar part) of position i = pair_index(t, u, q) and of its partner N - i (N / 2 for
// i = 0) of a paired remainder pass (fft_device.hpp); the u = 0 pairs carry lane 0's exceptions in the vector part
template <int LOGN, int LOGE> struct PairOff {
  int vi, si, vj, sj;
};
template <int LOGN, int LOGE> __device__ __forceinline__ PairOff<LOGN, LOGE> pair_off(const XferBuf &b, int t, int u, int q) {
  constexpr int LOGR = pass_rem_logr(LOGN, LOGE), R = 1 << LOGR, T = 1 << (LOGN - LOGE), NB = 1 << (LOGN - LOGR), N = 1 << LOGN;
  PairOff<LOGN, LOGE> o;
  if (u == 0) {
    const int i = pair_index<LOGN, LOGE>(t, 0, q);
    o.vi = i * 8;
    o.vj = (i == 0 ? N / 2 : N - i) * 8;
    o.si = o.sj = 0;
  } else if (q < R / 2) {   // i = t + u T + NB q ascending, partner N - i descending
    o.vi = b.va;
    o.si = (u * T + NB * q) * 8;
    o.vj = b.vd;
    o.sj = (N - NB * q - u * T - T) * 8;
  } else {                  // i = NB (R - q) - (t + u T) descending, partner ascending
    o.vi = b.vd;
    o.si = (NB * (R - q) - u * T - T) * 8;
    o.vj = b.va;
    o.sj = (N - NB * (R - q) + u * T) * 8;
  }
  return o;
}

template <int LOGN, int MODE, bool FWD = true>
__device__ __forceinline__ void lds_fft_load(cpx (&v)[LdsGeom<LOGN>::E], const cpx *x, int t) {
  // No predicates on purpose: callers clamp the transform index instead.  Loads inside
  // exec-masked or even uniform branches make hipcc lose count of them and wait vmcnt(0) at the
  // join, i.e. for the prefetch it has just issued (seen in the ISA); straight-line loads get a
  // counted s_waitcnt vmcnt(N) and stay in flight behind the passes.
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T;
  if constexpr (kLdsBufAddr<LOGN, MODE, FWD>) {
    const XferBuf b = xfer_buf<LOGN>(x, t);
    constexpr bool NT = MODE == MODE_C2C;   // the packed real kernels load plain (fft_xfer.hpp, ld_buf)
    if constexpr (MODE == MODE_C2R) {
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        if constexpr (pair_ok(LOGN, G::LOGE)) {   // pairs in the order pass_first_paired wants them
          constexpr int R = 1 << pass_rem_logr(LOGN, G::LOGE);
          const auto o = pair_off<LOGN, G::LOGE>(b, t, k / R, k % R);
          v[2 * k] = ld_buf<NT>(b, o.vi, o.si);
          v[2 * k + 1] = ld_buf<NT>(b, o.vj, o.sj);
        } else {
          v[2 * k] = ld_buf<NT>(b, b.va, T * k * 8);
          // partner N - (t + T k); pair 0 of lane 0 is (x[0], x[N/2])
          if (k == 0) v[1] = ld_buf<NT>(b, t == 0 ? (N / 2) * 8 : (N - t) * 8, 0);
          else v[2 * k + 1] = ld_buf<NT>(b, b.vd, (N - T * k - T) * 8);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; e++) v[e] = ld_buf<NT>(b, b.va, T * e * 8);
    }
    return;
  }
  if constexpr (MODE == MODE_C2R) {
#pragma unroll
    for (int k = 0; k < E / 2; k++) {
      int i = t + T * k;
      if constexpr (pair_ok(LOGN, G::LOGE)) {   // pairs in the order pass_first_paired wants them
        constexpr int R = 1 << pass_rem_logr(LOGN, G::LOGE);
        i = pair_index<LOGN, G::LOGE>(t, k / R, k % R);
      }
      v[2 * k] = ld_nt(x + i);
      v[2 * k + 1] = ld_nt(x + (i == 0 ? N / 2 : N - i));
    }
  } else {
#pragma unroll
    for (int e = 0; e < E; e++) v[e] = ld_nt(x + t + T * e);
  }
}

template <int LOGN, bool FWD, int MODE, bool SCALE>
__device__ __forceinline__ void fft_lds_body(cpx *__restrict__ data, const cpx *__restrict__ tab_g, const cpx *__restrict__ w2_g,
                                             long batch, long out_off) {
  // out_off: results go to data + out_off (complex elements; 0 = in place, else a disjoint destination: clfa_fft_exec_dev_oop)
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, WG = G::WG, FPW = G::FPW;
  // twiddles in LDS: half table W_n^k (k < n/2); n = 8192: the lane-addressed tables of LaneTab13
  // (fft_device.hpp: 1280 entries, which keeps the block at 78 KiB so that two workgroups share a CU)
  constexpr bool TWO = kLdsTwoLevel(LOGN);
  constexpr int NTAB = TWO ? kLaneLds : G::HALF;
  __shared__ cpx s_tab[NTAB];
  __shared__ cpx s_x[FPW * G::PADN];
  // packed real size 8192 (n = 4096): the twiddles of the pass that starts at 16 points from a 16 x 16 table (HalfRowTab)
  constexpr bool ROW16 = !TWO && LOGN == 12 && MODE != MODE_C2C;
  __shared__ cpx s_row[ROW16 ? kRow16Lds : 1];

  const int tid = threadIdx.x;
  const int f = FPW == 1 ? 0 : tid / T, t = FPW == 1 ? tid : tid % T;   // (FPW == 1: the base stays provably uniform)
  const long groups = (batch + FPW - 1) / FPW;
  long g = blockIdx.x;
  if (g >= groups) return;   // whole workgroup (uniform): launchers never over-provision the grid
  // the first transform's loads are issued before anything else: they fly while the tables are filled
  cpx v[E], vn[E];
  {
    const long b = g * FPW + f;
    lds_fft_load<LOGN, MODE, FWD>(v, data + (b < batch ? b : batch - 1) * (long)N, t);
  }
  for (int i = tid; i < (TWO ? kLane13Lds : N / 2); i += WG) s_tab[TWO ? lane_lds_index(i) : i] = tab_g[i];
  if constexpr (ROW16) lds_fill_row16<LOGN>(s_row, tab_g, tid, WG);
  cpx *xb = s_x + f * G::PADN;
  // the lane's own twiddle constants: W_8192^t (n = 8192); W_16384^t, ^(2 t), ^(3 t) (n = 16384)
  cpx wl[LOGN == 14 ? 3 : 1];
  wl[0] = mk(1.f, 0.f);
  if constexpr (TWO) {
#pragma unroll
    for (int k = 0; k < (LOGN == 14 ? 3 : 1); k++) wl[k] = tab_g[kLane13Lds + k * T + t];
  }

  // pack / unpack twiddles of this lane's pairs are the same for every transform
  constexpr int NP = (MODE == MODE_C2C) ? 1 : (E / 2 > 0 ? E / 2 : 1);
  // packed real transforms pair bins i, N-i inside the remainder pass when it has two butterflies
  // per lane (fft_device.hpp, pass_last_paired / pass_first_paired): one LDS exchange less
  constexpr bool PAIRED = MODE != MODE_C2C && pair_ok(LOGN, G::LOGE);
  constexpr int RREM = 1 << pass_rem_logr(LOGN, G::LOGE);
  // n = 8192 (M of config 3): the lane's eight pack twiddles W_16384^i, i = t + 512 u and 4096 - i, all
  // derive from ONE lane constant (g0 = w2[t]) times compile-time constants W_32^u, the partners being
  // -+i conj(.) — 2 VGPRs across the batch loop instead of 16 (the kernel runs under a 128-VGPR cap)
  constexpr bool W2LANE = TWO && PAIRED;
  // the pair maps' factors of 1/2 folded away (fft_device.hpp, r2c_pair_prescaled / c2r_pair_halfw): the forward
  // kernel scales its 16 values by 1 / (2N) instead of 1/N, the inverse kernel keeps its pair twiddles halved
  constexpr bool HALFW = MODE == MODE_C2R && PAIRED && LOGN != 14;   // (pair_tw14 carries unscaled constants for lane 0)
  constexpr bool PRESC = MODE == MODE_R2C && PAIRED;
  constexpr float wsc = HALFW ? 0.5f : 1.0f;
  cpx w2r[W2LANE ? 1 : NP];
  if constexpr (W2LANE) {
    w2r[0] = cscale(w2_g[t], wsc);
  } else if constexpr (MODE != MODE_C2C) {
#pragma unroll
    for (int k = 0; k < NP; k++) {
      if constexpr (PAIRED) w2r[k] = cscale(w2_g[pair_index<LOGN, G::LOGE>(t, k / RREM, k % RREM)], wsc);
      else w2r[k] = w2_g[t + T * k];
    }
  }
  // pair k = 2 u + q of the lane (pair_index): q = 0 -> w2[t + 512 u], q = 1 -> w2[4096 - (t + 512 u)]
  // (lane 0, u = 0: w2[2048] = W_8, with the table's sign)
  auto w2_of = [&](int k, int lane) -> cpx {
    if constexpr (W2LANE && LOGN == 14) {
      // pair k = 4 u + q of the lane: w2[i] = W_32768^i, i = pair_index(t, u, q), from the lane constant w2[t]
      return pair_tw14<FWD, 0>(w2r[0], k >> 2, k & 3, lane);
    } else if constexpr (W2LANE) {
      constexpr float c32[4] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f};
      constexpr float s32[4] = {0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f};
      const int u = k >> 1;
      cpx w = w2r[0];
      if (u == 1) w = ctw<FWD>(w, c32[1], s32[1]);
      if (u == 2) w = ctw<FWD>(w, c32[2], s32[2]);
      if (u == 3) w = ctw<FWD>(w, c32[3], s32[3]);
      if (k & 1) {
        w = FWD ? mk(-w.y, -w.x) : mk(w.y, w.x);   // W^(4096 - i) = -i conj(W^i) (forward sign), +i conj (inverse)
        if (k == 1 && lane == 0) w = mk(kC8 * wsc, (FWD ? -kC8 : kC8) * wsc);
      }
      return w;
    } else {
      return w2r[k];
    }
  };
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; e++) asm volatile("" : "+v"(v[e]));
  const int t_invariant = t;
#pragma unroll 1
  for (; g < groups; g += gridDim.x) {
    // Re-derive the lane index inside the loop through an opaque move: otherwise hipcc hoists every
    // LDS scatter/gather offset and global offset of all passes out of the batch loop, keeps
    // ~100 of them live across it and spills them (seen in the ISA as scratch stores in the
    // prologue and scratch loads in the loop).  Recomputing them costs a few VALU instructions.
    int t = t_invariant;
    asm volatile("" : "+v"(t));
    const auto tab2 = [&]() {
      if constexpr (LOGN == 14) return LaneTab14{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl[0], wl[1], wl[2]};
      else return LaneTab13{s_tab + kRow16Stride * (t & 15), s_tab + kRow16Lds + (t & 255), wl[0]};
    }();
    const auto tab1 = [&]() {
      if constexpr (ROW16) return HalfRowTab{s_tab, s_row + kRow16Stride * (t & 15)};
      else return static_cast<const cpx *>(s_tab);
    }();
    const long b = g * FPW + f;
    const bool active = b < batch;
    cpx *x = data + (active ? b : batch - 1) * (long)N;
    // software prefetch: the next transform's loads fly while this one is in the passes.
    // Always issued (index clamped to the last transform) so that it is straight-line code.
    // (every LDS size has it — LdsGeom::PREFETCH; at n = 8192 it fits under the 128-VGPR cap and is worth 5 %)
    if constexpr (G::PREFETCH) {
      long gn = g + gridDim.x;
      gn = gn < groups ? gn : groups - 1;
      const long bn = gn * FPW + f;
      lds_fft_load<LOGN, MODE, FWD>(vn, data + (bn < batch ? bn : batch - 1) * (long)N, t);
    }
    if constexpr (MODE == MODE_C2R && PAIRED) {
      // fused reference `iconv` (cl_fft.cpp:192-205) in registers, then the transposed pass chain
      cpx oi[E / 2], oj[E / 2];
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        const int i = pair_index<LOGN, G::LOGE>(t, k / RREM, k % RREM);
        if constexpr (HALFW) c2r_pair_halfw(v[2 * k], v[2 * k + 1], w2_of(k, t), oi[k], oj[k]);
        else c2r_pair(v[2 * k], v[2 * k + 1], w2_of(k, t), oi[k], oj[k]);
        if (k == 0) {   // lane 0: packed DC/Nyquist, bin N/2 copied through (selects, not a branch)
          const bool z = i == 0;
          oi[0] = mk(z ? v[0].x + v[0].y : oi[0].x, z ? v[0].x - v[0].y : oi[0].y);
          oj[0] = mk(z ? v[1].x : oj[0].x, z ? v[1].y : oj[0].y);
        }
      }
      if constexpr (TWO) pass_first_paired<LOGN, G::LOGE, FWD>(v, t, oi, oj, tab2);
      else pass_first_paired<LOGN, G::LOGE, FWD>(v, t, oi, oj, tab1);
      __syncthreads();
      pass_first_paired_scatter<LOGN, G::LOGE>(v, t, xb);
      __syncthreads();
      constexpr int L1 = pass_last_logns(LOGN, G::LOGE) - G::LOGE;
      if constexpr (TWO) wg_passes_dif_after<LOGN, G::LOGE, L1, FWD>(v, t, tab2, xb);
      else wg_passes_dif_after<LOGN, G::LOGE, L1, FWD>(v, t, tab1, xb);
    } else {
      if constexpr (MODE == MODE_C2R) {
        // fused reference `iconv` (cl_fft.cpp:192-205) on the way in
        __syncthreads();
#pragma unroll
        for (int k = 0; k < E / 2; k++) {
          const int i = t + T * k;
          if (i == 0) {
            xb[0] = mk(v[0].x + v[0].y, v[0].x - v[0].y);
            xb[lds_pad(N / 2)] = v[1];
          } else {
            cpx oi, oj;
            c2r_pair(v[2 * k], v[2 * k + 1], w2r[k], oi, oj);
            xb[lds_pad(i)] = oi;
            xb[lds_pad(N - i)] = oj;
          }
        }
        __syncthreads();
        pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
      }
      constexpr bool PL = MODE == MODE_R2C && PAIRED;
      // n = 8192: the middle passes on permuted lanes (fft_wg.hpp, wg_passes_sigma): conflict-free gathers
      if constexpr (TWO && FPW == 1) {
        const int ts = lane_sigma(t);
        const auto tab2s = [&]() {
          if constexpr (LOGN == 14) return LaneTab14{s_tab + kRow16Stride * (ts & 15), s_tab + kRow16Lds + (ts & 255), wl[0], wl[1], wl[2]};
          else return LaneTab13{s_tab + kRow16Stride * (ts & 15), s_tab + kRow16Lds + (ts & 255), wl[0]};
        }();
        wg_passes_sigma<LOGN, G::LOGE, 0, FWD, PL>(v, t, ts, tab2, tab2s, xb);
      } else if constexpr (TWO) wg_passes<LOGN, G::LOGE, 0, FWD, PL>(v, t, tab2, xb);
      else wg_passes<LOGN, G::LOGE, 0, FWD, PL>(v, t, tab1, xb);
    }

    if constexpr (SCALE || PRESC) {
      constexpr float inv = (SCALE ? 1.0f / (float)N : 1.0f) * (PRESC ? 0.5f : 1.0f);
#pragma unroll
      for (int e = 0; e < E; e++) v[e] = cscale(v[e], inv);
    }

    // Stores are unconditional as well (same reason as the loads).  Lanes of a ragged last
    // group whose transform index is past the batch were clamped to the LAST transform: they
    // loaded the same input in the same instruction as its owner and store bit-identical output.
    (void)active;
    [[maybe_unused]] XferBuf xo{};
    x += out_off;   // every access from here on is a store of this transform's results
    if constexpr (kLdsBufAddr<LOGN, MODE, FWD>) xo = xfer_buf<LOGN>(x, t);
    if constexpr (MODE == MODE_R2C && PAIRED) {
      // fused reference `conv` (cl_fft.cpp:178-191): both bins of every pair are in this lane's registers
      pairs_visit<LOGN, G::LOGE>(v, t, [&](int k, int i, cpx ci, cpx cj) {
        const int j = i == 0 ? N / 2 : N - i;
        cpx oi, oj;
        r2c_pair_prescaled(ci, cj, w2_of(k, t), oi, oj);   // (ci, cj carry the map's 1/2 already)
        if (k == 0 && i == 0) {   // packed DC/Nyquist; bin N/2 copied through
          oi = mk(ci.x + ci.y, ci.x - ci.y);
          oj = cscale(cj, 2.0f);
        }
        if constexpr (kLdsBufAddr<LOGN, MODE, FWD>) {
          const auto o = pair_off<LOGN, G::LOGE>(xo, t, k / RREM, k % RREM);
          st_buf(xo, o.vi, o.si, oi);
          st_buf(xo, o.vj, o.sj, oj);
        } else {
          st_nt(x + i, oi);
          st_nt(x + j, oj);
        }
      });
    } else if constexpr (MODE == MODE_R2C) {
      // fused reference `conv` (cl_fft.cpp:178-191) on the way out
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; e++) xb[lds_pad(t + T * e)] = v[e];
      __syncthreads();
#pragma unroll
      for (int k = 0; k < E / 2; k++) {
        // branch-free: pair 0 is (bin 0 packed DC/Nyquist, bin N/2 copied through), selected by value
        const int i = t + T * k;
        const int j = i == 0 ? N / 2 : N - i;
        const cpx ci = xb[lds_pad(i)], cj = xb[lds_pad(j)];
        cpx oi, oj;
        r2c_pair(ci, cj, w2r[k], oi, oj);
        if (i == 0) {
          oi = mk((ci.x + ci.y) * .5f, (ci.x - ci.y) * .5f);
          oj = cj;
        }
        if constexpr (kLdsBufAddr<LOGN, MODE, FWD>) {
          st_buf(xo, xo.va, T * k * 8, oi);
          if (k == 0) st_buf(xo, t == 0 ? (N / 2) * 8 : (N - t) * 8, 0, oj);
          else st_buf(xo, xo.vd, (N - T * k - T) * 8, oj);
        } else {
          st_nt(x + i, oi);
          st_nt(x + j, oj);
        }
      }
    } else if constexpr (kLdsBufAddr<LOGN, MODE, FWD>) {
#pragma unroll
      for (int e = 0; e < E; e++) st_buf(xo, xo.va, T * e * 8, v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < E; e++) st_nt(x + t + T * e, v[e]);
    }
    // Consume the prefetch HERE, in straight-line code after the stores: hipcc then waits with an
    // exact s_waitcnt vmcnt(<stores still in flight>).  If the first use were at the loop top, the
    // wait would be merged with the loop-entry path and drain this iteration's stores as well.
    if constexpr (G::PREFETCH) {
#pragma unroll
      for (int e = 0; e < E; e++) {
        asm volatile("" : "+v"(vn[e]));
        v[e] = vn[e];
      }
    } else {
      // no prefetch: load the next transform now (clamped, straight-line)
      long gn = g + gridDim.x;
      gn = gn < groups ? gn : groups - 1;
      const long bn = gn * FPW + f;
      lds_fft_load<LOGN, MODE, FWD>(v, data + (bn < batch ? bn : batch - 1) * (long)N, t);
    }
  }
}

template <int LOGN, bool FWD, int MODE, bool SCALE>
__global__ __launch_bounds__(LdsGeom<LOGN>::WG, LdsGeom<LOGN>::MIN_WAVES) void k_fft_lds(cpx *__restrict__ data,
                                                              const cpx *__restrict__ tab_g,
                                                              const cpx *__restrict__ w2_g, long batch, long out_off) {
  fft_lds_body<LOGN, FWD, MODE, SCALE>(data, tab_g, w2_g, batch, out_off);
}

// ---------------------------------------------------------------------------------
// n = 8 .. 64 (packed real: .. 256): the same passes, but global memory is touched in workgroup-wide coalesced rows
// ---------------------------------------------------------------------------------
// With T = n/16 < 8 lanes per transform, "lane t owns positions t + T*e" makes a wave's load touch 64
// different cache lines with 8..32 useful bytes each (measured: n = 16 at 0.96 TB/s).  Here the 256
// transforms of a workgroup (one contiguous chunk of 256*E elements) are read in E fully coalesced
// rows of 256 elements, parked in the per-transform padded LDS buffers at their natural positions, and
// picked up from there in the owning lanes' order (pass_gather_padded); results go back the same way.
template <int LOGN, bool FWD, int MODE, bool SCALE>
__global__ __launch_bounds__(256) void k_fft_small(cpx *__restrict__ data, long out_off, const cpx *__restrict__ tab_g,
                                                   const cpx *__restrict__ w2_g, long batch) {
  using G = LdsGeom<LOGN>;
  constexpr int N = G::N, E = G::E, T = G::T, FPW = G::FPW, CHUNK = FPW * N;
  static_assert(G::WG == 256 && CHUNK == 256 * E, "one chunk = E rows of 256 elements");
  __shared__ cpx s_tab[G::HALF];
  __shared__ cpx s_w2[MODE == MODE_C2C ? 1 : N / 2];
  __shared__ cpx s_x[FPW * G::PADN];
  const int tid = threadIdx.x;
  const int f = tid / T, t = tid % T;
  for (int i = tid; i < N / 2; i += 256) s_tab[i] = tab_g[i];
  if constexpr (MODE != MODE_C2C)
    for (int i = tid; i < N / 2; i += 256) s_w2[i] = w2_g[i];
  cpx *xb = s_x + f * G::PADN;
  // element `tid + 256*e` of the chunk: transform (tid >> LOGN) + (256 >> LOGN)*e, position tid & (N-1)
  cpx *park = s_x + (tid >> LOGN) * G::PADN + lds_pad(tid & (N - 1));
  constexpr int PARK_STEP = (256 >> LOGN) * G::PADN;
  const long groups = (batch + FPW - 1) / FPW;
  const long total = batch * (long)N;
  long g = blockIdx.x;
  if (g >= groups) return;
  cpx raw[E];
  auto load_rows = [&](long grp) {
    const long base = grp * CHUNK;
#pragma unroll
    for (int e = 0; e < E; e++) {
      long idx = base + tid + 256 * e;
      idx = idx < total ? idx : total - 1;   // ragged last group: clamped, straight-line
      raw[e] = ld_nt(data + idx);
    }
  };
  // the reference's pair maps (cl_fft.cpp:178-205) in place on the natural-order LDS copy: lane t of a
  // transform owns pairs i = t + T*k (and their partners n - i); pair 0 is the packed DC/Nyquist bin
  auto pair_map = [&]() {
#pragma unroll
    for (int k = 0; k < E / 2; k++) {
      const int i = t + T * k, j = i == 0 ? N / 2 : N - i;
      const cpx ci = xb[lds_pad(i)], cj = xb[lds_pad(j)];
      cpx oi, oj;
      if constexpr (MODE == MODE_R2C) r2c_pair(ci, cj, s_w2[i], oi, oj);
      else c2r_pair(ci, cj, s_w2[i], oi, oj);
      if (k == 0) {   // selects, not a branch
        const bool z = i == 0;
        const float h = MODE == MODE_R2C ? .5f : 1.f;
        oi = mk(z ? (ci.x + ci.y) * h : oi.x, z ? (ci.x - ci.y) * h : oi.y);
        oj = mk(z ? cj.x : oj.x, z ? cj.y : oj.y);
      }
      xb[lds_pad(i)] = oi;
      xb[lds_pad(j)] = oj;
    }
  };
  load_rows(g);
#pragma unroll
  for (int e = 0; e < E; e++) asm volatile("" : "+v"(raw[e]));
  __syncthreads();
#pragma unroll 1
  for (; g < groups; g += gridDim.x) {
    cpx v[E];
#pragma unroll
    for (int e = 0; e < E; e++) park[e * PARK_STEP] = raw[e];
    {  // the next chunk's rows fly behind this one's passes
      long gn = g + gridDim.x;
      load_rows(gn < groups ? gn : groups - 1);
    }
    __syncthreads();
    if constexpr (MODE == MODE_C2R) {
      pair_map();
      __syncthreads();
    }
    pass_gather_padded<LOGN, G::LOGE>(v, t, xb);
    wg_passes<LOGN, G::LOGE, 0, FWD>(v, t, s_tab, xb);
    if constexpr (SCALE) {
#pragma unroll
      for (int e = 0; e < E; e++) v[e] = cscale(v[e], 1.0f / (float)N);
    }
    __syncthreads();   // every lane is done with the exchange buffer
    dif_scatter_padded<LOGN, G::LOGE>(v, t, xb);
    __syncthreads();
    if constexpr (MODE == MODE_R2C) {
      pair_map();
      __syncthreads();
    }
    const long base = g * CHUNK;
    const bool full = base + CHUNK <= total;   // uniform
    if (full) {
#pragma unroll
      for (int e = 0; e < E; e++) st_nt(data + out_off + base + tid + 256 * e, park[e * PARK_STEP]);
    } else {
#pragma unroll
      for (int e = 0; e < E; e++)
        if (base + tid + 256 * e < total) data[out_off + base + tid + 256 * e] = park[e * PARK_STEP];
    }
    __syncthreads();   // the parked results are out before the next chunk is parked
#pragma unroll
    for (int e = 0; e < E; e++) asm volatile("" : "+v"(raw[e]));
  }
}

// How many workgroups of the persistent grids share a CU.  NOT "as many as fit": these kernels keep the next transform's
// loads in flight behind the current one's passes, so one workgroup per CU already covers the memory latency, and every
// further one only adds concurrent streams for the memory controllers to interleave.  Chosen per size and packing from
// interleaved A/Bs on random data, directions alternating (profiles/wgs_per_cu_r05.txt; one / two / three / all that fit):
// n = 1024 at one workgroup per CU 6.02 TB/s, at the three that fit 5.37; n = 16 .. 2048 and 8192 -4 .. -11 % of the time;
// n = 8 and n = 4096 like two.  The packed real kernels' pair maps stall between barriers, so most of them want company:
// sizes 8, 16, 64 .. 512, 2048, 4096 take two, sizes 32 and 1024 one (-2 .. -22 % against what fits at 2 GiB per launch),
// sizes 8192 and 16384 stay.
// All of this holds for batches that STREAM from HBM: up to about twice the 256 MiB Infinity Cache the same A/B reads the
// other way (n = 1024: 16 MiB +21 %, 256 MiB +2 %, 512 MiB -5 %, 1 GiB -10 %; n = 64 still +8 % at 768 MiB, -4 % at 1 GiB),
// so the table applies from 1 GiB of transforms per launch and smaller batches keep every workgroup that fits.
static inline bool streaming_batch(long batch, int logn) { return (batch << logn) >= (1L << 27); }   // 8-byte samples: 1 GiB
template <int LOGN, int MODE> constexpr int wgs_per_cu() {
  if (MODE == MODE_C2C) return LOGN == 3 || LOGN == 12 ? 2 : (LOGN >= 4 && LOGN <= 13) ? 1 : 64;
  switch (LOGN) {   // packed real size 2^(LOGN + 1), at 2 GiB per launch (the second table of profiles/wgs_per_cu_r05.txt)
    // (size 16384: one or two, forward or inverse, within 1 %; size 8192: -2 % at best; size 2048 with one: -7 % at 2 GiB,
    // but behind two in a sweep at 1 GiB — two is never behind)
    case 4: case 9: return 1;
    case 2: case 3: case 5: case 6: case 7: case 8: case 10: case 11: return 2;
    default: return 64;
  }
}

template <int LOGN, bool FWD, int MODE, bool SCALE>
static hipError_t launch_small_one(cpx *data, const FftTables &t, long batch, const DeviceInfo &di, hipStream_t s, long out_off) {
  using G = LdsGeom<LOGN>;
  long groups = (batch + G::FPW - 1) / G::FPW;
  static int occ = 0;
  if (occ == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_fft_small<LOGN, FWD, MODE, SCALE>, 256, 0) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    occ = nb;
  }
  long cap = (long)di.num_cus * (streaming_batch(batch, LOGN) && wgs_per_cu<LOGN, MODE>() < occ ? wgs_per_cu<LOGN, MODE>() : occ);
  int grid = (int)(groups < cap ? groups : cap);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((k_fft_small<LOGN, FWD, MODE, SCALE>), dim3(grid), dim3(256), 0, s, data, out_off, t.half, t.w2, batch);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// n = 2 and n = 4, complex: a copy kernel with a butterfly in it
// ---------------------------------------------------------------------------------
// Every lane moves 16 bytes (two complex samples) per access, lanes in address order — the access shape of a plain copy.
// n = 2: the lane holds the whole transform.  n = 4: lanes 2k and 2k + 1 hold (x0, x1) and (x2, x3) and read each other's
// pair through the DPP lane crossbar (quad_perm [1, 0, 3, 2]: four v_mov_dpp, no LDS); the even lane leaves with (X0, X1),
// the odd one with (X2, X3), so the stores are in address order as well.  The reference's two stages (cl_fft.cpp:24-41 on
// bit-reversed input): s0 = x0 + x2, d0 = x0 - x2, s1 = x1 + x3, d1 = x1 - x3; X0 = s0 + s1, X2 = s0 - s1,
// X1 = d0 + w d1, X3 = d0 - w d1, w = -i forward, +i inverse (exact in every rounding).  A workgroup moves contiguous
// runs of 256 * UNROLL pieces, UNROLL accesses of a lane in flight at once; a ragged tail is clamped on the load side and
// predicated on the store side (the lanes of a pair are always both inside or both outside: a transform is 32 bytes).
__device__ __forceinline__ float dpp_swap1(float v) {   // lane l <- lane l ^ 1
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
template <int LOGN, bool FWD, bool SCALE, int UNROLL>
__global__ __launch_bounds__(256) void k_fft_tiny(cpx *__restrict__ data, long out_off, long total16) {
  static_assert(LOGN == 1 || LOGN == 2, "n = 2 or 4");
  constexpr float sc = SCALE ? 1.0f / (float)(1 << LOGN) : 1.0f;
  constexpr long TILE = 256 * UNROLL;   // 16-byte pieces a workgroup moves per iteration: one contiguous run
  const bool odd = threadIdx.x & 1;
#pragma unroll 1
  for (long i0 = (long)blockIdx.x * TILE + threadIdx.x; i0 < total16; i0 += (long)gridDim.x * TILE) {
    f4v q[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      long i = i0 + u * 256;
      i = i < total16 ? i : total16 - 1;   // ragged tail: clamped, the result is not stored
      q[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(data + 2 * i));
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      const f4v m = q[u];
      f4v r;
      if constexpr (LOGN == 1) {
        r = f4v{(m.x + m.z) * sc, (m.y + m.w) * sc, (m.x - m.z) * sc, (m.y - m.w) * sc};
      } else {
        const f4v o = f4v{dpp_swap1(m.x), dpp_swap1(m.y), dpp_swap1(m.z), dpp_swap1(m.w)};
        // (x0, x1) = even lane's pair, (x2, x3) = odd lane's: sums are symmetric, differences change sign in the odd lane
        const float s0x = m.x + o.x, s0y = m.y + o.y, s1x = m.z + o.z, s1y = m.w + o.w;
        const float d0x = odd ? o.x - m.x : m.x - o.x, d0y = odd ? o.y - m.y : m.y - o.y;
        const float d1x = odd ? o.z - m.z : m.z - o.z, d1y = odd ? o.w - m.w : m.w - o.w;
        // w d1, w = -i (forward): (d1y, -d1x); +i (inverse): (-d1y, d1x)
        const float wx = FWD ? d1y : -d1y, wy = FWD ? -d1x : d1x;
        r = f4v{(odd ? s0x - s1x : s0x + s1x) * sc, (odd ? s0y - s1y : s0y + s1y) * sc,
                (odd ? d0x - wx : d0x + wx) * sc, (odd ? d0y - wy : d0y + wy) * sc};
      }
      const long i = i0 + u * 256;
      if (i < total16) st_nt16(data + out_off + 2 * i, r);
    }
  }
}
// Two accesses per lane in flight and four workgroups per CU: 5.9-6.1 TB/s in place (the chip's plain copy); one or eight
// workgroups per CU, or four / eight accesses per lane, 3.3-5.8 (profiles/tiny_r05.txt).
template <int LOGN, bool FWD, bool SCALE>
static hipError_t launch_tiny_one(cpx *data, long batch, const DeviceInfo &di, hipStream_t s, long out_off) {
  constexpr int UNROLL = 2;
  const long total16 = batch << (LOGN - 1);   // 16-byte pieces
  const long want = (total16 + 256 * UNROLL - 1) / (256 * UNROLL);
  const long cap = 4L * di.num_cus;
  hipLaunchKernelGGL((k_fft_tiny<LOGN, FWD, SCALE, UNROLL>), dim3((int)(want < cap ? want : cap)), dim3(256), 0, s, data, out_off, total16);
  return hipGetLastError();
}

template <int LOGN, bool FWD, int MODE, bool SCALE>
static hipError_t launch_lds_one(cpx *data, const FftTables &t, long batch, const DeviceInfo &di,
                                 hipStream_t s, long out_off) {
  using G = LdsGeom<LOGN>;
  long groups = (batch + G::FPW - 1) / G::FPW;
  // persistent grid: exactly the workgroups that are resident at once (occupancy x CUs), each
  // grid-striding over many transforms, so the LDS twiddle table is loaded once per workgroup
  // and every transform but the first is software-prefetched
  static int occ = 0;  // per instantiation
  if (occ == 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_fft_lds<LOGN, FWD, MODE, SCALE>, G::WG, 0) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    occ = nb;
  }
  long cap = (long)di.num_cus * (streaming_batch(batch, LOGN) && wgs_per_cu<LOGN, MODE>() < occ ? wgs_per_cu<LOGN, MODE>() : occ);
  int grid = (int)(groups < cap ? groups : cap);
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((k_fft_lds<LOGN, FWD, MODE, SCALE>), dim3(grid), dim3(G::WG), 0, s, data, t.half, t.w2, batch, out_off);
  return hipGetLastError();
}

template <int LOGN>
static hipError_t launch_lds_n(bool fwd, int mode, bool scale, cpx *data, const FftTables &t, long batch,
                               const DeviceInfo &di, hipStream_t s, long out_off) {
#define CLFA_CASE(F, M, S)                                                                                     \
  if (fwd == F && mode == M && scale == S) {                                                                   \
    /* tiny, else small, else lds: the predicates the kernel's name is chosen by (fft_route.hpp) */           \
    if constexpr (lds_tiny(LOGN, M)) return launch_tiny_one<LOGN, F, S>(data, batch, di, s, out_off);          \
    if constexpr (lds_small(LOGN, M)) return launch_small_one<LOGN, F, M, S>(data, t, batch, di, s, out_off);  \
    else return launch_lds_one<LOGN, F, M, S>(data, t, batch, di, s, out_off);                                 \
  }
  CLFA_CASE(true, MODE_C2C, true)
  CLFA_CASE(true, MODE_C2C, false)
  CLFA_CASE(false, MODE_C2C, false)
  CLFA_CASE(true, MODE_R2C, true)
  CLFA_CASE(false, MODE_C2R, false)
#undef CLFA_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_fft_lds(int logn, bool fwd, int mode, bool scale, cpx *data, const FftTables &t,
                          long batch, const DeviceInfo &di, hipStream_t s, long out_off) {
  if (batch <= 0) return hipSuccess;
  switch (logn) {
#define CLFA_N(L) \
  case L:         \
    return launch_lds_n<L>(fwd, mode, scale, data, t, batch, di, s, out_off);
    CLFA_N(1) CLFA_N(2) CLFA_N(3) CLFA_N(4) CLFA_N(5) CLFA_N(6) CLFA_N(7) CLFA_N(8) CLFA_N(9) CLFA_N(10)
    CLFA_N(11) CLFA_N(12) CLFA_N(13)
#undef CLFA_N
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace clfa
