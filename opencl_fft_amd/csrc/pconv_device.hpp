// pconv_device.hpp — device building blocks of the partitioned-convolution kernels (pconv_chain.hip, pconv_fused.inc,
// pconv_coop.hip, pconv_blocks.hip, pconv_matrix.hip, pconv_nup.hip), each defined once, and the launch plumbing their launchers share.
// The rules they carry exist once in the reference too: bin 0 of a packed frame holds DC and Nyquist and is multiplied component-wise; partial sums are added
// in a fixed ascending order; loads are clamped rather than predicated.
// Rule for a change here: compile these files before and after and compare them with tools/check_isa.py --same; a
// helper is used only where the kernel keeps its instructions.  Sites that carry the bin-0 rule in their own words because
// they did not: the c2r unpack, MAC term and overlap-add of k_pconv_fused and k_pconv_coop, the branch-form r2c pack of
// k_pconv_fwd and fwd_row (k_pconvb_fwd, k_nupc_fwd), and the tail loop of k_pconv_mac.  The same holds for the pass chains of k_pconv_fused and
// k_pconv_coop: each spells its forward and its inverse chain out (compute, barrier, scatter, barrier, gather, predicated on
// tid < T / work), because a recursive helper in the manner of wg_passes changed the instructions of all 32 instantiations.
#pragma once
#include <type_traits>

#include "fft_wg.hpp"

namespace clfa {

// ---- two adjacent bins (16 bytes) of a spectrum frame ------------------------------------------------------------------
struct alignas(16) cpx2 {
  cpx a, b;
};

// the rings (and the workspaces that stand in for them) are read exactly once per block and exceed the Infinity Cache at
// config 4: non-temporal 16-byte loads
__device__ __forceinline__ cpx2 ld_nt(const cpx2 *p) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f r = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(p));
  cpx2 o;
  o.a = mk(r.x, r.y);
  o.b = mk(r.z, r.w);
  return o;
}

// ---- one term of the multiply-accumulate (reference convol, cl_conv_kernels.h:102-118): (s0, s1) += x (.) h ----------
// dc: the lane's first bin is the packed DC / Nyquist bin, (re*re, im*im) — a select on the product, not a branch (a branch
// splits the loop body and the streaming loads stop overlapping).
__device__ __forceinline__ void mac_term(cpx &s0, cpx &s1, const cpx2 &x, const cpx2 &h, bool dc) {
  cpx pr = cmul_plain(x.a, h.a);
  pr = mk(dc ? x.a.x * h.a.x : pr.x, dc ? x.a.y * h.a.y : pr.y);
  s0 = cadd(s0, pr);
  s1 = cadd(s1, cmul_plain(x.b, h.b));
}

// ---- transform in natural order -> packed spectrum (reference r2c, cl_conv_kernels.h:61-85), on values ---------------
// pair (i, j = N - i) through the pair map; pair0: (bin 0, bin N/2) -> the packed (DC, Nyquist) bin and bin N/2 as it is
__device__ __forceinline__ void r2c_pack_pair(cpx ci, cpx cj, cpx w, bool pair0, cpx &oi, cpx &oj) {
  r2c_pair(ci, cj, w, oi, oj);
  if (pair0) {
    oi = mk((ci.x + ci.y) * .5f, (ci.x - ci.y) * .5f);
    oj = cj;
  }
}

// ---- one row of N real samples -> its packed spectrum frame (k_pconvb_fwd, k_nupc_fwd) -------------------------------
// (check_isa.py --same on k_pconvb_fwd with this helper: LOGB 6 and 8 keep their instructions; the other six keep their
// descriptors and the counts of every floating-point, LDS-read and global-memory instruction, and differ in the order and
// the registers of the integer address arithmetic — one v_mad_u32_u24 more or fewer, and at LOGB 7 one ds_write2_b64 as
// two ds_write_b64.  The table must stay an array reference and x a restrict pointer; with the frame computed by a
// functor hipcc emits a much shorter, different kernel.)
__device__ __forceinline__ cpx ld_pair(const float *p, bool aligned) {
  if (aligned) return *reinterpret_cast<const cpx *>(p);
  return mk(p[0], p[1]);
}
// One transform slot of a workgroup (lane t of its T, the slot's LDS row xb, the tables s_tab / w2_g): the samples at src,
// zero-padded to 2N, forward transform, r2c pack into x[0 .. N).  active: the slot has a row (the barriers are the whole
// workgroup's; the last one frees xb for the slot's next row).  keep(p, pair): sees pair p < N / 2 of the row as loaded
template <int LOGB, class Tab, class Keep>
__device__ __forceinline__ void fwd_row(const float *src, int aligned, bool active, cpx *__restrict__ x, int t, const Tab &s_tab,
                                        cpx *xb, const cpx *__restrict__ w2_g, Keep keep) {
  using G = LdsGeom<LOGB>;
  constexpr int N = G::N, E = G::E, T = G::T;
  cpx v[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    const int p = t + T * e;
    v[e] = (active && p < N / 2) ? ld_pair(src + 2 * p, aligned) : mk(0.f, 0.f);
    if (active && p < N / 2) keep(p, v[e]);
  }
  wg_passes<LOGB, G::LOGE, 0, true>(v, t, s_tab, xb);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < E; e++) xb[lds_pad(t + T * e)] = v[e];
  __syncthreads();
  if (active) {
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
  __syncthreads();
}

// ---- packed spectrum -> transform input in natural order (reference c2r, cl_conv_kernels.h:87-100) ------------------
// Pair i of N/2: bins (i, N - i) through the pair map; pair 0 is the packed bin (DC, Nyquist) and bin N/2, which the map
// does not visit.  ld(pos) / st(pos, value) see natural positions, w(i) is the pair twiddle.
template <int N, class Ld, class W, class St> __device__ __forceinline__ void c2r_unpack(int i, Ld ld, W w, St st) {
  if (i == 0) {
    const cpx c0 = ld(0);
    st(0, mk(c0.x + c0.y, c0.x - c0.y));
    st(N / 2, ld(N / 2));
  } else {
    cpx oi, oj;
    c2r_pair(ld(i), ld(N - i), w(i), oi, oj);
    st(i, oi);
    st(N - i, oj);
  }
}

// ---- the sliding window of input frames (k_pconvb_mac, k_pconvm_mac) ---------------------------------------------------
// consecutive outputs see consecutive input frames: the window moves by one per partition
template <int KT> __device__ __forceinline__ void window_shift(cpx2 (&win)[KT], const cpx2 &next) {
#pragma unroll
  for (int t = 0; t + 1 < KT; t++) win[t] = win[t + 1];
  win[KT - 1] = next;
}

// ---- commit launches: this call's results into the object's state, after every read of it ----------------------------
// spectra m0 .. K - 1 of every channel, X[ch][m] -> ring[ch][frame_of(m)]
template <class F>
__device__ __forceinline__ void commit_spectra(cpx *ring, const cpx *X, int m0, int K, int cap, int hb, int nparts,
                                               int channels, F frame_of) {
  const int cnt = K - m0;
  const long n = (long)channels * cnt * hb;
  const cpx2 *src = reinterpret_cast<const cpx2 *>(X);
  cpx2 *dst = reinterpret_cast<cpx2 *>(ring);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int item = (int)(i % hb);
    const long rest = i / hb;
    const int m = m0 + (int)(rest % cnt), ch = (int)(rest / cnt);
    dst[((long)ch * nparts + frame_of(m)) * hb + item] = src[((long)ch * cap + m) * hb + item];
  }
}
// ring A keeps the last min(K, nparts) spectra: m0 and the frame of spectrum m (w = the ring position before the call)
__device__ __forceinline__ int commit_first(int K, int nparts) { return K > nparts ? K - nparts : 0; }
__device__ __forceinline__ int ring_a_frame(int w, int m, int nparts) { return (w + m) % nparts; }

__device__ __forceinline__ void commit_tail(float *tail, const float *tail_new, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) tail[i] = tail_new[i];
}

// ---- launch plumbing (host) ---------------------------------------------------------------------------------------------
// f(std::integral_constant<int, L>) for L = logb in [LO, HI]: the launchers' way to their LdsGeom<L> instantiation
template <int LO, int HI, class F> hipError_t dispatch_logb(int logb, F f) {
  if constexpr (LO > HI) return hipErrorInvalidValue;
  else return logb == LO ? f(std::integral_constant<int, LO>{}) : dispatch_logb<LO + 1, HI>(logb, f);
}
// grid-stride kernels: one workgroup per group as far as `cap` goes
inline int grid_clamp(long groups, long cap) { return (int)(groups < cap ? groups : cap); }

}  // namespace clfa
