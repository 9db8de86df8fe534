// fft_res_real.inc (part of the translation unit fft_resident.hip) — the pair maps of the packed real transforms of size
// 2 kN = 131072 that k_fft_res16<R2C> runs inside phase 2 and k_fft_res16<C2R> inside phase 1.

namespace clfa {
namespace {

// ---- packed real transforms of size 2 kN = 131072, forward (R2C): the reference's `conv` pair map (cl_fft.cpp:178-191)
// inside phase 2, so that the transform still crosses HBM once.
//
// The map combines bins i and M - i (M = kN).  With i = 16 q + c + 256 (t + 16 e) (row block q, lane (c, t), register
// e) the partner is 16 (15 - q) + (16 - c) + 256 (15 - t) + 4096 (15 - e): row block 15 - q, and — if that block is
// worked through MIRRORED lane maps (the lane reads row (16 - c) mod 16 of the exchange and the first pass's output
// 15 - t) — the same lane's register 15 - e.  So phase 2 runs the row blocks in pairs A = q, B = 15 - q (q = 0..7),
// B mirrored, and the map is register-to-register in every lane with c != 0.  The lanes c = 0 (rows k1 = 16 rb) pair
// one block further: A_q's with B_(q-1)'s (still in the same lane), which is why B's results stay parked for one
// more block (in the AGPR row that block 15 has left free) and are completed there before their stores are issued;
// rows k1 = 0 (in A_0) and k1 = 128 (in B_7) pair within themselves, across the 16 lanes c = 0, through 2 KiB of LDS.
// Pair twiddles W_2M^i = W_2M^(16 q + c) * W_512^t * W_32^e: two lookups (the first 256 entries of the plan's w2 table
// and every 256th) and compile-time constants.  The map's 1/2 rides on the 1/N of the table (r2c_pair_prescaled).

// build switch of the packed real variants (debugging)
#ifndef CLFA_C2R_WAIT
#define CLFA_C2R_WAIT 1      // 0: every counted wait of the two packed real variants is vmcnt(0) (tools/check_waits.py)
#endif
constexpr bool kC2rWait = CLFA_C2R_WAIT;
// the inverse variant's natural loads cached as well: per 1024 transforms all streaming 0.265 ms, the mirrored
// loads cached 0.253, all cached 0.245 (profiles/rfft131072_fused_r04.txt)
constexpr bool kC2rKeepA = true;
constexpr int kTabPair = kTabSize;   // [W_2M^k, k < 256 | W_512^t, t < 16]
constexpr int kTabSizeR = kTabSize + 272;
constexpr int kParkAcc = 224;        // B' results parked in a[224:255] (keep row 15's registers, fetched first)
constexpr int kSlotAcc = 192;        // the slot's row block lands in a[192:223] (keep row 14's, free after pair 1)

// W_2M^i of the lane's register e: base * W_32^e
template <int E, bool FWD = true> __device__ __forceinline__ cpx pair_tw_e(cpx base) {
  if constexpr (E == 0) return base;
  else return ctw<FWD>(base, kC32[E], kS32[E]);
}
// r2c_pair_prescaled (fft_device.hpp) in six packed instructions: the conjugations and the rotation by i ride on the
// operand modifiers.  One wave per SIMD pays for every instruction in full, so the map is written out here.
__device__ __forceinline__ void r2c_pair6(cpx a, cpx b, cpx w, cpx &oi, cpx &oj) {
  cpx e, r, x, y;
  asm("v_pk_add_f32 %0, %4, %5 neg_hi:[0,1]\n\t"                                 // e = a + conj(b)
      "v_pk_add_f32 %1, %4, %5 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]\n\t"    // r = i (conj(b) - a) = (a.y + b.y, b.x - a.x)
      "v_pk_mul_f32 %2, %6, %1 op_sel_hi:[0,1]\n\t"                              // x = w r
      "v_pk_fma_f32 %2, %6, %1, %2 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
      "v_pk_add_f32 %3, %0, %2 neg_lo:[0,1] neg_hi:[1,0]\n\t"                    // y = conj(e - x)
      "v_pk_add_f32 %2, %0, %2"                                                   // x = e + x
      : "=&v"(e), "=&v"(r), "=&v"(x), "=&v"(y)
      : "v"(a), "v"(b), "v"(w));
  oi = x;
  oj = y;
}
// ... with the A value in (and the result back into) the landing register pair of register E: no moves
template <int E> __device__ __forceinline__ void r2c_pair6_land(cpx &b, cpx w) {
  cpx e, r, y;
  asm volatile("v_pk_add_f32 %0, v[%c5:%c6], %3 neg_hi:[0,1]\n\t"
               "v_pk_add_f32 %1, v[%c5:%c6], %3 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]\n\t"
               "v_pk_mul_f32 v[%c5:%c6], %4, %1 op_sel_hi:[0,1]\n\t"
               "v_pk_fma_f32 v[%c5:%c6], %4, %1, v[%c5:%c6] op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
               "v_pk_add_f32 %2, %0, v[%c5:%c6] neg_lo:[0,1] neg_hi:[1,0]\n\t"
               "v_pk_add_f32 v[%c5:%c6], %0, v[%c5:%c6]"
               : "=&v"(e), "=&v"(r), "=&v"(y)
               : "v"(b), "v"(w), "n"(224 + 2 * E), "n"(225 + 2 * E));
  b = y;
}
// lanes c != 0, end of pair q: the A block (raw, in the landing registers) against the B block (raw, in v); A' stays
// in the landing registers, B' in v
__device__ __forceinline__ void res_pair_map(cpx (&v)[16], cpx base) {
  static_for<16>([&](auto E) {
    constexpr int e = decltype(E)::value;
    r2c_pair6_land<e>(v[15 - e], pair_tw_e<e>(base));
    // (every two pairs a fence: hipcc otherwise piles up all 16 twiddles and spills — into AGPRs, this kernel's own)
    if (e & 1) __builtin_amdgcn_sched_barrier(0);
  });
}
// lanes c = 0, pair q >= 1, after the A block: its rows k1 = 16 q pair with the previous B block's k1 = 16 (16 - q),
// parked raw in a[kParkAcc ...] of these lanes; both are finished here
__device__ __forceinline__ void res_pair_patch_c0(cpx (&v)[16], cpx base) {
  static_for<16>([&](auto E) {
    constexpr int e = decltype(E)::value, pe = kParkAcc + 2 * (15 - e);
    const cpx bq = mk(acc_read<pe>(), acc_read<pe + 1>());
    cpx oi, oj;
    r2c_pair6(v[e], bq, pair_tw_e<e>(base), oi, oj);
    v[e] = oi;
    asm volatile("" : "+v"(v[e]));
    acc_write<pe>(oj.x);
    acc_write<pe + 1>(oj.y);
    if (e & 1) __builtin_amdgcn_sched_barrier(0);
  });
}
// lanes c = 0 of a block whose row pairs within itself (k1 = 0: natural lanes, k2 = t + 16 e; k1 = 128: mirrored
// lanes, k2 = (15 - t) + 16 e): the partners are in other lanes c = 0 -> through s_c0[t][e].  Every lane computes
// its own 16 results (each pair twice, by both of its lanes).  ROW0 has the reference's two exceptions: bin 0 packs
// DC / Nyquist, bin M/2 is left as the complex transform made it (cl_fft.cpp:178-191 starts at i = 1 and never
// reaches M/2).  Called by all lanes (barrier inside).
template <bool ROW0> __device__ __forceinline__ void res_pair_self_row(cpx (&v)[16], int c, int t, cpx base, cpx *s_c0) {
  if (c == 0) {
#pragma unroll
    for (int e = 0; e < 16; e++) s_c0[t * 16 + e] = v[e];
  }
  __syncthreads();
  if (c == 0) {
    static_for<16>([&](auto E) {
      constexpr int e = decltype(E)::value;
      int idx;
      if constexpr (ROW0) {
        const int k2 = (256 - (t + 16 * e)) & 255;
        idx = (k2 & 15) * 16 + (k2 >> 4);
      } else {
        idx = (15 - t) * 16 + (15 - e);
      }
      const cpx ci = v[e], zp = s_c0[idx];
      cpx oi, oj;
      r2c_pair6(ci, zp, pair_tw_e<e>(base), oi, oj);
      if constexpr (ROW0 && e == 0) {
        if (t == 0) oi = mk(ci.x + ci.y, ci.x - ci.y);
      }
      if constexpr (ROW0 && e == 8) {
        if (t == 0) oi = cscale(ci, 2.0f);
      }
      v[e] = oi;
      asm volatile("" : "+v"(v[e]));
      if (e & 1) __builtin_amdgcn_sched_barrier(0);
    });
  }
}

// ---- packed real transforms of size 2 kN = 131072, inverse (C2R): the reference's `iconv` pair map (cl_fft.cpp:192-205)
// inside phase 1.
//
// The input index has the structure of the forward kernel's output: i = 16 cb + c + 256 (t + 16 e) pairs with column
// 16 - c of column block 15 - cb, row (15 - t) + 16 (15 - e).  Phase 1 takes the column blocks in pairs A = q natural,
// B = 15 - q loaded through mirrored lanes (q = 7 .. 0): the map is register-to-register (A in the lane's registers,
// B in the landing registers), and B un-mirrors itself in its own exchange — the lane writes its first-pass results to
// column slot 16 - c at position 16 (15 - t) and the natural lanes read them.  The lanes c = 0 have loaded column 0 of
// block 16 - q (the partners of their A column): it belongs to the NEXT pair's B block, so its first-pass results go
// to a copy buffer that the next B block's lanes c = 0 read instead of slot 0 (loads do not mind the detour; the
// forward kernel's stores did, profiles/rfft131072_fused_r04.txt).  Columns 0 (in A_0) and 128 (block 8's, loaded
// separately before the first pair) pair within themselves across the 16 lanes c = 0.
// The map's two factors 1/2 ride on the four-step twiddle table (x 0.5); the untouched bins 0 and M/2 are doubled.
// Both blocks of the next pair are loaded along the A block (two loads per hook point, into the two AGPR zones; the
// B data then move to the landing registers); the last pair's B block comes through the landing registers directly.
__device__ __forceinline__ void c2r_pair6(cpx a, cpx b, cpx w, cpx &oi, cpx &oj) {
  cpx e, r, x, y;
  asm("v_pk_add_f32 %0, %4, %5 neg_hi:[0,1]\n\t"                                                // e = a + conj(b)
      "v_pk_add_f32 %1, %4, %5 op_sel:[1,1] op_sel_hi:[0,0] neg_lo:[1,1] neg_hi:[0,1]\n\t"      // r = i (a - conj(b))
      "v_pk_mul_f32 %2, %6, %1 op_sel_hi:[0,1]\n\t"                                             // x = w r
      "v_pk_fma_f32 %2, %6, %1, %2 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
      "v_pk_add_f32 %3, %0, %2 neg_lo:[0,1] neg_hi:[1,0]\n\t"                                   // y = conj(e - x)
      "v_pk_add_f32 %2, %0, %2"                                                                // x = e + x
      : "=&v"(e), "=&v"(r), "=&v"(x), "=&v"(y)
      : "v"(a), "v"(b), "v"(w));
  oi = x;
  oj = y;
}
// ... with the B value in (and its result back into) the landing register pair VB
template <int VB> __device__ __forceinline__ void c2r_pair6_land(cpx &a, cpx w) {
  cpx e, r, x;
  asm volatile("v_pk_add_f32 %0, %3, v[%c5:%c6] neg_hi:[0,1]\n\t"
               "v_pk_add_f32 %1, %3, v[%c5:%c6] op_sel:[1,1] op_sel_hi:[0,0] neg_lo:[1,1] neg_hi:[0,1]\n\t"
               "v_pk_mul_f32 %2, %4, %1 op_sel_hi:[0,1]\n\t"
               "v_pk_fma_f32 %2, %4, %1, %2 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
               "v_pk_add_f32 v[%c5:%c6], %0, %2 neg_lo:[0,1] neg_hi:[1,0]\n\t"
               "v_pk_add_f32 %2, %0, %2"
               : "=&v"(e), "=&v"(r), "=&v"(x)
               : "v"(a), "v"(w), "n"(VB), "n"(VB + 1));
  a = x;
}
// start of a pair: the A block (raw, in v) against the B block (raw, in the landing registers), both finished in place
__device__ __forceinline__ void res_unpair_map(cpx (&v)[16], cpx base) {
  static_for<16>([&](auto E) {
    constexpr int e = decltype(E)::value;
    c2r_pair6_land<224 + 2 * (15 - e)>(v[e], pair_tw_e<e, false>(base));
    if (e & 1) __builtin_amdgcn_sched_barrier(0);
  });
}
// lanes c = 0 of a column that pairs within itself (COL0: n2 = 0, natural lanes, row n1 = t + 16 e pairs with 256 - n1,
// rows 0 and 128 are the reference's untouched bins 0 and M/2; else n2 = 128, mirrored lanes, n1 = (15 - t) + 16 e pairs
// with 255 - n1).  Every lane computes its own 16 values.  Called by all lanes (barrier inside).
template <bool COL0> __device__ __forceinline__ void res_unpair_self_col(cpx (&v)[16], int c, int t, cpx base, cpx *s_c0) {
  if (c == 0) {
#pragma unroll
    for (int e = 0; e < 16; e++) s_c0[t * 16 + e] = v[e];
  }
  __syncthreads();
  if (c == 0) {
    static_for<16>([&](auto E) {
      constexpr int e = decltype(E)::value;
      int idx;
      if constexpr (COL0) {
        const int n1 = (256 - (t + 16 * e)) & 255;
        idx = (n1 & 15) * 16 + (n1 >> 4);
      } else {
        idx = (15 - t) * 16 + (15 - e);
      }
      const cpx ci = v[e], zp = s_c0[idx];
      cpx oi, oj;
      c2r_pair6(ci, zp, pair_tw_e<e, false>(base), oi, oj);
      if constexpr (COL0 && e == 0) {
        if (t == 0) oi = mk(2.0f * (ci.x + ci.y), 2.0f * (ci.x - ci.y));
      }
      if constexpr (COL0 && e == 8) {
        if (t == 0) oi = cscale(ci, 2.0f);
      }
      v[e] = oi;
      asm volatile("" : "+v"(v[e]));
      if (e & 1) __builtin_amdgcn_sched_barrier(0);
    });
  }
}
// zone Z1 (AGPR columns 12, 13) -> landing registers
__device__ __forceinline__ void res_zone1_to_land() {
  static_for<16>([&](auto E) {
    constexpr int e = decltype(E)::value, src = 32 * (e & 7) + 2 * (kZone1 + (e >> 3));
    asm volatile("v_accvgpr_read_b32 v[%c0], a[%c2]\n\tv_accvgpr_read_b32 v[%c1], a[%c3]" ::"n"(224 + 2 * e), "n"(225 + 2 * e), "n"(src), "n"(src + 1));
  });
}

}  // namespace
}  // namespace clfa
