// fft_res_blocks.inc (part of the translation unit fft_resident.hip) — the arithmetic of k_fft_res16: the 16-point
// passes with their hook points, one column block (phase 1) and one row block (phase 2), and the moves between a
// block's results and the lane's keep matrix.  The LDS layouts and the table blob are defined here, next to their users.

namespace clfa {
namespace {

// the lane-private LDS rows of the keep matrix (rb 0..2), bytes per lane: 3 x 128 + 16 = 100 dwords.  The b128 reads of phase 2 (16-lane groups over 64 banks: 36 l mod 64) are
// conflict-free; the three ds_write_b64 of a deposit (16 contiguous lanes over 32 banks: 4 l mod 32) pair lanes l, l + 8 —
// 8 LDS-array cycles against the 6 the instruction takes to hand its operands over anyway: 2 cycles per write.  A stride
// that serves both (2 x odd dwords) would turn the reads into 16 x b64 for nothing measurable.
constexpr int kSpillStride = 400;
constexpr int kXA = 258;            // phase-1 exchange: element (column c, position p) at c * 258 + p
constexpr int kXB = 290;            // phase-2 exchange: element (row r, position p) at r * 290 + p + 2 (p / 16)
constexpr int kXSize = 16 * kXB;
// table blob (host: fill_res16_tables): [tw 16x16 | lo 256 | hi 256 | S 4x256]
constexpr int kTabTw = 0, kTabLo = 256, kTabHi = 512, kTabS = 768, kTabSize = 1792;

__device__ __forceinline__ f4 pack2(cpx a, cpx b) { return f4{a.x, a.y, b.x, b.y}; }

// hook-point maps: eight local points of dft16_h -> global hook numbers (-1: none)
struct HookMap {
  int p[8];
};
constexpr HookMap kMapColA{{0, -1, 1, -1, 2, -1, 3, -1}};      // column block, first pass: hooks 0..3
constexpr HookMap kMapColB{{8, -1, 9, -1, 10, -1, 11, -1}};    // ... second pass: hooks 8..11 (4..7: twiddles, 12..15: four-step)
constexpr HookMap kMapRowC{{0, 1, 2, -1, 3, 4, 5, -1}};        // row block, first pass: hooks 0..5
constexpr HookMap kMapRowD{{10, 11, 12, -1, 13, 14, 15, -1}};  // ... second pass: hooks 10..15 (6..9: twiddles)
// dft16 of fft_device.hpp with eight hook points
struct NoTail {
  __device__ __forceinline__ void operator()() const {}
};
// `tail` runs after hook point P6, ahead of the last two butterflies (res_col_block issues its table lookups there)
template <bool FWD, class H, int P0, int P1, int P2, int P3, int P4, int P5, int P6, int P7, class T = NoTail>
__device__ __forceinline__ void dft16_hp(cpx (&v)[16], const H &hook, const T &tail = T()) {
  bf4<FWD>(v[0], v[4], v[8], v[12]);
  hook_at<P0>(hook);
  bf4<FWD>(v[1], v[5], v[9], v[13]);
  hook_at<P1>(hook);
  bf4<FWD>(v[2], v[6], v[10], v[14]);
  hook_at<P2>(hook);
  bf4<FWD>(v[3], v[7], v[11], v[15]);
  ctw2<FWD>(v[4 + 1], kC16, kS16, v[4 + 2], kC8, kC8);
  hook_at<P3>(hook);
  ctw2<FWD>(v[4 + 3], kS16, kC16, v[8 + 1], kC8, kC8);
  ctw2<FWD>(v[8 + 3], -kC8, kC8, v[12 + 1], kS16, kC16);
  hook_at<P4>(hook);
  ctw2<FWD>(v[12 + 2], -kC8, kC8, v[12 + 3], -kC16, -kS16);
  cpx x[16];
#pragma unroll
  for (int t = 0; t < 16; t++) x[t] = v[t];
  bf4<FWD>(x[0], x[1], x[2], x[3]);
  hook_at<P5>(hook);
  bf4<FWD>(x[4], x[5], x[6], x[7]);
  hook_at<P6>(hook);
  tail();
  bf4_rot2<FWD>(x[8], x[9], x[10], x[11]);
  hook_at<P7>(hook);
  bf4<FWD>(x[12], x[13], x[14], x[15]);
#pragma unroll
  for (int q0 = 0; q0 < 4; q0++)
#pragma unroll
    for (int q1 = 0; q1 < 4; q1++) v[q0 + 4 * q1] = x[4 * q0 + q1];
}
// The last four butterflies of a row block's second pass with their results written straight into the landing registers
// (v[224 + 2 k] for result k): the block's results are stored from there along the next block, and the 16 moves of
// res_stage() are 3 % of this kernel's VALU instructions — which one wave per SIMD pays in full.  Result k = q0 + 4 q1 of
// butterfly q0 overwrites landing register k only after hook point k has issued its store (hooks 0..13 precede the first
// of these butterflies, 14 follows the first, 15 the second; butterfly q0 writes k = q0, q0 + 4, q0 + 8, q0 + 12).
#define CLFA_PLUS ""
#define CLFA_MINUS " neg_lo:[0,1] neg_hi:[0,1]"
#define CLFA_ROTF " op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]"   /* x + (-i) y */
#define CLFA_ROTI " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]"   /* x + (+i) y */
#define CLFA_BF4_LAND(M02A, M02B, MR1, MR3)                                                              \
  asm volatile("v_pk_add_f32 %0, %4, %6" M02A "\n\t"                                                     \
               "v_pk_add_f32 %1, %4, %6" M02B "\n\t"                                                     \
               "v_pk_add_f32 %2, %5, %7\n\t"                                                             \
               "v_pk_add_f32 %3, %5, %7" CLFA_MINUS "\n\t"                                               \
               "v_pk_add_f32 v[%c8:%c9], %0, %2\n\t"                                                     \
               "v_pk_add_f32 v[%c10:%c11], %1, %3" MR1 "\n\t"                                            \
               "v_pk_add_f32 v[%c12:%c13], %0, %2" CLFA_MINUS "\n\t"                                     \
               "v_pk_add_f32 v[%c14:%c15], %1, %3" MR3                                                   \
               : "=&v"(s02), "=&v"(d02), "=&v"(s13), "=&v"(d13)                                          \
               : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "n"(224 + 2 * Q0), "n"(225 + 2 * Q0), "n"(232 + 2 * Q0), \
                 "n"(233 + 2 * Q0), "n"(240 + 2 * Q0), "n"(241 + 2 * Q0), "n"(248 + 2 * Q0), "n"(249 + 2 * Q0))
template <bool FWD, bool ROT2, int Q0> __device__ __forceinline__ void bf4_land(cpx a0, cpx a1, cpx a2, cpx a3) {
  cpx s02, d02, s13, d13;
  if constexpr (FWD && !ROT2) CLFA_BF4_LAND(CLFA_PLUS, CLFA_MINUS, CLFA_ROTF, CLFA_ROTI);
  if constexpr (!FWD && !ROT2) CLFA_BF4_LAND(CLFA_PLUS, CLFA_MINUS, CLFA_ROTI, CLFA_ROTF);
  if constexpr (FWD && ROT2) CLFA_BF4_LAND(CLFA_ROTF, CLFA_ROTI, CLFA_ROTF, CLFA_ROTI);
  if constexpr (!FWD && ROT2) CLFA_BF4_LAND(CLFA_ROTI, CLFA_ROTF, CLFA_ROTI, CLFA_ROTF);
}
#undef CLFA_BF4_LAND
// dft16_hp whose results end in the landing registers (nothing is left in v)
template <bool FWD, class H, int P0, int P1, int P2, int P3, int P4, int P5, int P6, int P7>
__device__ __forceinline__ void dft16_hp_land(cpx (&v)[16], const H &hook) {
  bf4<FWD>(v[0], v[4], v[8], v[12]);
  hook_at<P0>(hook);
  bf4<FWD>(v[1], v[5], v[9], v[13]);
  hook_at<P1>(hook);
  bf4<FWD>(v[2], v[6], v[10], v[14]);
  hook_at<P2>(hook);
  bf4<FWD>(v[3], v[7], v[11], v[15]);
  ctw2<FWD>(v[4 + 1], kC16, kS16, v[4 + 2], kC8, kC8);
  hook_at<P3>(hook);
  ctw2<FWD>(v[4 + 3], kS16, kC16, v[8 + 1], kC8, kC8);
  ctw2<FWD>(v[8 + 3], -kC8, kC8, v[12 + 1], kS16, kC16);
  hook_at<P4>(hook);
  ctw2<FWD>(v[12 + 2], -kC8, kC8, v[12 + 3], -kC16, -kS16);
  static_assert(P4 >= 13 && P5 == 14 && P6 == 15 && P7 < 0, "landing register k is free once hook k has issued its store");
  bf4_land<FWD, false, 0>(v[0], v[1], v[2], v[3]);
  hook_at<P5>(hook);
  bf4_land<FWD, false, 1>(v[4], v[5], v[6], v[7]);
  hook_at<P6>(hook);
  bf4_land<FWD, true, 2>(v[8], v[9], v[10], v[11]);
  bf4_land<FWD, false, 3>(v[12], v[13], v[14], v[15]);
}
#define CLFA_DFT16_H(FWD, v, hook, M) \
  dft16_hp<FWD, decltype(hook), M.p[0], M.p[1], M.p[2], M.p[3], M.p[4], M.p[5], M.p[6], M.p[7]>(v, hook)
#define CLFA_DFT16_HT(FWD, v, hook, M, tail) \
  dft16_hp<FWD, decltype(hook), M.p[0], M.p[1], M.p[2], M.p[3], M.p[4], M.p[5], M.p[6], M.p[7], decltype(tail)>(v, hook, tail)

struct ResLane {
  int c, t;          // lane = c + 16 t
  int voff;          // byte offset of the lane inside a column / row block of global memory
  cpx *xa_w;         // phase-1 exchange: 16 consecutive elements written (b128)
  const cpx *xa_r;   //   ... elements 16 e apart read
  cpx *xb_w;         // phase-2 exchange
  const cpx *xb_r;
  const cpx *tw_row; // W_256^(t j), j = 0..15
  char *spill;       // lane-private LDS rows
  int slot_off;      // byte offset of the lane in one [cb] row of the workgroup's global slot
};

// second pass of a block: inputs times W_256^(t j) (row t of the table); hooks H0 .. H0 + 3 after the four groups
// AHEAD: the twiddle rows are read one group (two b128) ahead of their use: the hook points are scheduling fences, and a
// read issued right before its use costs one wave per SIMD the whole LDS latency, three times per block
// (profiles/ab_res16_lds_r05.txt)
template <bool FWD, int H0, bool AHEAD, class H> __device__ __forceinline__ void res_tw_rows(cpx (&v)[16], const ResLane &L, const H &hook) {
  const f4 *pt = reinterpret_cast<const f4 *>(L.tw_row);
  if constexpr (AHEAD) {
    f4 wa = pt[0], wb = pt[1], na = pt[2], nb = pt[3];
    static_for<4>([&](auto G) {
      constexpr int g = decltype(G)::value;
      if constexpr (g == 0) v[1] = cmulc<!FWD>(v[1], mk(wa.z, wa.w));
      else cmulc2<!FWD>(v[4 * g], v[4 * g + 1], v[4 * g], mk(wa.x, wa.y), v[4 * g + 1], mk(wa.z, wa.w));
      cmulc2<!FWD>(v[4 * g + 2], v[4 * g + 3], v[4 * g + 2], mk(wb.x, wb.y), v[4 * g + 3], mk(wb.z, wb.w));
      wa = na;
      wb = nb;
      if constexpr (g < 2) {   // the group after next, issued ahead of the fence
        na = pt[2 * g + 4];
        nb = pt[2 * g + 5];
      }
      hook_at<H0 + g>(hook);
    });
  } else {
    {
      const f4 w = pt[0];
      v[1] = cmulc<!FWD>(v[1], mk(w.z, w.w));
    }
#pragma unroll
    for (int i = 1; i < 8; i++) {
      const f4 w = pt[i];
      cmulc2<!FWD>(v[2 * i], v[2 * i + 1], v[2 * i], mk(w.x, w.y), v[2 * i + 1], mk(w.z, w.w));
      if (i == 1) hook_at<H0>(hook);
      if (i == 3) hook_at<H0 + 1>(hook);
      if (i == 5) hook_at<H0 + 2>(hook);
      if (i == 7) hook_at<H0 + 3>(hook);
    }
  }
}

// ---- phase 1: one column block ------------------------------------------------------------------
// v: rows t + 16 e of column n2 = 16 cb + c (already loaded) -> o[e] = Z[t + 16 e][n2]
template <bool FWD, class H = HookNone>
__device__ __forceinline__ void res_col_block(cpx (&v)[16], const ResLane &L, int cb, const cpx *s_tab, cpx *s_x,
                                              const H &hook = H()) {
  CLFA_DFT16_H(FWD, v, hook, kMapColA);
  __syncthreads();   // the previous block's readers are done with the exchange buffer
  {
    f4 *pw = reinterpret_cast<f4 *>(L.xa_w);
#pragma unroll
    for (int i = 0; i < 8; i++) pw[i] = pack2(v[2 * i], v[2 * i + 1]);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = L.xa_r[16 * e];
  // second pass: inputs times W_256^(t j) (row t of the table), then the butterflies
  res_tw_rows<FWD, 4, true>(v, L, hook);
  // four-step twiddles W_N^(n2 (t + 16 e)) = b * s^e,  b = W_N^(n2 t),  s = W_4096^n2
  const int n2 = cb * 16 + L.c;
  const int m = n2 * L.t;   // < 4096
  const cpx *ps = s_tab + kTabS + n2;
  cpx blo, bhi, s1, s2, s4, s8;
  auto lookups = [&]() {
    blo = s_tab[kTabLo + (m & 255)], bhi = s_tab[kTabHi + (m >> 8)];
    s1 = ps[0], s2 = ps[256], s4 = ps[512], s8 = ps[768];
  };
  // the six reads go out ahead of the pass's last two butterflies (a fence keeps them there; -0.25 %,
  // profiles/ab_res16_lds_r05.txt)
  auto tail = [&]() {
    lookups();
    __builtin_amdgcn_sched_barrier(0);
  };
  CLFA_DFT16_HT(FWD, v, hook, kMapColB, tail);
  const cpx b = cmul(blo, bhi);
  // product tree in halves of four (T_r = b s^r, U_r = T_r s^8), two products per statement
  cpx T[4], U[4];
  T[0] = b;
  cmulc2(T[1], T[2], b, s1, b, s2);
  cmulc2(T[3], U[0], T[1], s2, b, s8);
  hook_at<12>(hook);
  cmulc2(U[1], U[2], T[1], s8, T[2], s8);
  U[3] = cmul(T[3], s8);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    cmulc2<!FWD>(v[r], v[r + 8], v[r], T[r], v[r + 8], U[r]);
    if (r == 1) hook_at<13>(hook);
  }
  cmulc2(T[0], T[1], T[0], s4, T[1], s4);
  cmulc2(T[2], T[3], T[2], s4, T[3], s4);
  hook_at<14>(hook);
  cmulc2(U[0], U[1], T[0], s8, T[1], s8);
  cmulc2(U[2], U[3], T[2], s8, T[3], s8);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    cmulc2<!FWD>(v[r + 4], v[r + 12], v[r + 4], T[r], v[r + 12], U[r]);
    if (r == 1) hook_at<15>(hook);
  }
}

// o[e] -> keep[e][cb]
// LAST (column block 15): the slot's element goes straight to its landing register (the rest of that row
// block is on its way there, HookSlot)
template <bool LAST = false, bool INV = false>
__device__ __forceinline__ void res_deposit(const cpx (&o)[16], const ResLane &L, int cb, f32x32 (&K)[kVgprBlk],
                                            __amdgpu_buffer_rsrc_t slot) {
  {
    cpx *ps = reinterpret_cast<cpx *>(L.spill + cb * 8);
#pragma unroll
    for (int e = 0; e < kLdsBlk; e++) ps[e * 16] = o[e];
  }
  // the one row block that does not fit the CU: [cb][lane] in the workgroup's 32 KiB slot (L2-resident)
  if constexpr (LAST) res_stage_one15(o[kLdsBlk]);
  else
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o[kLdsBlk]), slot, L.slot_off, cb * 2048, 0);
#pragma unroll
  for (int j = 0; j < kVgprBlk; j++) {
    K[j][2 * cb] = o[kVgprFirst + j].x;
    K[j][2 * cb + 1] = o[kVgprFirst + j].y;
  }
  using S8 = std::make_integer_sequence<int, kAgprBlk>;
  switch (cb) {
#define CLFA_C(c) case c: acc_deposit<c, INV>(o, S8()); break;
    CLFA_C(0) CLFA_C(1) CLFA_C(2) CLFA_C(3) CLFA_C(4) CLFA_C(5) CLFA_C(6) CLFA_C(7)
    CLFA_C(8) CLFA_C(9) CLFA_C(10) CLFA_C(11) CLFA_C(12) CLFA_C(13) CLFA_C(14)
#undef CLFA_C
    default: acc_deposit<15, INV>(o, S8()); break;
  }
}

// keep[rb][e] -> v[e]
template <int RB, bool INV = false> __device__ __forceinline__ void res_fetch_static(cpx (&v)[16], const ResLane &L, const f32x32 (&K)[kVgprBlk]) {
  if constexpr (RB < kLdsBlk) {
    const f4 *pf = reinterpret_cast<const f4 *>(L.spill + RB * 128);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const f4 w = pf[i];
      v[2 * i] = mk(w.x, w.y);
      v[2 * i + 1] = mk(w.z, w.w);
    }
  } else if constexpr (RB < kVgprFirst) {
    static_assert(RB >= kVgprFirst || RB < kLdsBlk, "the global slot's block is fetched by res_slot_load");
  } else if constexpr (RB < kAgprFirst) {
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = mk(K[RB - kVgprFirst][2 * e], K[RB - kVgprFirst][2 * e + 1]);
  } else {
    acc_fetch<RB - kAgprFirst, INV>(v, std::make_integer_sequence<int, 16>());
  }
}
// ---- phase 2: one row block ---------------------------------------------------------------------
// v[e] = Z[16 rb + t][c + 16 e] -> X[16 rb + c + 256 (t + 16 e)] left in v[e] (lane = row c, k2 = t + 16 e)
// LAND: the results go straight into the landing registers (dft16_hp_land) instead of v
// TWA: the twiddle rows read a group ahead (res_tw_rows; the packed real forward kernel has no registers for it)
template <bool FWD, bool LAND = false, bool TWA = true, class H = HookNone>
__device__ __forceinline__ void res_row_block(cpx (&v)[16], const ResLane &L, const H &hook = H()) {
  CLFA_DFT16_H(FWD, v, hook, kMapRowC);
  __syncthreads();
  {
    f4 *pw = reinterpret_cast<f4 *>(L.xb_w);
#pragma unroll
    for (int i = 0; i < 8; i++) pw[i] = pack2(v[2 * i], v[2 * i + 1]);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = L.xb_r[18 * e];
  res_tw_rows<FWD, 6, TWA>(v, L, hook);
  if constexpr (LAND) dft16_hp_land<FWD, H, kMapRowD.p[0], kMapRowD.p[1], kMapRowD.p[2], kMapRowD.p[3], kMapRowD.p[4], kMapRowD.p[5], kMapRowD.p[6], kMapRowD.p[7]>(v, hook);
  else CLFA_DFT16_H(FWD, v, hook, kMapRowD);
}

// phase 1, one column block: wait for its data (N younger asm loads), take it out of its landing zone
// (ZC >= 0: AGPR columns ZC, ZC + 1; ZC < 0: v[224:255]), transform it with the loads of the block two
// ahead riding along (-> AGPR columns NZ, NZ + 1, or the landing registers for NZ < 0; none if !LOAD)
// draw: the shared assignment's step (res_draw_step), behind the wait and ahead of the block's hooked loads
template <bool FWD, int ZC, int NZ, bool LOAD, int N = 16, bool LAST = false, class DS = NoTail>
__device__ __forceinline__ void res_phase1_block(cpx (&v)[16], const ResLane &L, const cpx *x, int cb,
                                                 const int (&so)[16], f32x32 (&K)[kVgprBlk], __amdgpu_buffer_rsrc_t slot,
                                                 const cpx *s_tab, cpx *s_x, const DS &draw = DS()) {
  res_wait_vm<N>();
  if constexpr (ZC >= 0) acc_fetch_raw<ZC>(v, std::make_integer_sequence<int, 8>());
  else res_land_fetch(v);
  draw();
  if constexpr (LOAD) {
    const __amdgpu_buffer_rsrc_t r = res_rsrc(x + (cb + 2) * 16);
    if constexpr (NZ >= 0) res_col_block<FWD>(v, L, cb, s_tab, s_x, HookAcc<NZ>{r, L.voff, so});
    else res_col_block<FWD>(v, L, cb, s_tab, s_x, HookLand{r, L.voff, so});
  } else if constexpr (LAST) {
    res_col_block<FWD>(v, L, cb, s_tab, s_x, HookSlot{slot, L.slot_off, so});
  } else {
    res_col_block<FWD>(v, L, cb, s_tab, s_x);
  }
  res_deposit<LAST>(v, L, cb, K, slot);
}

}  // namespace
}  // namespace clfa
