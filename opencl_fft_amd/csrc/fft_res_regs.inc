// fft_res_regs.inc (part of the translation unit fft_resident.hip) — the register files and the memory accesses of
// k_fft_res16 that hipcc does not manage: the AGPR file addressed by literal register numbers, the landing registers
// v[224:255], the global loads / stores issued from inline asm with their explicit waits, and the hook structs that
// issue one such access per hook point.

namespace clfa {
namespace {

// cache policy of the streams (tuning switches for A/B builds; the library's choice is the default):
// CLFA_LDNT / CLFA_STNT = the modifier string of the asm accesses, CLFA_ST_AUX = the same policy as the aux
// operand of the store builtin (bit 0 sc0, bit 1 nt, bit 4 sc1)
#ifndef CLFA_LDNT
#define CLFA_LDNT " nt"
#endif
#ifndef CLFA_STNT
#define CLFA_STNT " nt"
#define CLFA_ST_AUX 2
#endif
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int kN = 65536;
// row blocks per storage class, in this order: rb 0..2 LDS, rb 3 global slot, rb 4..7 VGPR, rb 8..15 AGPR
constexpr int kLdsBlk = 3, kGlbBlk = 1, kVgprBlk = 4, kAgprBlk = 8;
constexpr int kVgprFirst = kLdsBlk + kGlbBlk, kAgprFirst = kVgprFirst + kVgprBlk;
static_assert(kAgprFirst + kAgprBlk == 16, "16 row blocks");

// ---- AGPR file, addressed by literal register numbers ------------------------------------------
template <int I> __device__ __forceinline__ void acc_write(float v) {
  asm volatile("v_accvgpr_write_b32 a[%0], %1" ::"n"(I), "v"(v));
}
template <int I> __device__ __forceinline__ float acc_read() {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(v) : "n"(I));
  return v;
}
// the kernel's descriptor has to allocate all 256 AGPRs: name them as clobbered once
#define CLFA_A10(p) "a" #p "0", "a" #p "1", "a" #p "2", "a" #p "3", "a" #p "4", "a" #p "5", "a" #p "6", "a" #p "7", "a" #p "8", "a" #p "9"
__device__ __forceinline__ void acc_claim_all() {
  asm volatile("" ::: "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", CLFA_A10(1), CLFA_A10(2), CLFA_A10(3),
               CLFA_A10(4), CLFA_A10(5), CLFA_A10(6), CLFA_A10(7), CLFA_A10(8), CLFA_A10(9), CLFA_A10(10), CLFA_A10(11),
               CLFA_A10(12), CLFA_A10(13), CLFA_A10(14), CLFA_A10(15), CLFA_A10(16), CLFA_A10(17), CLFA_A10(18),
               CLFA_A10(19), CLFA_A10(20), CLFA_A10(21), CLFA_A10(22), CLFA_A10(23), CLFA_A10(24), "a250", "a251", "a252",
               "a253", "a254", "a255",
               // ... and the landing registers v[224:255] (kept out of hipcc's hands by amdgpu_num_vgpr(224))
               "v224", "v225", "v226", "v227", "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237",
               "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251",
               "v252", "v253", "v254", "v255");
}
#undef CLFA_A10
// Two AGPR column pairs double as landing zones for the even column blocks' loads while they are
// still empty: Z0 = columns 14, 15 (blocks 0, 4, 8, 12), Z1 = columns 12, 13 (blocks 2, 6, 10, 14).
// They fall free in the order Z0 (block 12 taken out), Z1 (block 14 taken out), so the keep matrix's
// columns 12..15 are stored swapped: logical column c lives in physical column acc_col(c).
constexpr int kZone0 = 14, kZone1 = 12;
// INV (the packed real inverse kernel, whose phase 1 takes the column blocks in the order 7, 8, 6, 9, ... 0, 15): the
// zones are the columns of the blocks deposited last there — Z0 = blocks 0, 15, Z1 = blocks 1, 14
template <bool INV = false> constexpr int acc_col(int c) {
  if (INV) return c == 0 ? 14 : c == 15 ? 15 : c == 1 ? 12 : c == 14 ? 13 : c - 2;
  return c < 12 ? c : c ^ 2;
}
// column block CB: element e = 8 + J of the lane's results goes to a[32 J + 2 acc_col(CB)]
template <int CB, bool INV, int... J> __device__ __forceinline__ void acc_deposit(const cpx (&o)[16], std::integer_sequence<int, J...>) {
  ((acc_write<32 * J + 2 * acc_col<INV>(CB)>(o[kAgprFirst + J].x), acc_write<32 * J + 2 * acc_col<INV>(CB) + 1>(o[kAgprFirst + J].y)), ...);
}
// row block 8 + RB: a[32 RB + 2 acc_col(e)] -> v[e]
template <int RB, bool INV, int... E> __device__ __forceinline__ void acc_fetch(cpx (&v)[16], std::integer_sequence<int, E...>) {
  ((v[E].x = acc_read<32 * RB + 2 * acc_col<INV>(E)>(), v[E].y = acc_read<32 * RB + 2 * acc_col<INV>(E) + 1>()), ...);
}

// ---- global accesses ----------------------------------------------------------------------------
// raw buffer descriptor over one transform (base wave-uniform: it stays in SGPRs)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t res_rsrc(const cpx *base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<cpx *>(base), 0, 0x7fffffff, 0x00020000);
}
// 16 rows 16 apart (32 KiB), lane offset `voff` bytes; non-temporal (aux 2)
__device__ __forceinline__ void res_store(const cpx (&v)[16], __amdgpu_buffer_rsrc_t r, int voff) {
#pragma unroll
  for (int e = 0; e < 16; e++)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v[e]), r, voff, e * 32768, CLFA_ST_AUX);
}

// ---- loads the compiler does not see ---------------------------------------------------------------
// Phase 1 keeps TWO column blocks in flight (64 KiB per CU: one block ahead is latency-bound, see
// DESIGN.md), and there are no 32 spare VGPRs for the second one.  It lands in the accumulation
// registers of the keep matrix's columns cb and cb + 1, which are still empty while block cb waits
// (rows e < 8 -> a[32 e + 2 cb], rows e >= 8 -> a[32 (e - 8) + 2 (cb + 1)]); blocks with odd cb land
// in reserved VGPRs (below).  hipcc counts neither kind (all are asm), so the waits are explicit: s_waitcnt vmcnt(N) with
// N = the asm loads issued after the awaited ones (compiler-issued stores in between only make the
// wait stronger).  The s_nop 4 covers SALU-written descriptor / offset SGPRs read by VMEM.
template <int COL, int E0> __device__ __forceinline__ void res_load_acc8(__amdgpu_buffer_rsrc_t r, int voff) {
  asm volatile("s_nop 4\n\t"
               "buffer_load_dwordx2 a[%c2:%c3], %0, %1, %18 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c4:%c5], %0, %1, %19 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c6:%c7], %0, %1, %20 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c8:%c9], %0, %1, %21 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c10:%c11], %0, %1, %22 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c12:%c13], %0, %1, %23 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c14:%c15], %0, %1, %24 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 a[%c16:%c17], %0, %1, %25 offen" CLFA_LDNT
               :
               : "v"(voff), "s"(r), "n"(0 * 32 + 2 * COL), "n"(0 * 32 + 2 * COL + 1), "n"(1 * 32 + 2 * COL),
                 "n"(1 * 32 + 2 * COL + 1), "n"(2 * 32 + 2 * COL), "n"(2 * 32 + 2 * COL + 1), "n"(3 * 32 + 2 * COL),
                 "n"(3 * 32 + 2 * COL + 1), "n"(4 * 32 + 2 * COL), "n"(4 * 32 + 2 * COL + 1), "n"(5 * 32 + 2 * COL),
                 "n"(5 * 32 + 2 * COL + 1), "n"(6 * 32 + 2 * COL), "n"(6 * 32 + 2 * COL + 1), "n"(7 * 32 + 2 * COL),
                 "n"(7 * 32 + 2 * COL + 1), "s"((E0 + 0) * 32768), "s"((E0 + 1) * 32768), "s"((E0 + 2) * 32768),
                 "s"((E0 + 3) * 32768), "s"((E0 + 4) * 32768), "s"((E0 + 5) * 32768), "s"((E0 + 6) * 32768),
                 "s"((E0 + 7) * 32768)
               : "memory");
}
// one column block (at `base`) -> AGPR columns ZC, ZC + 1, all 16 loads at once
template <int ZC> __device__ __forceinline__ void res_load_acc(const cpx *base, int voff) {
  const __amdgpu_buffer_rsrc_t r = res_rsrc(base);
  res_load_acc8<ZC, 0>(r, voff);
  res_load_acc8<ZC + 1, 8>(r, voff);
}
// ... and back out, once its wait has passed
template <int CB, int... E> __device__ __forceinline__ void acc_fetch_raw(cpx (&v)[16], std::integer_sequence<int, E...>) {
  ((v[E].x = acc_read<32 * E + 2 * CB>(), v[E].y = acc_read<32 * E + 2 * CB + 1>()), ...);
  ((v[8 + E].x = acc_read<32 * E + 2 * CB + 2>(), v[8 + E].y = acc_read<32 * E + 2 * CB + 3>()), ...);
}
// Blocks with odd cb land in v[224:255].  The kernel is compiled with amdgpu_num_vgpr(224), so hipcc
// allocates v0..v223 only and never reads, copies or spills a register with a load still pending on it
// (with compiler-allocated destinations it did: it moved them ahead of the wait).
template <int E0> __device__ __forceinline__ void res_load_land8(__amdgpu_buffer_rsrc_t r, int voff) {
  asm volatile("s_nop 4\n\t"
               "buffer_load_dwordx2 v[%c2:%c3], %0, %1, %18 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c4:%c5], %0, %1, %19 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c6:%c7], %0, %1, %20 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c8:%c9], %0, %1, %21 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c10:%c11], %0, %1, %22 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c12:%c13], %0, %1, %23 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c14:%c15], %0, %1, %24 offen" CLFA_LDNT "\n\t"
               "buffer_load_dwordx2 v[%c16:%c17], %0, %1, %25 offen" CLFA_LDNT
               :
               : "v"(voff), "s"(r), "n"(224 + 2 * E0), "n"(225 + 2 * E0), "n"(226 + 2 * E0), "n"(227 + 2 * E0),
                 "n"(228 + 2 * E0), "n"(229 + 2 * E0), "n"(230 + 2 * E0), "n"(231 + 2 * E0), "n"(232 + 2 * E0),
                 "n"(233 + 2 * E0), "n"(234 + 2 * E0), "n"(235 + 2 * E0), "n"(236 + 2 * E0), "n"(237 + 2 * E0),
                 "n"(238 + 2 * E0), "n"(239 + 2 * E0), "s"((E0 + 0) * 32768), "s"((E0 + 1) * 32768),
                 "s"((E0 + 2) * 32768), "s"((E0 + 3) * 32768), "s"((E0 + 4) * 32768), "s"((E0 + 5) * 32768),
                 "s"((E0 + 6) * 32768), "s"((E0 + 7) * 32768)
               : "memory");
}
__device__ __forceinline__ void res_load_land(const cpx *base, int voff) {
  const __amdgpu_buffer_rsrc_t r = res_rsrc(base);
  res_load_land8<0>(r, voff);
  res_load_land8<8>(r, voff);
}
// ... and out of the landing registers (after the wait)
__device__ __forceinline__ void res_land_fetch(cpx (&v)[16]) {
  asm volatile("v_mov_b64 %0, v[224:225]\n\tv_mov_b64 %1, v[226:227]\n\tv_mov_b64 %2, v[228:229]\n\tv_mov_b64 %3, v[230:231]\n\t"
               "v_mov_b64 %4, v[232:233]\n\tv_mov_b64 %5, v[234:235]\n\tv_mov_b64 %6, v[236:237]\n\tv_mov_b64 %7, v[238:239]"
               : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]), "=v"(v[4]), "=v"(v[5]), "=v"(v[6]), "=v"(v[7]));
  asm volatile("v_mov_b64 %0, v[240:241]\n\tv_mov_b64 %1, v[242:243]\n\tv_mov_b64 %2, v[244:245]\n\tv_mov_b64 %3, v[246:247]\n\t"
               "v_mov_b64 %4, v[248:249]\n\tv_mov_b64 %5, v[250:251]\n\tv_mov_b64 %6, v[252:253]\n\tv_mov_b64 %7, v[254:255]"
               : "=v"(v[8]), "=v"(v[9]), "=v"(v[10]), "=v"(v[11]), "=v"(v[12]), "=v"(v[13]), "=v"(v[14]), "=v"(v[15]));
}
// waits for the asm loads: N = the asm loads issued after the awaited ones
template <int N> __device__ __forceinline__ void res_wait_vm() {
  static_assert(N == 0 || N == 1 || N == 2 || N == 16 || N == 32 || N == 48, "");
  if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  if constexpr (N == 48) asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  if constexpr (N == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
}

// ---- the shared assignment's draws (k_fft_res16<..., DYN>) -------------------------------------------------------------
// One returning add of 1 on a word of the plan's counters (agent scope: the form hipcc emits for a relaxed
// __hip_atomic_fetch_add, executed at the memory side), issued by ONE lane of wave 0.  Like the loads it must land where
// hipcc never looks while it is pending: in the first register of an AGPR landing zone that is empty for this and the next
// column block (REG = a[2 * zone column]: the block that took its data out of the zone issues into the first column, the
// block after it into the second; the zone's next loads are hooked to the block after that).  It is issued behind the
// block's wait and ahead of its 16 hooked loads, so the next block's vmcnt(16) covers it and no count changes.
template <int REG> __device__ __forceinline__ void res_draw_issue(unsigned *ctr, int byte_off) {
  asm volatile("v_accvgpr_write_b32 a[%c0], 1\n\ts_nop 4\n\tglobal_atomic_add a[%c0], %1, a[%c0], %2 sc0" ::"n"(REG), "v"(byte_off), "s"(ctr) : "memory");
}
// the counters: one per XCD and the launch's count of workgroups that have drawn for the last time, 128 bytes apart
constexpr int kDrawStride = 128, kDrawDone = 8;
// The steps' state is uniform, but hipcc does not see that: said so (readfirstlane), it stays in scalar registers — as
// three VGPRs more the keep matrix no longer fits.  Scalar registers are as short: the two small fields share one, and
// what a step derives from the grid and the batch is worked out again in every step (opaque copies) instead of being
// carried round the transform's loop.
__device__ __forceinline__ int res_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
struct ResDraw {   // wave 0's
  int st;    // kk + 16 (dk + 1): kk = the next draw's place in the rotation (0 = the XCD's own counter, k = that of XCD
             // x + k, 8 = none left), dk = the pending draw's place (kDrawDone: the arrival at the launch's end, -1: none)
  int nxt;   // the next transform, -1 = none yet
};
// One step of wave 0, behind column block cb's wait: take the draw issued a block ago out of a[RP], issue the next into
// a[RC].  A draw beyond the XCD's share moves on to the other XCDs' counters, one draw each in a fixed rotation that
// goes on where the previous transform's steps stopped: at most 8 draws per transform (blocks 0..7), nothing waits for
// another workgroup.  Block 8 posts the outcome for the other waves (read in phase 2, many barriers later) and, when
// nothing is left, counts the workgroup as done; the workgroup that arrives last (block 9) returns the nine words to
// zero for the next launch — no workgroup can draw after every one of them has given up.
template <int RP, int RC>
__device__ __forceinline__ void res_draw_step(ResDraw &D, int cb, unsigned *ctr, unsigned grid, unsigned batch, int tid, int *s_next) {
  asm volatile("" : "+s"(grid), "+s"(batch));
  const unsigned x = blockIdx.x & 7;
  int kk = D.st & 15;
  const int dk = (D.st >> 4) - 1;
  int pend = -1;
  if (dk >= 0) {
    const unsigned d = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, acc_read<RP>()));
    if (dk < kDrawDone) {
      // the first G / 8 positions of every XCD are the workgroups' first transforms (xcd_first): the counters start behind them
      const unsigned xs = (x + dk) & 7, p = d + (grid >> 3);
      const bool hit = p < xcd_share(xs, grid, batch);
      if (hit) D.nxt = res_uniform((int)xcd_transform(xs, grid, p));
      // On purpose, not left-over rotation state: only the XCD's own counter is drawn from again after a hit.  A hit on
      // another XCD's counter moves on as a miss does — at most one draw per other XCD in a workgroup's life, which bounds
      // every path and keeps the stolen tail to about one transform per workgroup (profiles/res16_balance.txt, section 1).
      kk = hit && dk == 0 ? 0 : dk + 1;
    } else if (d == grid - 1 && tid <= kDrawDone) {
      // (a zero of its own: one shared with the keep matrix's initial zeros hipcc keeps in a[0:31] for the whole kernel)
      unsigned zero = 0;
      asm volatile("" : "+v"(zero));
      __hip_atomic_store(ctr + tid * (kDrawStride / 4), zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (cb < 8) {
    if (D.nxt < 0 && kk < 8) {
      if (tid == 0) res_draw_issue<RC>(ctr, (int)(((x + kk) & 7) * kDrawStride));
      pend = kk;
    }
  } else if (cb == 8) {
    if (tid == 0) *s_next = D.nxt;
    if (D.nxt < 0) {
      if (tid == 0) res_draw_issue<RC>(ctr, kDrawDone * kDrawStride);
      pend = kDrawDone;
    }
  }
  D.st = res_uniform(kk + 16 * (pend + 1));
}

// ---- loads interleaved with the arithmetic ---------------------------------------------------------
// One wave per SIMD cannot afford to issue a block's 16 loads back to back: with the memory pipeline
// saturated every load instruction then waits ~80 cycles for a queue slot, and nothing else runs on
// that SIMD meanwhile (measured: the loads cost the same whether or not anything waits for their
// data, profiles/res16_probe_r02.txt).  So a column block's code has 16 hook points, ~20 instructions
// apart, and each issues ONE load of the block two ahead.  so[e] = e * 32 KiB, pinned in SGPRs.
template <int K> using ic = std::integral_constant<int, K>;
template <int... I, class F> __device__ __forceinline__ void static_for_(std::integer_sequence<int, I...>, F &&f) { (f(ic<I>()), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F &&f) { static_for_(std::make_integer_sequence<int, N>(), f); }
struct HookNone {
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {}
};
// KEEP: a plain (cached) load instead of the streaming one — the mirrored loads of the packed real inverse kernel touch
// every line twice, one pair apart (15 of its 16 columns, then the last), and the second touch should find it in L2
template <int CB, bool KEEP = false> struct HookAcc {   // -> AGPR columns CB, CB + 1 (a landing zone)
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
    constexpr int lo = 32 * (K & 7) + 2 * (K < 8 ? CB : CB + 1);
    // K == 0: the descriptor's SGPRs may be fresh from SALU — 5 wait states before VMEM reads them, in the SAME asm
    // statement as the load (between two statements hipcc may re-materialise the descriptor)
#define CLFA_LD_ACC(PRE, POL) \
  asm volatile(PRE "buffer_load_dwordx2 a[%c2:%c3], %0, %1, %4 offen" POL ::"v"(voff), "s"(r), "n"(lo), "n"(lo + 1), "s"(so[K]) : "memory")
    if constexpr (K == 0 && KEEP) CLFA_LD_ACC("s_nop 4\n\t", "");
    else if constexpr (K == 0) CLFA_LD_ACC("s_nop 4\n\t", CLFA_LDNT);
    else if constexpr (KEEP) CLFA_LD_ACC("", "");
    else CLFA_LD_ACC("", CLFA_LDNT);
#undef CLFA_LD_ACC
  }
};
template <bool KEEP = false> struct HookLandT {   // -> landing registers v[224:255]
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
#define CLFA_LD_LAND(PRE, POL) \
  asm volatile(PRE "buffer_load_dwordx2 v[%c2:%c3], %0, %1, %4 offen" POL ::"v"(voff), "s"(r), "n"(224 + 2 * K), "n"(225 + 2 * K), "s"(so[K]) : "memory")
    if constexpr (K == 0 && KEEP) CLFA_LD_LAND("s_nop 4\n\t", "");
    else if constexpr (K == 0) CLFA_LD_LAND("s_nop 4\n\t", CLFA_LDNT);
    else if constexpr (KEEP) CLFA_LD_LAND("", "");
    else CLFA_LD_LAND("", CLFA_LDNT);
#undef CLFA_LD_LAND
  }
};
using HookLand = HookLandT<false>;
// block 15 of phase 1 has nothing left to prefetch: its hooks bring the global slot's row block back
// (columns 0..14; column 15 is still in the lane's registers then) into v[224:253]; agent scope (sc1): the
// loads bypass this CU's L1, which may still hold the previous transform's lines
struct HookSlot {
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
    if constexpr (K < 15) {
      int off;
      asm volatile("s_lshr_b32 %0, %3, 4\n\ts_nop 4\n\tbuffer_load_dwordx2 v[%c4:%c5], %1, %2, %0 offen sc1"
                   : "=&s"(off)
                   : "v"(voff), "s"(r), "s"(so[K]), "n"(224 + 2 * K), "n"(225 + 2 * K)
                   : "memory", "scc");
    }
  }
};
// phase 2: a row block's 16 stores ride along the NEXT block's arithmetic, out of the landing registers
// (idle in phase 2), where res_stage() has put the block's results
struct HookStore {
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
    if constexpr (K == 0)
      asm volatile("s_nop 4\n\tbuffer_store_dwordx2 v[%c2:%c3], %0, %1, %4 offen" CLFA_STNT ::"v"(voff), "s"(r), "n"(224 + 2 * K), "n"(225 + 2 * K), "s"(so[K]) : "memory");
    else
      asm volatile("buffer_store_dwordx2 v[%c2:%c3], %0, %1, %4 offen" CLFA_STNT ::"v"(voff), "s"(r), "n"(224 + 2 * K), "n"(225 + 2 * K), "s"(so[K]) : "memory");
  }
};
__device__ __forceinline__ void res_stage(const cpx (&v)[16]) {
  asm volatile("v_mov_b64 v[224:225], %0\n\tv_mov_b64 v[226:227], %1\n\tv_mov_b64 v[228:229], %2\n\tv_mov_b64 v[230:231], %3\n\t"
               "v_mov_b64 v[232:233], %4\n\tv_mov_b64 v[234:235], %5\n\tv_mov_b64 v[236:237], %6\n\tv_mov_b64 v[238:239], %7"
               ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
  asm volatile("v_mov_b64 v[240:241], %0\n\tv_mov_b64 v[242:243], %1\n\tv_mov_b64 v[244:245], %2\n\tv_mov_b64 v[246:247], %3\n\t"
               "v_mov_b64 v[248:249], %4\n\tv_mov_b64 v[250:251], %5\n\tv_mov_b64 v[252:253], %6\n\tv_mov_b64 v[254:255], %7"
               ::"v"(v[8]), "v"(v[9]), "v"(v[10]), "v"(v[11]), "v"(v[12]), "v"(v[13]), "v"(v[14]), "v"(v[15]));
}
__device__ __forceinline__ void res_stage_one15(cpx o) { asm volatile("v_mov_b64 v[254:255], %0" ::"v"(o)); }
// a hook stays where it is written: without the fences hipcc lets the arithmetic drift around the asm
// statements and the loads end up in clusters of four
template <int G, class H> __device__ __forceinline__ void hook_at(const H &hook) {
  if constexpr (G >= 0 && !std::is_same<H, HookNone>::value) {
    __builtin_amdgcn_sched_barrier(0);
    hook(ic<G>());
    __builtin_amdgcn_sched_barrier(0);
  }
}
template <class H> __device__ __forceinline__ void res_issue_all(const H &h) {
  static_for<16>([&](auto Kc) { h(Kc); });
}
// a whole 16-register row of the AGPR file, a[BASE ...], as one block (the packed real forward kernel parks blocks there)
template <int BASE> __device__ __forceinline__ void acc_fetch_flat(cpx (&v)[16]) {
  static_for<16>([&](auto E) { v[decltype(E)::value] = mk(acc_read<BASE + 2 * decltype(E)::value>(), acc_read<BASE + 2 * decltype(E)::value + 1>()); });
}
template <int BASE> __device__ __forceinline__ void acc_park_flat(const cpx (&v)[16]) {
  static_for<16>([&](auto E) { acc_write<BASE + 2 * decltype(E)::value>(v[decltype(E)::value].x); acc_write<BASE + 2 * decltype(E)::value + 1>(v[decltype(E)::value].y); });
}
template <int BASE> struct HookStoreAcc {   // stores out of a[BASE ...] (a parked block)
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
    if constexpr (K == 0)
      asm volatile("s_nop 4\n\tbuffer_store_dwordx2 a[%c2:%c3], %0, %1, %4 offen" CLFA_STNT ::"v"(voff), "s"(r), "n"(BASE + 2 * K), "n"(BASE + 1 + 2 * K), "s"(so[K]) : "memory");
    else
      asm volatile("buffer_store_dwordx2 a[%c2:%c3], %0, %1, %4 offen" CLFA_STNT ::"v"(voff), "s"(r), "n"(BASE + 2 * K), "n"(BASE + 1 + 2 * K), "s"(so[K]) : "memory");
  }
};
template <int BASE> struct HookSlotAcc {   // the global slot's row block (all 16 columns) -> a[BASE ...]; sc1 as in HookSlot
  __amdgpu_buffer_rsrc_t r;
  int voff;
  const int (&so)[16];
  template <int K> __device__ __forceinline__ void operator()(ic<K>) const {
    int off;
    asm volatile("s_lshr_b32 %0, %3, 4\n\ts_nop 4\n\tbuffer_load_dwordx2 a[%c4:%c5], %1, %2, %0 offen sc1"
                 : "=&s"(off)
                 : "v"(voff), "s"(r), "s"(so[K]), "n"(BASE + 2 * K), "n"(BASE + 1 + 2 * K)
                 : "memory", "scc");
  }
};
template <class A, class B> struct Hook2 {
  A a;
  B b;
  template <int K> __device__ __forceinline__ void operator()(ic<K> k) const {
    a(k);
    b(k);
  }
};
// all 16 stores of the landing registers at once (the last A' block of a transform)
__device__ __forceinline__ void res_store_land(__amdgpu_buffer_rsrc_t r, int voff, const int (&so)[16]) {
  res_issue_all(HookStore{r, voff, so});
}
// a block's 16 stores out of compiler registers, with the pinned row offsets (the builtin of res_store() would make
// hipcc hold a second copy of the 15 offsets in SGPRs, which this variant of the kernel does not have)
__device__ __forceinline__ void res_store_so(const cpx (&v)[16], __amdgpu_buffer_rsrc_t r, int voff, const int (&so)[16]) {
  // (the descriptor's SGPRs may be fresh from SALU: the wait states sit in the first store's own statement)
  asm volatile("s_nop 4\n\tbuffer_store_dwordx2 %0, %1, %2, %3 offen" CLFA_STNT ::"v"(v[0]), "v"(voff), "s"(r), "s"(so[0]) : "memory");
#pragma unroll
  for (int e = 1; e < 16; e++)
    asm volatile("buffer_store_dwordx2 %0, %1, %2, %3 offen" CLFA_STNT ::"v"(v[e]), "v"(voff), "s"(r), "s"(so[e]) : "memory");
}

}  // namespace
}  // namespace clfa
