// fft_resident.hip — n = 65536 complex in one HBM pass: the intermediate of the four-step transform
// stays on the compute unit.
//
// Replaces the reference's reorder + 16 stage launches for N = 65536 (cl_fft.cpp:24-41, 138-151).
//
// The transform is N1 x N2 = 256 x 256 (four-step): phase 1 = 256-point FFTs down the columns of the
// row-major input times W_N^(n2 k1), phase 2 = 256-point FFTs along the rows, stored transposed
// (X[k1 + 256 k2]).  512 KiB per transform do not fit the 160 KiB of LDS — but they (almost) fit the
// compute unit: ONE 256-lane workgroup per CU (one wave per SIMD) owns the whole 512-entry register
// file of every lane (256 arch VGPRs + 256 accumulation VGPRs).
//
// Lane l = c + 16 t.  Phase 1, column block cb (16 columns, 128-byte row segments): the lane takes
// rows t + 16 e of column n2 = 16 cb + c, and after the two radix-16 passes (one LDS exchange) it
// holds Z[k1 = t + 16 e][n2].  Phase 2, row block rb (16 rows): the lane that works on row
// k1 = 16 rb + t at positions n2 = c + 16 e needs exactly Z[16 rb + t][16 e + c], e = 0..15 — the
// values this very lane produced for e = rb in column blocks cb = 0..15.  So the intermediate never
// changes lanes: every lane keeps a private 16 x 16 matrix keep[rb][cb] of complex values
//   rb 0..2   in LDS          (lane-private spill area, 400 bytes per lane)
//   rb 3      in a 32 KiB per-workgroup global slot (8 MiB for the whole chip, read back from L2) — the
//             one sixteenth that the register file cannot take next to the working registers
//   rb 4..7   in arch VGPRs   (four 32-float vectors, written through s_set_gpr_idx)
//   rb 8..15  in AGPRs        (a[32 (rb-8) + 2 cb], moved by v_accvgpr_* with literal register
//                              numbers inside a uniform switch)
// and no hand-over between the phases exists at all.  Fabric traffic is the algorithmic 16 bytes per
// sample plus the slot's 0.5 (written through) and at most 0.5 (read back).
//
// What one wave per SIMD costs, and what the kernel does about it (every item was measured on this kernel with
// parts left out: profiles/res16_probe_r02.txt; that scaffolding has left the source, profiles/HISTORY.md):
//   * nothing else runs while the wave waits, so a block's 16 loads / stores cannot be issued back
//     to back (each then waits ~80 cycles for a queue slot): they ride along the arithmetic, one per
//     hook point (16 per block, ~20 instructions apart) — the loads of the column block TWO ahead in
//     phase 1, the stores of the PREVIOUS row block in phase 2;
//   * those loads need somewhere to land that hipcc does not touch (it copies "its" registers
//     whenever it likes, also while a load is still pending on them): even column blocks land in AGPR
//     columns of the keep matrix that are still empty, odd ones in v[224:255] — the kernel is compiled
//     with amdgpu_num_vgpr(224), so the register allocator never sees those; the same registers park
//     a row block's results in phase 2 until their stores have been issued;
//   * hipcc counts none of that traffic: every wait is an explicit s_waitcnt vmcnt(N), N = the asm
//     loads issued after the awaited ones.
// tools/check_isa.py audits the code object (no compiler-generated AGPR moves, no compiler instruction
// on v[224:255], no scratch); tests/test_abi_cpu.py runs it on every build.
//
// Global accesses are buffer_load/store_dwordx2 ... offen nt with the row offsets e * 32 KiB in
// SGPRs: one instruction per access, no address arithmetic.  Both LDS exchanges write 8 x b128 and
// read 16 x SINGLE b64 (CLFA_RES16_TARGET below: paired into ds_read2_b64, as hipcc would, every read is a 2-way bank
// conflict), conflict-free under MI355X_MICROARCH.md's lane-group rules (layouts in fft_res_blocks.inc; rocprofv3 round 5:
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.29 -> 0.05, what is left is the spill deposit).  The four-step twiddles W_N^(n2 (t + 16 e)) =
// b * s^e come from one two-level lookup (b), four exact table values s, s^2, s^4, s^8 and a
// product tree (15 complex multiplies for 16 values); the forward 1/N rides on the table of b.
//
// The same kernel carries the packed real transforms of size 131072 (the largest of the reference's range,
// cl_fft.cpp:208-211, 267-296) in one pass as well: template flags R2C (the reference's `conv` pair map inside phase 2) and
// C2R (`iconv` inside phase 1) — fft_res_real.inc.
//
// One translation unit, one file per layer (every device function is inlined into the five kernels):
//   fft_res_regs.inc    the register files and the memory: AGPR access, landing registers, asm loads / stores, waits, hooks;
//   fft_res_blocks.inc  the 16-point passes with their hook points, one column block, one row block, the keep matrix's
//                       deposit / fetch; the LDS layouts and the table blob;
//   fft_res_real.inc    the two pair maps of the packed real transforms and the derivation of the pairing;
//   fft_resident.hip    the phase bodies, the kernel (prologue, phase 1, phase 2 per transform) and its launchers.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "fft_device.hpp"
#include "fft_launch.hpp"

#include "fft_res_regs.inc"
#include "fft_res_blocks.inc"
#include "fft_res_real.inc"

namespace clfa {
namespace {

// The two phase-2 bodies.  Common arguments: K = the keep matrix's VGPR rows, so = the pinned row offsets, lane (lane_m) =
// the kernel's lane builders, y = this transform's output, xn = the next transform's input.  (The two phase-1 bodies stay
// inside the kernel: as functions of their own hipcc optimises their loops apart from the kernel's and the code object
// changes, profiles/res16_refactor.txt.)

// ---- phase 2: row blocks in the order slot (its data are in the landing registers by now), AGPR
// (the accumulation file is then free for the next transform's block 0), VGPR, LDS.  All but the last block leave
// their results in the landing registers themselves (dft16_hp_land), from where they are stored while the next block
// is computed.
// v: the kernel's 16 working values (nothing is carried in them from phase 1)
// C2R: the keep matrix's AGPR columns are in the inverse kernel's order, and the next transform's first loads are its
template <bool FWD, bool C2R, class LF>
__device__ __forceinline__ void res_phase2_c2c(cpx (&v)[16], const f32x32 (&K)[kVgprBlk], const int (&so)[16], const LF &lane,
                                               const cpx *xn, cpx *y) {
  {
    const ResLane L = lane();
    res_wait_vm<0>();
    res_land_fetch(v);
    res_row_block<FWD, true>(v, L);
  }
  int rb_prev = kLdsBlk;
#pragma unroll 1
  for (int it = 1; it < 15; it++) {
    const ResLane L = lane();
    int rb;
    switch (it) {
#define CLFA_C(k, r) case k: res_fetch_static<r, C2R>(v, L, K); rb = r; break;
      CLFA_C(1, 8) CLFA_C(2, 9) CLFA_C(3, 10) CLFA_C(4, 11) CLFA_C(5, 12) CLFA_C(6, 13) CLFA_C(7, 14) CLFA_C(8, 15)
      CLFA_C(9, 4) CLFA_C(10, 5) CLFA_C(11, 6) CLFA_C(12, 7) CLFA_C(13, 0)
#undef CLFA_C
      default: res_fetch_static<1>(v, L, K); rb = 1; break;
    }
    if (it == 13) {
      if constexpr (C2R) res_issue_all(HookAcc<kZone0, kC2rKeepA>{res_rsrc(xn + 7 * 16), L.voff, so});   // the next transform's block 7
      else res_load_acc<kZone0>(xn, L.voff);
    }
    res_row_block<FWD, true>(v, L, HookStore{res_rsrc(y + rb_prev * 16), L.voff, so});
    rb_prev = rb;
  }
  {
    const ResLane L = lane();
    res_fetch_static<2>(v, L, K);
    res_row_block<FWD>(v, L, HookStore{res_rsrc(y + rb_prev * 16), L.voff, so});
    res_store(v, res_rsrc(y + 2 * 16), L.voff);
    // the next transform's block 1 -> landing registers (after this block's parked stores have been issued)
    if constexpr (C2R) {   // the next transform's block 8 (mirrored) and column 128
      res_issue_all(HookLandT<true>{res_rsrc(xn + 8 * 16), (15 - L.t) * 2048 + (16 - L.c) * 8, so});
      res_issue_all(HookAcc<kZone1, true>{res_rsrc(xn + 8 * 16), (15 - L.t) * 2048 + L.c * 8, so});
    } else res_load_land(xn + 16, L.voff);
  }
}

// ---- phase 2 of the packed real forward transform: pairs of row blocks (A = q natural, B = 15 - q mirrored),
// the reference's conv map behind each pair (fft_res_real.inc).  The working values are the function's own here: handed in
// by the kernel like res_phase2_c2c's they cost this variant three instructions (profiles/res16_refactor.txt).
template <class LF, class LM>
__device__ __forceinline__ void res_phase2_r2c(const f32x32 (&K)[kVgprBlk], const int (&so)[16], __amdgpu_buffer_rsrc_t slot,
                                               const LF &lane, const LM &lane_m, const cpx *xn, cpx *y, const cpx *s_tab,
                                               cpx *s_c0) {
  cpx v[16];
#pragma unroll 1
  for (int q = 0; q < 8; q++) {
    // stores into a zero-length buffer are dropped: pair 0 has nothing to store yet
    const unsigned live = q ? 0x7fffffffu : 0u;
    cpx base;
    {
      const ResLane L = lane();
      switch (q) {
        case 0: res_fetch_static<0>(v, L, K); break;
        case 1: res_fetch_static<1>(v, L, K); break;
        case 2: res_fetch_static<2>(v, L, K); break;
        case 3:   // the slot's block: loaded along block A_2; the 16 stores of block B_2 are younger
          res_wait_vm<kC2rWait ? 16 : 0>();
          acc_fetch_flat<kSlotAcc>(v);
          break;
        case 4: res_fetch_static<4>(v, L, K); break;
        case 5: res_fetch_static<5>(v, L, K); break;
        case 6: res_fetch_static<6>(v, L, K); break;
        default: res_fetch_static<7>(v, L, K); break;
      }
      // ... with the stores of A'_(q-1) (landing registers) riding along
      const __amdgpu_buffer_rsrc_t ra =
          __builtin_amdgcn_make_buffer_rsrc(y + (q - 1) * 16, 0, live, 0x00020000);
      if (q == 2) res_row_block<true, false, false>(v, L, Hook2<HookStore, HookSlotAcc<kSlotAcc>>{HookStore{ra, L.voff, so}, HookSlotAcc<kSlotAcc>{slot, L.slot_off, so}});
      else res_row_block<true, false, false>(v, L, HookStore{ra, L.voff, so});
      base = cmul(s_tab[kTabPair + 16 * q + L.c], s_tab[kTabPair + 256 + L.t]);
      if (q == 0) {
        res_pair_self_row<true>(v, L.c, L.t, base, s_c0);
      } else if (L.c == 0) {
        res_pair_patch_c0(v, base);
      }
      res_stage(v);   // A_q: raw in the lanes c != 0, finished in the lanes c = 0
    }
    {
      const ResLane L = lane_m();
      switch (q) {
        case 0: res_fetch_static<15>(v, L, K); break;
        case 1: res_fetch_static<14>(v, L, K); break;
        case 2: res_fetch_static<13>(v, L, K); break;
        case 3: res_fetch_static<12>(v, L, K); break;
        case 4: res_fetch_static<11>(v, L, K); break;
        case 5: res_fetch_static<10>(v, L, K); break;
        case 6: res_fetch_static<9>(v, L, K); break;
        default: res_fetch_static<8>(v, L, K); break;
      }
      // ... with the stores of B'_(q-1) (parked in the accumulation registers, finished by the patch above)
      const __amdgpu_buffer_rsrc_t rb =
          __builtin_amdgcn_make_buffer_rsrc(y + (16 - q) * 16, 0, live, 0x00020000);
      res_row_block<true, false, false>(v, L, HookStoreAcc<kParkAcc>{rb, L.voff, so});
      if (L.c != 0) res_pair_map(v, base);
      if (q == 7) {
        const cpx bm = cmul(s_tab[kTabPair + 128], s_tab[kTabPair + 256 + 15 - L.t]);
        res_pair_self_row<false>(v, L.c, L.t, bm, s_c0);
      } else {
        acc_park_flat<kParkAcc>(v);   // B'_q (its lanes c = 0 still raw)
      }
    }
  }
  {
    const ResLane L = lane(), Lm = lane_m();
    res_store_land(res_rsrc(y + 7 * 16), L.voff, so);
    res_store_so(v, res_rsrc(y + 8 * 16), Lm.voff, so);
    // the next transform's blocks 0 and 1
    res_load_acc<kZone0>(xn, L.voff);
    res_load_land(xn + 16, L.voff);
  }
}

}  // namespace

// slots: one 32 KiB slot per workgroup (the single row block that does not fit the CU)
// R2C: packed real transforms of size 2 kN, forward — the same transform with the reference's pair map inside phase 2
// (fft_res_real.inc); w2_g = the plan's pair twiddles W_2M^i (cl_fft.cpp:233-238), M entries
// C2R: ... inverse — the pair map inside phase 1
// hipcc's load / store optimiser pairs the exchanges' sixteen ds_read_b64 into eight ds_read2_b64, which the
// LDS serves per 16 contiguous lanes over 32 banks at half the rate (MI355X_MICROARCH.md, LDS table): in the layouts of
// fft_res_blocks.inc — made for the single reads, 2 x 32 lanes over 64 banks — every access is then a 2-way conflict,
// four times the LDS cycles (rocprofv3 round 4: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.29).  The pass is off for this kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#define CLFA_RES16_TARGET __attribute__((target("no-load-store-opt")))
#else
#define CLFA_RES16_TARGET
#endif
// DYN (complex transforms, batch > grid, grid a multiple of 8: xcd_shared_ok): the shared assignment.  A workgroup's first
// transform is today's (xcd_first); every further one is a position drawn from its XCD's counter `ctr` — today's
// XCD-compact sequence, dealt to whichever of the XCD's workgroups asks next — and once that share is used up, one draw
// from each other XCD's counter (res_draw_step, fft_res_regs.inc): the XCDs that finish early take over the tail of the
// ones that run late (profiles/res16_balance.txt), every transform still runs exactly once and its arithmetic does not
// depend on who runs it.  ctr: nine zeroed words kDrawStride bytes apart, zero again when the launch ends.
// rec (null in every ordinary call): one ResRecord per workgroup, written as it exits.
// Both are arguments of the complex instantiations only (X = unsigned *, ResRecord *); the packed real ones (X empty) keep
// the arguments, and with them the code, they had without either.
__device__ __forceinline__ unsigned *res_ctr_of() { return nullptr; }
__device__ __forceinline__ unsigned *res_ctr_of(unsigned *ctr, ResRecord *) { return ctr; }
__device__ __forceinline__ ResRecord *res_rec_of() { return nullptr; }
__device__ __forceinline__ ResRecord *res_rec_of(unsigned *, ResRecord *rec) { return rec; }
template <bool FWD, bool SCALE, bool R2C = false, bool C2R = false, bool DYN = false, class... X>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(224))) CLFA_RES16_TARGET void k_fft_res16(const cpx *data, cpx *out, cpx *__restrict__ slots,
                                                   const cpx *__restrict__ tabs_g, long batch,
                                                   const cpx *__restrict__ w2_g, X... extra) {
  static_assert(sizeof...(X) == ((R2C || C2R) ? 0 : 2), "ctr and rec: the complex transforms'");
  [[maybe_unused]] unsigned *const ctr = res_ctr_of(extra...);
  [[maybe_unused]] ResRecord *const rec = res_rec_of(extra...);
  static_assert(!R2C || (FWD && SCALE && !C2R), "the fused forward pair map");
  static_assert(!C2R || (!FWD && !SCALE), "the fused inverse pair map");
  static_assert(!DYN || (!R2C && !C2R), "the packed real transforms keep the static assignment");
  constexpr bool REC = !R2C && !C2R;
  [[maybe_unused]] __shared__ int s_next;
  [[maybe_unused]] unsigned done = 0;
  __shared__ __attribute__((aligned(16))) cpx s_tab[(R2C || C2R) ? kTabSizeR : kTabSize];
  __shared__ __attribute__((aligned(16))) cpx s_x[kXSize];
  __shared__ __attribute__((aligned(16))) char s_spill[256 * kSpillStride];
  __shared__ __attribute__((aligned(16))) cpx s_c0[(R2C || C2R) ? 256 : 1];
  __shared__ __attribute__((aligned(16))) cpx s_col0[C2R ? 2 * kXA : 1];   // first-pass results of the B blocks' column 0
  acc_claim_all();
  const int tid = threadIdx.x;
  for (int i = tid; i < kTabSize; i += 256) {
    cpx w = tabs_g[i];
    // exact: powers of two (R2C: the pair map's 1/2 as well)
    if (SCALE && i >= kTabLo && i < kTabHi) w = cscale(w, R2C ? 0.5f / (float)kN : 1.0f / (float)kN);
    if (C2R && i >= kTabLo && i < kTabHi) w = cscale(w, 0.5f);   // the inverse map's two factors 1/2
    s_tab[i] = w;
  }
  if constexpr (R2C || C2R) {
    s_tab[kTabPair + tid] = w2_g[tid];
    if (tid < 16) s_tab[kTabPair + 256 + tid] = w2_g[256 * tid];
  }
  // The lane's addresses are recomputed from an opaque copy of the lane index wherever a block
  // starts: as loop invariants they would cost ~13 VGPRs for the whole kernel, which hipcc then
  // parks in AGPRs (this kernel's own)
  auto lane = [&]() {
    int l = tid;
    asm volatile("" : "+v"(l));
    ResLane L;
    L.c = l & 15;
    L.t = l >> 4;
    L.voff = L.t * 2048 + L.c * 8;
    L.xa_w = s_x + L.c * kXA + 16 * L.t;
    L.xa_r = s_x + L.c * kXA + L.t;
    L.xb_w = s_x + L.t * kXB + 18 * L.c;
    L.xb_r = s_x + L.c * kXB + L.t;
    L.tw_row = s_tab + kTabTw + 16 * L.t;
    L.spill = s_spill + l * kSpillStride;
    L.slot_off = l * 8;
    return L;
  };
  // R2C, the B block of a pair: row (16 - c) mod 16 of the exchange, first-pass output 15 - t (and the stores follow)
  [[maybe_unused]] auto lane_m = [&]() {
    ResLane L = lane();
    const int cm = (16 - L.c) & 15, tm = 15 - L.t;
    L.voff = tm * 2048 + cm * 8;
    L.xb_r = s_x + cm * kXB + tm;
    L.tw_row = s_tab + kTabTw + 16 * tm;
    return L;
  };
  // C2R, the B block of a pair: first-pass results go to column slot 16 - c at position 16 (15 - t); the lanes c = 0
  // hold the NEXT pair's column 0 (-> copy buffer `save_w`) and read this block's from the previous pair's (`save_r`)
  [[maybe_unused]] auto lane_b = [&](cpx *save_w, const cpx *save_r) {
    ResLane L = lane();
    const int cm = 16 - L.c, tm = 15 - L.t;
    L.xa_w = (L.c ? s_x + cm * kXA : save_w) + 16 * tm;
    if (L.c == 0) L.xa_r = save_r + L.t;
    return L;
  };
  int so[16];   // row offsets e * 32 KiB of the asm loads, pinned in SGPRs (never rematerialised next to a load)
#pragma unroll
  for (int e = 0; e < 16; e++) {
    so[e] = e * 32768;
    asm volatile("" : "+s"(so[e]));
  }
  const __amdgpu_buffer_rsrc_t slot = res_rsrc(slots + (long)blockIdx.x * 4096);
  __syncthreads();

  f32x32 K[kVgprBlk];
#pragma unroll
  for (int j = 0; j < kVgprBlk; j++) K[j] = 0.f;
  cpx v[16];
  long b = xcd_first(blockIdx.x, gridDim.x);   // XCD-compact assignment (fft_device.hpp)
  [[maybe_unused]] ResDraw D{0, -1};
  // (an opaque copy of the lane index, as in lane(): what is derived from it is recomputed where it is used)
  [[maybe_unused]] auto draw_step = [&](auto RP, auto RC, int cb) {
    return [&, cb]() {
      if constexpr (DYN) {
        int l = tid;
        asm volatile("" : "+v"(l));
        if (__builtin_amdgcn_readfirstlane(l) < 64)
          res_draw_step<decltype(RP)::value, decltype(RC)::value>(D, cb, ctr, gridDim.x, (unsigned)batch, l, &s_next);
      }
    };
  };
  // the draws' registers: the first words of the landing zones' columns, in the order the zones fall empty (blocks 4 q,
  // 4 q + 1: Z0; 4 q + 2, 4 q + 3: Z1)
  constexpr int kD0 = 2 * kZone0, kD1 = 2 * kZone0 + 2, kD2 = 2 * kZone1, kD3 = 2 * kZone1 + 2;
  // blocks 0 and 1 of the first transform
  if constexpr (C2R) {
    // the first pair: block 7 -> Z0, block 8 mirrored -> landing registers, column 128 (lanes c = 0, mirrored rows) -> Z1
    const ResLane L0 = lane();
    const cpx *x0 = data + b * (long)kN;
    res_issue_all(HookAcc<kZone0, kC2rKeepA>{res_rsrc(x0 + 7 * 16), L0.voff, so});
    res_issue_all(HookLandT<true>{res_rsrc(x0 + 8 * 16), (15 - L0.t) * 2048 + (16 - L0.c) * 8, so});
    res_issue_all(HookAcc<kZone1, true>{res_rsrc(x0 + 8 * 16), (15 - L0.t) * 2048 + L0.c * 8, so});
  } else {
    const ResLane L0 = lane();
    res_load_acc<kZone0>(data + b * (long)kN, L0.voff);
    res_load_land(data + b * (long)kN + 16, L0.voff);
  }
#pragma unroll 1
  for (; b < batch;) {
    if constexpr (REC) done++;
    if constexpr (DYN) D.nxt = -1;
    const cpx *x = data + b * (long)kN;
    cpx *y = out + b * (long)kN;   // out == data: in place
    if constexpr (C2R) {
      // ---- phase 1 of the packed real inverse: pairs of column blocks, the reference's iconv map first (fft_res_real.inc)
      res_wait_vm<0>();
      {   // column 128 (lanes c = 0, out of Z1): pairs within itself; its first-pass results -> copy buffer 0
        const ResLane L = lane();
        acc_fetch_raw<kZone1>(v, std::make_integer_sequence<int, 8>());
        const cpx bm = cmul(s_tab[kTabPair + 128], s_tab[kTabPair + 256 + 15 - L.t]);
        res_unpair_self_col<false>(v, L.c, L.t, bm, s_c0);
        if (L.c == 0) {
          const HookNone none;
          CLFA_DFT16_H(false, v, none, kMapColA);
          f4 *pw = reinterpret_cast<f4 *>(s_col0 + 16 * (15 - L.t));
#pragma unroll
          for (int i = 0; i < 8; i++) pw[i] = pack2(v[2 * i], v[2 * i + 1]);
        }
      }
      // MODE 0: pairs 0..5, 1: pair 6 (the last pair's B block comes through the landing registers), 2: pair 7
      auto pair_step = [&](auto MODE, int p) {
        constexpr int mode = decltype(MODE)::value;
        const int q = 7 - p;
        {
          const ResLane L = lane();
          // loads of this pair: issued along the previous pair's A block (pair 7's B block: along pair 6's B block);
          // younger than they are only the slot stores of the blocks since (pair 0: waited for above)
          if (mode == 2) res_wait_vm<kC2rWait ? 1 : 0>();
          else if (p > 0) res_wait_vm<kC2rWait ? 2 : 0>();
          acc_fetch_raw<kZone0>(v, std::make_integer_sequence<int, 8>());
          if (mode == 1 || (mode == 0 && p > 0)) res_zone1_to_land();
          const cpx base = cmul(s_tab[kTabPair + 16 * q + L.c], s_tab[kTabPair + 256 + L.t]);
          if constexpr (mode == 2) {
            res_unpair_self_col<true>(v, L.c, L.t, base, s_c0);   // column 0
            if (L.c != 0) res_unpair_map(v, base);
          } else {
            res_unpair_map(v, base);
          }
          const int voff_m = (15 - L.t) * 2048 + (16 - L.c) * 8;
          if constexpr (mode == 0) {
            res_col_block<false>(v, L, q, s_tab, s_x,
                                 Hook2<HookAcc<kZone0, kC2rKeepA>, HookAcc<kZone1, true>>{HookAcc<kZone0, kC2rKeepA>{res_rsrc(x + (q - 1) * 16), L.voff, so},
                                                                                          HookAcc<kZone1, true>{res_rsrc(x + (16 - q) * 16), voff_m, so}});
          } else if constexpr (mode == 1) {
            res_col_block<false>(v, L, q, s_tab, s_x, HookAcc<kZone0, kC2rKeepA>{res_rsrc(x + (q - 1) * 16), L.voff, so});
          } else {
            res_col_block<false>(v, L, q, s_tab, s_x);
          }
          res_deposit<false, true>(v, L, q, K, slot);
        }
        {
          const ResLane L = lane_b(s_col0 + ((p + 1) & 1) * kXA, s_col0 + (p & 1) * kXA);
          res_land_fetch(v);
          if constexpr (mode == 0) {
            res_col_block<false>(v, L, 15 - q, s_tab, s_x);
          } else if constexpr (mode == 1) {
            // block 15 mirrored (its lanes c = 0 have no partner column to fetch: out of the buffer's range)
            const int voff_m = L.c ? (15 - L.t) * 2048 + (16 - L.c) * 8 : (int)0x80000000;
            res_col_block<false>(v, L, 15 - q, s_tab, s_x, HookLandT<true>{res_rsrc(x + 15 * 16), voff_m, so});
          } else {
            res_col_block<false>(v, L, 15 - q, s_tab, s_x, HookSlot{slot, L.slot_off, so});
          }
          res_deposit<mode == 2, true>(v, L, 15 - q, K, slot);
        }
      };
#pragma unroll 1
      for (int p = 0; p < 6; p++) pair_step(ic<0>(), p);
      pair_step(ic<1>(), 6);
      pair_step(ic<2>(), 7);
    } else {
      // ---- phase 1: four column blocks per round (landing zones Z0, v[224:255], Z1, v[224:255]); on entry
      // block 0 is in (or on its way to) Z0 and block 1 on its way to the landing registers
#pragma unroll 1
      for (int cb = 0; cb < 12; cb += 4) {
        if constexpr (DYN) {
          res_phase1_block<FWD, kZone0, kZone1, true, 16, false>(v, lane(), x, cb, so, K, slot, s_tab, s_x, draw_step(ic<kD3>(), ic<kD0>(), cb));
          res_phase1_block<FWD, -1, -1, true, 16, false>(v, lane(), x, cb + 1, so, K, slot, s_tab, s_x, draw_step(ic<kD0>(), ic<kD1>(), cb + 1));
          res_phase1_block<FWD, kZone1, kZone0, true, 16, false>(v, lane(), x, cb + 2, so, K, slot, s_tab, s_x, draw_step(ic<kD1>(), ic<kD2>(), cb + 2));
          res_phase1_block<FWD, -1, -1, true, 16, false>(v, lane(), x, cb + 3, so, K, slot, s_tab, s_x, draw_step(ic<kD2>(), ic<kD3>(), cb + 3));
        } else {
        res_phase1_block<FWD, kZone0, kZone1, true>(v, lane(), x, cb, so, K, slot, s_tab, s_x);
        res_phase1_block<FWD, -1, -1, true>(v, lane(), x, cb + 1, so, K, slot, s_tab, s_x);
        res_phase1_block<FWD, kZone1, kZone0, true>(v, lane(), x, cb + 2, so, K, slot, s_tab, s_x);
        res_phase1_block<FWD, -1, -1, true>(v, lane(), x, cb + 3, so, K, slot, s_tab, s_x);
        }
      }
      res_phase1_block<FWD, kZone0, kZone1, true>(v, lane(), x, 12, so, K, slot, s_tab, s_x);
      res_phase1_block<FWD, -1, -1, true>(v, lane(), x, 13, so, K, slot, s_tab, s_x);
      res_phase1_block<FWD, kZone1, -1, false>(v, lane(), x, 14, so, K, slot, s_tab, s_x);
      // (R2C fetches the slot's row block later, along its phase 2: HookSlotAcc)
      res_phase1_block<FWD, -1, -1, false, 0, !R2C>(v, lane(), x, 15, so, K, slot, s_tab, s_x);
    }
    // ---- phase 2 (the next transform's first loads ride along: clamped, they are issued unconditionally)
    long bn;
    if constexpr (DYN) {
      // wave 0 posted the draws' outcome in column block 8; without a next transform the loads re-read this one
      const int nx = __builtin_amdgcn_readfirstlane(s_next);
      bn = nx < 0 ? b : (long)nx;
      const cpx *xn = data + bn * (long)kN;
      res_phase2_c2c<FWD, C2R>(v, K, so, lane, xn, y);
      b = nx < 0 ? batch : bn;
    } else {
      bn = b + gridDim.x;
      bn = bn < batch ? bn : batch - 1;
      const cpx *xn = data + bn * (long)kN;
      if constexpr (R2C) res_phase2_r2c(K, so, slot, lane, lane_m, xn, y, s_tab, s_c0);
      else res_phase2_c2c<FWD, C2R>(v, K, so, lane, xn, y);
      b += gridDim.x;
    }
  }
  if constexpr (REC) {
    if (rec && tid == 0) {
      rec[blockIdx.x] = ResRecord{done, blockIdx.x & 7, (unsigned long long)wall_clock64()};
    }
  }
}

namespace {

// one workgroup per CU (fewer for small batches); X: the complex instantiations' counters and records
int res_grid(long batch, const DeviceInfo &di) { return (int)(batch < di.num_cus ? batch : di.num_cus); }
template <class... X>
hipError_t res_launch(void (*k)(const cpx *, cpx *, cpx *, const cpx *, long, const cpx *, X...), const cpx *data, cpx *out,
                      cpx *slots, const cpx *tabs, const cpx *w2, long batch, const DeviceInfo &di, hipStream_t s, X... extra) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(k, dim3(res_grid(batch, di)), dim3(256), 0, s, data, out, slots, tabs, batch, w2, extra...);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fft_res16(bool fwd, bool scale, const cpx *data, cpx *out, cpx *slots, const cpx *tabs, long batch,
                            const DeviceInfo &di, hipStream_t s, unsigned *ctr, ResRecord *rec) {
  if (batch <= 0) return hipSuccess;
  if (!fwd && scale) return hipErrorInvalidValue;
  // the shared assignment where it applies (and the caller has counters for it), else the static one
  if (ctr && xcd_shared_ok(batch, (unsigned)res_grid(batch, di))) {
    const auto k = !fwd ? k_fft_res16<false, false, false, false, true, unsigned *, ResRecord *>
                   : scale ? k_fft_res16<true, true, false, false, true, unsigned *, ResRecord *>
                           : k_fft_res16<true, false, false, false, true, unsigned *, ResRecord *>;
    return res_launch(k, data, out, slots, tabs, (const cpx *)nullptr, batch, di, s, ctr, rec);
  }
  const auto k = !fwd ? k_fft_res16<false, false, false, false, false, unsigned *, ResRecord *>
                 : scale ? k_fft_res16<true, true, false, false, false, unsigned *, ResRecord *>
                         : k_fft_res16<true, false, false, false, false, unsigned *, ResRecord *>;
  return res_launch(k, data, out, slots, tabs, (const cpx *)nullptr, batch, di, s, (unsigned *)nullptr, rec);
}

hipError_t launch_crfft_res16(const cpx *data, cpx *out, cpx *slots, const cpx *tabs, const cpx *w2, long batch,
                              const DeviceInfo &di, hipStream_t s) {
  return res_launch(k_fft_res16<false, false, false, true>, data, out, slots, tabs, w2, batch, di, s);
}

hipError_t launch_rfft_res16(const cpx *data, cpx *out, cpx *slots, const cpx *tabs, const cpx *w2, long batch,
                             const DeviceInfo &di, hipStream_t s) {
  return res_launch(k_fft_res16<true, true, true>, data, out, slots, tabs, w2, batch, di, s);
}

}  // namespace clfa
