// cpx.hpp — the complex value every kernel, launcher and host table shares: the cpx type, CLFA_HD, and the arithmetic
// on one value (mk, cadd, csub, cscale, cconj, cmulc, cmulc2, cmul, cmul_plain).  Nothing of the FFT engine: that is
// fft_device.hpp, which includes this.
//
// The header is also host-compilable (CLFA_HD) so tests/cpp/emulate_engine.cpp
// can run the same pass code on the CPU, lane by lane.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLFA_HD __host__ __device__ __forceinline__
#else
#define CLFA_HD inline
#endif

namespace clfa {

// A complex value is a native 2-float vector on the device (and wherever clang compiles this
// header): it lives in an aligned VGPR pair from the 8-byte load to the 8-byte store, and the
// arithmetic below is CDNA's packed fp32 (v_pk_add/mul/fma_f32: both halves per instruction, the
// same issue slot as a scalar op).  The multiplies and the +-i rotations use the instructions'
// operand swizzles (op_sel: which half of a source feeds each half of the result; neg_lo/neg_hi)
// through inline asm, because hipcc materialises such swizzles as v_mov / v_xor instead of folding
// them: a complex multiply is 2 instructions instead of 4, add/sub (also with one operand times
// +-i) 1 instead of 2.  g++ (tests/cpp/emulate_engine.cpp) sees a plain struct and scalar code.
#if defined(__clang__)
typedef float cpx __attribute__((ext_vector_type(2)));
#define CLFA_VEC 1
#else
struct alignas(8) cpx {
  float x, y;
};
#define CLFA_VEC 0
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define CLFA_PK 1
#else
#define CLFA_PK 0
#endif

CLFA_HD cpx mk(float x, float y) { cpx r; r.x = x; r.y = y; return r; }
#if CLFA_VEC
CLFA_HD cpx cadd(cpx a, cpx b) { return a + b; }
CLFA_HD cpx csub(cpx a, cpx b) { return a - b; }
CLFA_HD cpx cscale(cpx a, float s) { return a * s; }
#else
CLFA_HD cpx cadd(cpx a, cpx b) { return mk(a.x + b.x, a.y + b.y); }
CLFA_HD cpx csub(cpx a, cpx b) { return mk(a.x - b.x, a.y - b.y); }
CLFA_HD cpx cscale(cpx a, float s) { return mk(a.x * s, a.y * s); }
#endif
CLFA_HD cpx cconj(cpx a) { return mk(a.x, -a.y); }
// a * b, or a * conj(b).  The two instructions sit in ONE asm statement: hipcc pads every statement
// whose result the next instruction reads with an s_nop (it cannot see that this is a plain VALU
// dependency), which cost one issue slot per complex multiply.
template <bool CONJ = false> CLFA_HD cpx cmulc(cpx a, cpx b) {
#if CLFA_PK
  cpx r;
  if (!CONJ) {
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"                                                // (ax bx, ax by)
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"                  // (-ay by, ay bx) + t
        : "=&v"(r) : "v"(a), "v"(b));
  } else {
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1] neg_hi:[0,1]\n\t"                                   // (ax bx, -ax by)
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1]"                                 // (ay by, ay bx) + t
        : "=&v"(r) : "v"(a), "v"(b));
  }
  return r;
#else
  return CONJ ? mk(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y) : mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
#endif
}
// two independent products in one statement, interleaved (mul, mul, fma, fma): no dependent
// back-to-back issue and one statement boundary for four instructions
template <bool CONJ = false> CLFA_HD void cmulc2(cpx &r0, cpx &r1, cpx a0, cpx b0, cpx a1, cpx b1) {
#if CLFA_PK
  cpx x, y;
  if (!CONJ) {
    asm("v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %4, %5 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n\t"
        "v_pk_fma_f32 %1, %4, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(x), "=&v"(y) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
  } else {
    asm("v_pk_mul_f32 %0, %2, %3 op_sel_hi:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %1, %4, %5 op_sel_hi:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %1, %4, %5, %1 op_sel:[1,1,0] op_sel_hi:[1,0,1]"
        : "=&v"(x), "=&v"(y) : "v"(a0), "v"(b0), "v"(a1), "v"(b1));
  }
  r0 = x;
  r1 = y;
#else
  r0 = cmulc<CONJ>(a0, b0);
  r1 = cmulc<CONJ>(a1, b1);
#endif
}
CLFA_HD cpx cmul(cpx a, cpx b) { return cmulc<false>(a, b); }
// the same without inline asm, for loops hipcc has to unroll with a run-time trip count: HIP treats
// every asm statement as convergent, and a loop with a convergent operation is not given a remainder loop
CLFA_HD cpx cmul_plain(cpx a, cpx b) { return mk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

}  // namespace clfa
