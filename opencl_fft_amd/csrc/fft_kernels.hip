// fft_kernels.hip — batched 1-D FFT kernels for gfx950 (MI355X): one translation unit, one file per kernel family.
//
//   fft_lds.inc    k_fft_lds, k_fft_small, k_fft_tiny: a transform (n <= 8192) in the VGPRs + LDS of one workgroup;
//   fft_2x.inc     k_rfft_2x, k_cfft_2x: two runs of that machinery and a radix-2 step in registers;
//   fft_4step.inc  k_fft_4step: n = 2^14 .. 2^16, N1 x N2 in one persistent kernel;
//   fft_big.inc    k_big2_*, k_big_*: n = 2^17 .. 2^24, composed with the above;
//   fft_aux.inc    k_r2c_pack / k_c2r_unpack, k_reorder, Bluestein (k_blue_*).
// The families meet only through the launchers of fft_launch.hpp and the pieces of fft_xfer.hpp.  They stay ONE translation
// unit, in this order, because of the compiler: every device function is inlined, in the order the module lists them, and
// that order follows the first use in the unit.  Compiled apart, 26 of the 144 kernels here (k_fft_lds<13>, k_big2_*,
// k_blue_lds<12 | 13>, k_fft_4step_rows<14>, k_rfft_2x_s<13> inverse) come out with other instructions
// (profiles/fft_split_isa_r09.txt); together they are the kernels every figure in profiles/ was measured on.
#include "fft_launch.hpp"   // the launchers the families define
#include "fft_route.hpp"    // kLdsMaxLog, kMaxLog, kBig2MaxLog, FftMode and the small-size predicates

#include "fft_lds.inc"
#include "fft_2x.inc"
#include "fft_4step.inc"
#include "fft_big.inc"
#include "fft_aux.inc"
