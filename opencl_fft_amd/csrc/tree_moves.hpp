// tree_moves.hpp — the in-wave moves and the fold of the descriptors' TREE SUM (include/clfft_amd.h), for the kernel files
// that form such sums: pvoc_desc.hip and pvoc_demix.hip (through pvoc_device.hpp) and bank_kernels.hip, which shares
// nothing else with the launchers of the frame operations.
//   desc_dpp, desc_xor_bits, desc_xor   a DPP move by its control word; v of lane ^ STEP
//   desc_fold, desc_bitrev2             one level of the tree on the values a lane holds; where a value ends up
#pragma once
#include <hip/hip_runtime.h>

namespace clfa {

// The moves of the TREE SUM inside a wave: a DPP move by its control word, and v of lane ^ STEP (quad_perm for ^ 1 and
// ^ 2, ds_swizzle for ^ 4 and ^ 16, row_ror:8 for ^ 8, ds_bpermute for ^ 32)
template <int CTRL>
__device__ __forceinline__ int desc_dpp(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// v of lane ^ STEP
template <int STEP>
__device__ __forceinline__ int desc_xor_bits(int v) {
  static_assert(STEP == 1 || STEP == 2 || STEP == 4 || STEP == 8 || STEP == 16 || STEP == 32, "a level of one wave");
  if constexpr (STEP == 1) return desc_dpp<0xB1>(v);                            // quad_perm [1,0,3,2]
  else if constexpr (STEP == 2) return desc_dpp<0x4E>(v);                       // quad_perm [2,3,0,1]
  else if constexpr (STEP == 4) return __builtin_amdgcn_ds_swizzle(v, 0x101F);  // and 0x1f, xor 0x04
  else if constexpr (STEP == 8) return desc_dpp<0x128>(v);                      // row_ror:8
  else if constexpr (STEP == 16) return __builtin_amdgcn_ds_swizzle(v, 0x401F); // and 0x1f, xor 0x10
  else return __shfl_xor(v, 32);
}
template <int STEP>
__device__ __forceinline__ float desc_xor(float v) {
  return __builtin_bit_cast(float, desc_xor_bits<STEP>(__builtin_bit_cast(int, v)));
}


// One level of the tree on the N values the lane still holds, V[0 .. N): the half that bit STEP of the lane names stays
// and takes the partner's partial sum, the other half goes to the partner; N / 2 values are left, in V[0 .. N/2).  After
// the levels of 1 and 2 lanes on four values a lane holds value number desc_bitrev2(lane & 3)
template <int STEP, int N, int LEN>
__device__ __forceinline__ void desc_fold(float (&V)[LEN], bool up) {
#pragma clang fp contract(off)
  static_assert(N <= LEN, "the values held");
#pragma unroll
  for (int i = 0; i < N / 2; i++) {
    const float keep = up ? V[i + N / 2] : V[i], send = up ? V[i] : V[i + N / 2];
    V[i] = keep + desc_xor<STEP>(send);
  }
}
__device__ __forceinline__ int desc_bitrev2(int x) { return ((x & 1) << 1) | ((x >> 1) & 1); }

}  // namespace clfa
