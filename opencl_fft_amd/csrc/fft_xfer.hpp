// fft_xfer.hpp — how the FFT kernel families (fft_lds.inc, fft_2x.inc, fft_4step.inc, fft_big.inc) touch global memory:
// non-temporal 8- and 16-byte accesses, buffer-descriptor addressing for transforms owned by a whole workgroup, and the
// function attribute that keeps a kernel's LDS accesses single.
#pragma once
#include "fft_wg.hpp"

namespace clfa {

typedef float f4v __attribute__((ext_vector_type(4)));

// every transform is read once and written once: non-temporal streams (copy kernels on this chip:
// 5.2 TB/s with nt vs 4.95 plain)
__device__ __forceinline__ cpx ld_nt(const cpx *p) {
  const unsigned long long raw = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long *>(p));
  return *reinterpret_cast<const cpx *>(&raw);
}
__device__ __forceinline__ void st_nt(cpx *p, cpx v) {
  __builtin_nontemporal_store(*reinterpret_cast<unsigned long long *>(&v), reinterpret_cast<unsigned long long *>(p));
}
__device__ __forceinline__ f4v ld_nt16(const cpx *p) { return *reinterpret_cast<const f4v *>(p); }   // (a plain load: the cache policy below)
__device__ __forceinline__ void st_nt16(cpx *p, f4v v) { __builtin_nontemporal_store(v, reinterpret_cast<f4v *>(p)); }

// Transforms owned by a whole workgroup (T >= 256 lanes, one transform per workgroup): the transform's base is
// wave-uniform, so its accesses go through a buffer descriptor — the lane's byte offset in ONE VGPR, everything
// else (the element stride of the pass, the mirrored position of a pair's partner) in the instruction's scalar
// offset.  With flat 64-bit addresses hipcc kept one address pair per access alive (16 pairs = 32 VGPRs for the
// two store streams of the packed real kernels, under a 128-VGPR cap) and rebuilt them every iteration.
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
struct XferBuf {
  __amdgpu_buffer_rsrc_t r;
  int va;   // t * 8: ascending positions t + c
  int vd;   // (T - t) * 8: descending positions c - t, as vd + (c - T) * 8
};
template <int LOGN> __device__ __forceinline__ XferBuf xfer_buf(const cpx *x, int t) {
  return XferBuf{__builtin_amdgcn_make_buffer_rsrc(const_cast<cpx *>(x), 0, 0x7fffffff, 0x00020000), t * 8,
                 (LdsGeom<LOGN>::T - t) * 8};
}
// Cache policy of the packed real kernels' loads: PLAIN loads, non-temporal stores.  Measured (interleaved A/B, steps
// alternating r2c / c2r, 1 GiB): size 16384 0.2054 -> 0.1974 ms (5.23 -> 5.44 TB/s) with both directions' loads plain,
// 0.2012 / 0.2027 with one of them; sizes 8192 and 32768 within 1 %.  (The complex kernels lose 2-9 % with plain
// loads and 3-8 % with plain stores: they keep non-temporal both ways — profiles/ab_cache_policy_r03.txt.)
// The same holds for the persistent four-step kernel (n = 2^14, 2^15: 4.80 -> 4.83, 4.82 -> 4.93 TB/s) and for packed
// real size 65536 (k_rfft_2x<14>: 3.80 -> 3.96 TB/s): plain loads, non-temporal stores.
template <bool NT> __device__ __forceinline__ cpx ld_buf(const XferBuf &b, int voff, int soff) {
  return __builtin_bit_cast(cpx, __builtin_amdgcn_raw_buffer_load_b64(b.r, voff, soff, NT ? 2 : 0));   // aux 2: non-temporal
}
__device__ __forceinline__ void st_buf(const XferBuf &b, int voff, int soff, cpx v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, v), b.r, voff, soff, 2);
}

// hipcc pairs neighbouring ds_read_b64 / ds_write_b64 into ds_read2(st64)_b64 / ds_write2_b64, which the LDS serves at half
// the bytes per clock (MI355X_MICROARCH.md, LDS table; fft_resident.hip has the whole story).  Kernels marked CLFA_DS_SINGLE_FN
// are compiled without that pass.  It is a property of the FUNCTION, not of an instantiation, and pays for some
// instantiations only (profiles/ab_ds_single_r05.txt: n = 32768 -2.0 %, packed real 32768 -1.3 .. -1.5 %, real 16384 0 .. -0.9 %;
// complex 8192 +2.1 %, 1024 +2.0 %, real 65536 +3.3 %): k_fft_4step has it, k_rfft_2x exists as one body and two kernels
// (`_s`: single LDS accesses, real size 32768), k_fft_lds and k_cfft_2x stay paired.
#if defined(__HIP_DEVICE_COMPILE__)
#define CLFA_DS_SINGLE_FN __attribute__((target("no-load-store-opt")))
#else
#define CLFA_DS_SINGLE_FN
#endif

}  // namespace clfa
