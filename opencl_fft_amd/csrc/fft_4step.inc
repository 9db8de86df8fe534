// fft_4step.inc (part of the translation unit fft_kernels.hip) — batched 1-D FFTs of n = 2^14 .. 2^16 for gfx950 (MI355X).
//
//   k_fft_4step  n = 2^14..2^16: N1 x N2 decomposition, both phases in ONE persistent
//                kernel, one 512-lane workgroup per CU; the intermediate stays on the CU —
//                two row blocks in LDS, up to ten in the registers of the lanes that
//                computed them, handed over through LDS — all of it for n <= 2^15, 3/4 at
//                n = 2^16 (the rest goes through a 512 KiB scratch slot per workgroup);
//   k_fft_4step_cols / k_fft_4step_rows  the two phases as two launches, for a few transforms.
// (n = 65536 with more than a few transforms runs the resident kernel, fft_resident.hip.)
#include "fft_xfer.hpp"

#include <type_traits>

namespace clfa {

// ---------------------------------------------------------------------------------
// four-step FFT for n = 2^14 .. 2^16
// ---------------------------------------------------------------------------------

int fourstep_split(int logn, int *l1, int *l2, int *loglo) {
  if (logn < 14 || logn > 16) return -1;
  *l1 = logn / 2;
  *l2 = logn - *l1;
  *loglo = logn / 2;
  return 0;
}

constexpr int kFourRrb16 = 5;   // register-resident row blocks per slice of the n = 65536 kernel
template <int LOGN> struct FourGeom {
  static constexpr int LOGN1 = LOGN / 2, LOGN2 = LOGN - LOGN1;
  static constexpr int N = 1 << LOGN, N1 = 1 << LOGN1, N2 = 1 << LOGN2;
  static constexpr int LOGLO = LOGN / 2, LO = 1 << LOGLO, HI = 1 << (LOGN - LOGLO);
  static constexpr int SLICE = 256;                 // lanes per slice
  static constexpr int T1 = N1 / 16, C1 = SLICE / T1;   // lanes per column FFT, columns per slice
  static constexpr int T2 = N2 / 16, R2 = SLICE / T2;   // lanes per row FFT, rows per slice
  static constexpr int S2 = lds_padded_size(N2) | 1;    // odd row stride in LDS
  static constexpr int SL = (N1 * C1 > R2 * S2) ? N1 * C1 : R2 * S2;  // exchange elements per slice
  static constexpr int NCB = N2 / C1, NRB = N1 / R2;    // column blocks, row blocks per transform
  static constexpr int TABS = N1 / 2 + N2 / 2 + LO + HI;
  // rows of the intermediate kept in LDS instead of the scratch (k_fft_4step, KL rows): row stride
  // N2 + 16 elements puts the 4 rows a wave touches on 2 x 32 banks (the 2 passes 512 B need anyway)
  static constexpr int RS = N2 + 16;
};

// Wave-uniform base pointers kept in SGPR pairs.  A global access whose address is
// (uniform 64-bit base) + (32-bit lane offset) uses the saddr form  global_load v, v_off, s[b:b+1]:
// no 64-bit VALU add with carry (and its hazard nops) per access.  The base goes through an opaque
// SGPR integer so that hipcc cannot fold the lane part into it, and comes back as a global-memory
// (address space 1) pointer so that the access is not demoted to a flat one.
typedef __attribute__((address_space(1))) unsigned long long *gptr;
typedef const __attribute__((address_space(1))) unsigned long long *gcptr;
__device__ __forceinline__ gptr sgpr_base(const cpx *p) {
  unsigned long long b = reinterpret_cast<unsigned long long>(p);
  asm volatile("" : "+s"(b));
  return reinterpret_cast<gptr>(b);
}
// streaming mode: 0 plain, 1 non-temporal stores and plain loads (fft_xfer.hpp, ld_buf: +0.6 .. 2 %), 2 system scope
// (sc0 sc1), 3 agent scope (sc1: bypasses the CU's L1)
template <int SM> __device__ __forceinline__ cpx ld_g(gcptr p) {
  unsigned long long raw;
  if constexpr (SM == 2) raw = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else if constexpr (SM == 3) raw = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else raw = *p;
  return *reinterpret_cast<const cpx *>(&raw);
}
template <int SM> __device__ __forceinline__ void st_g(gptr p, cpx v) {
  const unsigned long long raw = *reinterpret_cast<const unsigned long long *>(&v);
  if constexpr (SM == 1) __builtin_nontemporal_store(raw, p);
  else if constexpr (SM == 2) __hip_atomic_store(p, raw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else *p = raw;
}

// phase 1 of one slice: column block cb of `src` (N1 x N2, row-major) ->
// N1-point FFT down the columns, times W_N^(n2*k1), stored to dst[k1][n2].
// streaming mode of the input loads / output stores: 0 plain, 1 non-temporal, 2 system scope (sc0 sc1)
template <int LOGN, int SM>
__device__ __forceinline__ void four_load1(cpx (&v)[16], const cpx *__restrict__ src, int cb, int l) {
  using G = FourGeom<LOGN>;
  const unsigned col = (unsigned)l % G::C1, tf = ((unsigned)l & (G::SLICE - 1)) / G::C1;
  const unsigned lane = tf * G::N2 + col;
  const cpx *base = src + cb * G::C1;   // cb is wave-uniform
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = ld_g<SM>(sgpr_base(base + (long)(G::T1 * e) * G::N2) + lane);
}
// A lane's results of one register-resident row block over the column blocks of its slice (8 values
// for every n: n = 65536 has 1 row set per block x 8 column blocks, 32768 2 x 4, 16384 4 x 2).  A native
// vector so that hipcc indexes it with the uniform loop counter through s_set_gpr_idx (an array would
// go to scratch memory).
typedef float vkeep __attribute__((ext_vector_type(16)));
struct NoKeep {};
// KL > 0: rows k1 < KL of the result (the first KL / R2 row blocks) stay in LDS (`rows`, stride RS) and
// never reach the scratch; NE > 0: the next NE row blocks stay in the lane's own registers
// (`keep[block]`, element it * EB + eb for the slice's it-th column block) until phase 2 hands them
// over through LDS
template <int LOGN, bool FWD, int KL = 0, int NE = 0, class Keep = NoKeep, class Tab = const cpx *>
__device__ __forceinline__ void four_body1(cpx (&v)[16], cpx *__restrict__ dst, int cb, int l, const Tab &tab1,
                                           const cpx *tlo, const cpx *thi, cpx *sx, cpx *rows = nullptr,
                                           Keep *keep = nullptr, int it = 0) {
  using G = FourGeom<LOGN>;
  const int col = (unsigned)l % G::C1, tf = ((unsigned)l & (G::SLICE - 1)) / G::C1;
  const int n2 = cb * G::C1 + col;
  pass_compute<G::LOGN1, 4, 0, FWD>(v, tf, tab1);
  __syncthreads();
  pass_scatter<G::LOGN1, 4, 0>(v, tf, [&](int p, cpx val) { sx[p * G::C1 + col] = val; });
  __syncthreads();
  pass_gather<G::LOGN1, 4>(v, tf, [&](int p) { return sx[p * G::C1 + col]; });
  pass_compute<G::LOGN1, 4, 4, FWD>(v, tf, tab1);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k1 = tf + G::T1 * e;
    const int ex = n2 * k1;  // < N
    const cpx o = cmulc<!FWD>(v[e], cmul(tlo[ex & (G::LO - 1)], thi[ex >> G::LOGLO]));
    // row k1 = tf + T1*e belongs to row block e / EB (EB row sets per block): all decided at compile time
    constexpr int EB = G::R2 / G::T1;
    const int blk = e / EB, eb = e % EB;
    if (blk < KL / G::R2) {
      rows[k1 * G::RS + n2] = o;
    } else if (blk < KL / G::R2 + NE) {
      if constexpr (NE > 0) {
        keep[blk - KL / G::R2][2 * (it * EB + eb)] = o.x;
        keep[blk - KL / G::R2][2 * (it * EB + eb) + 1] = o.y;
      }
    } else {
      st_g<0>(sgpr_base(dst + (long)(G::T1 * e) * G::N2 + cb * G::C1) + (unsigned)(tf * G::N2 + col), o);
    }
  }
}
template <int LOGN, bool FWD, int SM>
__device__ __forceinline__ void four_phase1(const cpx *__restrict__ src, cpx *__restrict__ dst, int cb, int l,
                                            const cpx *tab1, const cpx *tlo, const cpx *thi, cpx *sx) {
  cpx v[16];
  four_load1<LOGN, SM>(v, src, cb, l);
  four_body1<LOGN, FWD>(v, dst, cb, l, tab1, tlo, thi, sx);
}

// 8-byte load that bypasses the CU's vector L1 (global_load_dwordx2 ... sc1): data another
// CU of the same XCD has stored is served from the shared L2 (MI355X_MICROARCH.md, workgroup
// dispatch & inter-workgroup visibility)
__device__ __forceinline__ cpx ld_sc1(const cpx *p) {
  unsigned long long raw = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
  return *reinterpret_cast<cpx *>(&raw);
}

template <int LOGN, bool SC1>
__device__ __forceinline__ void four_load2(cpx (&v)[16], const cpx *__restrict__ src, int rb, int l) {
  using G = FourGeom<LOGN>;
  const int tf = (unsigned)l % G::T2, row = ((unsigned)l & (G::SLICE - 1)) / G::T2;
  const gcptr p = sgpr_base(src + (long)(rb * G::R2) * G::N2) + (unsigned)(row * G::N2 + tf);   // rb is wave-uniform
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = ld_g<SC1 ? 3 : 0>(p + G::T2 * e);
}
// the same row block out of the LDS-resident rows
template <int LOGN>
__device__ __forceinline__ void four_load2_rows(cpx (&v)[16], const cpx *rows, int rb, int l) {
  using G = FourGeom<LOGN>;
  const int tf = l % G::T2, row = l / G::T2;
  const cpx *p = rows + (rb * G::R2 + row) * G::RS + tf;
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = p[G::T2 * e];
}
struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};
// `between` runs between the block's two barriers (after every wave has passed the first one): the
// register-resident row blocks are handed over there at no extra barrier
template <int LOGN, bool FWD, bool SCALE, int SM, class Tab = const cpx *, class Hook = NoHook>
__device__ __forceinline__ void four_body2(cpx (&v)[16], cpx *__restrict__ dst, int rb, int l, const Tab &tab2,
                                           cpx *sx, unsigned *read_done = nullptr, Hook between = Hook()) {
  using G = FourGeom<LOGN>;
  {
    const int tf = l % G::T2, row = l / G::T2;
    pass_compute<G::LOGN2, 4, 0, FWD>(v, tf, tab2);
    __syncthreads();
    cpx *xr = sx + row * G::S2;
    pass_scatter_padded<G::LOGN2, 4, 0>(v, tf, xr);
    between();
    __syncthreads();
    // every lane has consumed its loads from the scratch: the slot may be reused
    if (read_done != nullptr && l == 0)
      (void)__hip_atomic_fetch_add(read_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // in the XCD's L2
  }
  // the last pass runs with rows on the fast lane index so that the transposed
  // store below is contiguous across lanes
  // (masked: the lane index passes through an opaque move in the callers; its range has to be visible
  // for the 32-bit lane offsets of the saddr addressing)
  const int row = (unsigned)l % G::R2, tf = ((unsigned)l & (G::SLICE - 1)) / G::R2;
  const cpx *xr = sx + row * G::S2;
  pass_gather_padded<G::LOGN2, 4>(v, tf, xr);
  pass_compute<G::LOGN2, 4, 4, FWD>(v, tf, tab2);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k2 = tf + G::T2 * e;
    cpx o = v[e];
    if constexpr (SCALE) o = cscale(o, 1.0f / (float)G::N);
    (void)k2;
    st_g<SM>(sgpr_base(dst + (long)(G::T2 * e) * G::N1 + rb * G::R2) + (unsigned)(tf * G::N1 + row), o);
  }
}
// phase 2 of one slice: row block rb of `src` (rows k1, contiguous n2) ->
// N2-point FFT along each row -> dst[k1 + N1*k2] (natural order of the result)
template <int LOGN, bool FWD, bool SCALE, int SM, bool SC1 = false>
__device__ __forceinline__ void four_phase2(const cpx *__restrict__ src, cpx *__restrict__ dst, int rb, int l,
                                            const cpx *tab2, cpx *sx, unsigned *read_done = nullptr) {
  cpx v[16];
  four_load2<LOGN, SC1>(v, src, rb, l);
  four_body2<LOGN, FWD, SCALE, SM>(v, dst, rb, l, tab2, sx, read_done);
}

// The first row block of every slice — rows k1 < KL = NSLICE * R2, 1/8 of the
// intermediate for n = 65536 — stays in LDS between the phases instead of going through the scratch
template <int LOGN, bool FWD, bool SCALE>
__global__ __launch_bounds__(512) CLFA_DS_SINGLE_FN void k_fft_4step(cpx *__restrict__ data, cpx *__restrict__ scratch,
                                                           const cpx *__restrict__ tabs_g, long batch, long out_off) {
  using G = FourGeom<LOGN>;
  constexpr int NSLICE = 2;        // two 256-lane slices per workgroup
  constexpr bool NT = true;        // non-temporal input loads / output stores
  constexpr bool ROWS = true, PF = true;
  constexpr int KL = NSLICE * G::R2;
  // ... and the next RRB row blocks of every slice in registers (16 VGPRs per block; the 512-lane
  // workgroup has 256 per lane): 5 of the remaining 7 for n = 65536, all of them for 32768 (3) and
  // 16384 (1), whose scratch is then never touched
  constexpr int RRB = !(ROWS && NSLICE == 2) ? 0 : LOGN == 16 ? kFourRrb16 : G::NRB / NSLICE - 1;
  constexpr int NE = RRB * NSLICE;
  constexpr int EB = G::R2 / G::T1, NIT = G::NCB / NSLICE;
  static_assert(NE == 0 || EB * NIT == 8, "a row block is 8 values per lane");
  __shared__ cpx s_tabs[G::TABS];
  __shared__ cpx s_x[NSLICE * G::SL];
  __shared__ cpx s_rows[ROWS ? KL * G::RS : 1];
  // full W_N1 / W_N2 tables for the pass twiddles of the prefetching form (no half-table sign logic)
  __shared__ cpx s_full[PF ? G::N1 + G::N2 : 1];
  const int tid = threadIdx.x;
  for (int i = tid; i < G::TABS; i += 256 * NSLICE) s_tabs[i] = tabs_g[i];
  const cpx *tlo = s_tabs + G::N1 / 2 + G::N2 / 2, *thi = tlo + G::LO;
  if constexpr (PF) {
    for (int i = tid; i < G::N1 + G::N2; i += 256 * NSLICE) {
      const bool second = i >= G::N1;
      const int k = second ? i - G::N1 : i, h = (second ? G::N2 : G::N1) / 2;
      const cpx w = tabs_g[(second ? G::N1 / 2 : 0) + (k & (h - 1))];
      s_full[i] = (k & h) ? mk(-w.x, -w.y) : w;
    }
  }
  const FullTab ftab1{s_full}, ftab2{s_full + G::N1};
  // the slice index is wave-uniform (a slice is 4 whole waves): say so, so that block indices and the
  // pointers derived from them stay in SGPRs
  const int slice = __builtin_amdgcn_readfirstlane(tid / G::SLICE), l = tid % G::SLICE;
  cpx *sx = s_x + slice * G::SL;
  cpx *mid = scratch + (long)blockIdx.x * G::N;
  __syncthreads();

  // prefetching form: the first column block of a transform is loaded behind the last row block of the
  // previous one (`vnext`), so that only the very first load of the workgroup is exposed
  cpx vnext[16];
  if constexpr (PF) four_load1<LOGN, NT ? 1 : 0>(vnext, data + xcd_first(blockIdx.x, gridDim.x) * G::N, slice, l);
#pragma unroll 1
  for (long b = xcd_first(blockIdx.x, gridDim.x); b < batch; b += gridDim.x) {
    cpx *x = data + b * (long)G::N;
    {
      // software-prefetched form: the next block's loads fly behind the current block's passes.
      // The last block of each phase is peeled so that every prefetch is straight-line code
      // (counted s_waitcnt, see k_fft_lds), and consumed at the end of the iteration.
      cpx v[16], vn[16];
      vkeep keep[NE > 0 ? NE : 1];
      int it = 0;   // the slice's column-block counter: uniform, indexes `keep`
      // consumed before the loop: otherwise the wait for these loads is merged into the loop header,
      // where it turns into vmcnt(0) on the back edge too and drains every iteration's scratch stores
#pragma unroll
      for (int e = 0; e < 16; e++) {
        asm volatile("" : "+v"(vnext[e]));
        v[e] = vnext[e];
      }
#pragma unroll 1
      for (int cb = slice; cb + NSLICE < G::NCB; cb += NSLICE) {
        int lo_ = l;   // opaque per iteration (see above)
        asm volatile("" : "+v"(lo_));
        four_load1<LOGN, NT ? 1 : 0>(vn, x, cb + NSLICE, lo_);
        four_body1<LOGN, FWD, KL, NE>(v, mid, cb, lo_, ftab1, tlo, thi, sx, s_rows, keep, it);
        it++;
#pragma unroll
        for (int e = 0; e < 16; e++) {
          asm volatile("" : "+v"(vn[e]));
          v[e] = vn[e];
        }
      }
      {
        int lo_ = l;
        asm volatile("" : "+v"(lo_));
        four_body1<LOGN, FWD, KL, NE>(v, mid, G::NCB - NSLICE + slice, lo_, ftab1, tlo, thi, sx, s_rows, keep,
                                      G::NCB / NSLICE - 1);
      }
      __syncthreads();
      if constexpr (ROWS) four_load2_rows<LOGN>(v, s_rows, slice, l);
      else four_load2<LOGN, false>(v, mid, slice, l);
#pragma unroll
      for (int e = 0; e < 16; e++) asm volatile("" : "+v"(v[e]));
      int rb0 = slice;
      if constexpr (NE > 0) {
        // Row blocks 1..RRB of each slice (rows 32.., alternating between the slices): every lane hands
        // its register-resident results over through the LDS rows the previous blocks have just left.
        // Block r+1 is dumped between the two barriers of block r-1's passes: at the first of them every
        // wave has already taken block r out of those rows (its load precedes the passes in program
        // order), the second publishes the dump — no barrier of its own except for the first block.
        auto dump = [&](auto rc) {
          constexpr int r = decltype(rc)::value;
          const int col = l % G::C1, tf = l / G::C1;
#pragma unroll
          for (int q = 0; q < NSLICE; q++) {
#pragma unroll
            for (int eb = 0; eb < EB; eb++) {
              cpx *pr = s_rows + (q * G::R2 + tf + G::T1 * eb) * G::RS + slice * G::C1 + col;
#pragma unroll
              for (int j = 0; j < NIT; j++)
                pr[j * NSLICE * G::C1] = mk(keep[NSLICE * r + q][2 * (j * EB + eb)], keep[NSLICE * r + q][2 * (j * EB + eb) + 1]);
            }
          }
        };
        __syncthreads();
        dump(std::integral_constant<int, 0>());
        __syncthreads();
        auto round = [&](auto rc) {
          constexpr int r = decltype(rc)::value;
          int lo_ = l;
          asm volatile("" : "+v"(lo_));
          four_load2_rows<LOGN>(vn, s_rows, slice, lo_);
          if constexpr (r + 1 < RRB) {
            four_body2<LOGN, FWD, SCALE, NT ? 1 : 0>(v, x + out_off, slice + NSLICE * r, lo_, ftab2, sx, nullptr,
                                                     [&]() { dump(std::integral_constant<int, r + 1>()); });
          } else {
            four_body2<LOGN, FWD, SCALE, NT ? 1 : 0>(v, x + out_off, slice + NSLICE * r, lo_, ftab2, sx);
          }
#pragma unroll
          for (int e = 0; e < 16; e++) v[e] = vn[e];
        };
        round(std::integral_constant<int, 0>());
        if constexpr (RRB > 1) round(std::integral_constant<int, 1>());
        if constexpr (RRB > 2) round(std::integral_constant<int, 2>());
        if constexpr (RRB > 3) round(std::integral_constant<int, 3>());
        if constexpr (RRB > 4) round(std::integral_constant<int, 4>());
        if constexpr (RRB > 5) round(std::integral_constant<int, 5>());
        static_assert(RRB <= 6, "unrolled by hand up to 6 rounds");
        rb0 = slice + NSLICE * RRB;
      }
#pragma unroll 1
      for (int rb = rb0; rb + NSLICE < G::NRB; rb += NSLICE) {
        int lo_ = l;
        asm volatile("" : "+v"(lo_));
        four_load2<LOGN, false>(vn, mid, rb + NSLICE, lo_);
        four_body2<LOGN, FWD, SCALE, NT ? 1 : 0>(v, x + out_off, rb, lo_, ftab2, sx);
#pragma unroll
        for (int e = 0; e < 16; e++) {
          asm volatile("" : "+v"(vn[e]));
          v[e] = vn[e];
        }
      }
      {
        int lo_ = l;
        asm volatile("" : "+v"(lo_));
        // the next transform's first column block (index clamped to the last transform: straight-line loads)
        long bn = b + gridDim.x;
        bn = bn < batch ? bn : batch - 1;
        four_load1<LOGN, NT ? 1 : 0>(vnext, data + bn * (long)G::N, slice, lo_);
        four_body2<LOGN, FWD, SCALE, NT ? 1 : 0>(v, x + out_off, G::NRB - NSLICE + slice, lo_, ftab2, sx);
      }
      __syncthreads();
    }
  }
}

// Small batches (fewer transforms than resident workgroups): one workgroup per column block,
// then one per row block — two launches, N2/C1 workgroups per transform, instead of one
// persistent workgroup walking all 32 blocks of its transform serially (86 us for batch 1).
template <int LOGN, bool FWD>
__global__ __launch_bounds__(256) void k_fft_4step_cols(const cpx *__restrict__ data, cpx *__restrict__ scratch,
                                                        const cpx *__restrict__ tabs_g) {
  using G = FourGeom<LOGN>;
  __shared__ cpx s_tabs[G::TABS];
  __shared__ cpx s_x[G::SL];
  const int tid = threadIdx.x;
  for (int i = tid; i < G::TABS; i += 256) s_tabs[i] = tabs_g[i];
  const cpx *tab1 = s_tabs, *tlo = s_tabs + G::N1 / 2 + G::N2 / 2, *thi = tlo + G::LO;
  __syncthreads();
  const long b = blockIdx.y;
  four_phase1<LOGN, FWD, 0>(data + b * (long)G::N, scratch + b * (long)G::N, blockIdx.x, tid, tab1, tlo, thi, s_x);
}
template <int LOGN, bool FWD, bool SCALE>
__global__ __launch_bounds__(256) void k_fft_4step_rows(cpx *__restrict__ data, const cpx *__restrict__ scratch,
                                                        const cpx *__restrict__ tabs_g) {
  using G = FourGeom<LOGN>;
  __shared__ cpx s_tabs[G::TABS];
  __shared__ cpx s_x[G::SL];
  const int tid = threadIdx.x;
  for (int i = tid; i < G::TABS; i += 256) s_tabs[i] = tabs_g[i];
  const cpx *tab2 = s_tabs + G::N1 / 2;
  __syncthreads();
  const long b = blockIdx.y;
  four_phase2<LOGN, FWD, SCALE, 0>(scratch + b * (long)G::N, data + b * (long)G::N, blockIdx.x, tid, tab2, s_x);
}

int fourstep_grid(const DeviceInfo &di) { return di.num_cus; }   // one 512-lane workgroup per CU

template <int LOGN, bool FWD, bool SCALE>
static hipError_t launch_4step_v(cpx *data, cpx *scratch, const FftTables &t, long batch, const DeviceInfo &di,
                                 hipStream_t s, long out_off) {
  int grid = fourstep_grid(di);
  if (fourstep_spread(batch, grid)) {
    // few transforms: spread each over its column / row blocks (scratch holds `grid` transforms)
    using G = FourGeom<LOGN>;
    hipLaunchKernelGGL((k_fft_4step_cols<LOGN, FWD>), dim3(G::NCB, (unsigned)batch), dim3(256), 0, s, data, scratch, t.four);
    hipLaunchKernelGGL((k_fft_4step_rows<LOGN, FWD, SCALE>), dim3(G::NRB, (unsigned)batch), dim3(256), 0, s, data + out_off,
                       scratch, t.four);
    return hipGetLastError();
  }
  if constexpr (LOGN == 16) {
    // n = 65536: the resident kernel (fft_resident.hip); `scratch` provides its per-workgroup slots
    return launch_fft_res16(FWD, SCALE, data, data + out_off, scratch, t.res16, batch, di, s);
  } else {
    if (batch < grid) grid = (int)batch;
    hipLaunchKernelGGL((k_fft_4step<LOGN, FWD, SCALE>), dim3(grid), dim3(512), 0, s, data, scratch, t.four, batch, out_off);
    return hipGetLastError();
  }
}

template <int LOGN>
static hipError_t launch_4step_n(bool fwd, bool scale, cpx *data, cpx *scratch, const FftTables &t, long batch,
                                 const DeviceInfo &di, hipStream_t s, long out_off) {
  if (fwd && scale) return launch_4step_v<LOGN, true, true>(data, scratch, t, batch, di, s, out_off);
  if (fwd && !scale) return launch_4step_v<LOGN, true, false>(data, scratch, t, batch, di, s, out_off);
  if (!fwd && !scale) return launch_4step_v<LOGN, false, false>(data, scratch, t, batch, di, s, out_off);
  return hipErrorInvalidValue;
}

hipError_t launch_fft_4step(int logn, bool fwd, bool scale, cpx *data, cpx *scratch, const FftTables &t, long batch,
                            const DeviceInfo &di, hipStream_t s, long out_off) {
  if (batch <= 0) return hipSuccess;
  switch (logn) {
    case 14: return launch_4step_n<14>(fwd, scale, data, scratch, t, batch, di, s, out_off);
    case 15: return launch_4step_n<15>(fwd, scale, data, scratch, t, batch, di, s, out_off);
    case 16: return launch_4step_n<16>(fwd, scale, data, scratch, t, batch, di, s, out_off);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clfa
