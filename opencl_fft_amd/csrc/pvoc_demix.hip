// pvoc_demix.hip — stereo demix by azimuth of two streams of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): the two
// inputs are the left and the right channel of one recording, every bin is placed on a signed azimuth axis of 2P + 1
// positions by the gain that cancels it best (Csound's pvsdemix, the ADRess method), the bins inside a frame's window are
// kept, and the azimuth profile — the summed magnitudes per position — can be had beside the frames.  Stateless, one launch
// per call, no atomics, no waiting between workgroups.  What a bin and a window are is pvoc_demix_bin.hpp's (two bisections
// instead of the definition's scan over the P + 1 gains); the tile kernel's prologue and launch (pvoc_bin, pvoc_tiles) and
// the in-wave moves and the fold of the tree (desc_xor, desc_fold) are pvoc_device.hpp's.
//
//   k_pvoc_demix          without the profile: a lane takes bin k of one frame, reads the pair of the left and of the right
//                         input and writes one pair; rows of consecutive bins, 16 bytes in and 8 out per lane, no LDS.  A bin
//                         outside the range needs its side alone (the freq it passes on) and is not scanned.
//   k_pvoc_demix_az<LOGM> with the profile: a workgroup of 256 lanes takes whole frames, one at a time.  Phase 1 is the
//                         kernel above, bins tid, tid + 256, ..., and leaves (u, mag) of every bin in LDS — 8 bytes a bin,
//                         64 KiB at M = 8192, two workgroups a CU — where a bin that is not placed or lies outside the range
//                         has a u no column asks for.  Phase 2 forms the 2P + 1 columns, each the descriptors' TREE SUM of
//                         the frame's terms: the columns are dealt over the four waves in blocks of four.  A wave walks the
//                         frame once per block; lane l holds the tree's p[Q l .. Q l + Q - 1] of each of the four columns
//                         (Q = W / 64 positions a lane, W = min(M, 256)), a term being mag where the bin's u is the column's
//                         and +0 elsewhere.  The tree's first levels are then the lane's own additions ((p0 + p1) + (p2 +
//                         p3)), at the levels of 1 and 2 lanes the lane and its partner split the four columns (k_pvoc_desc's
//                         fold), and the levels of 4 to 32 lanes work on the one column left.  Lanes 0..3 add the Nyquist
//                         term and store a column each.  Every term is >= +0, so a lane that has no bin adds +0 and changes
//                         nothing (W = 32: the upper half of the wave).  Each input frame is read once, each output written
//                         once.
//
// Every float32 step of the definition is rounded on its own: contraction is off in every function below.
// tests/pvoc_demix_model.py restates it.
#include "pvoc_demix_bin.hpp"
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kDemixWG = 256;               // lanes = bins per tile (k_pvoc_demix), lanes of a frame's workgroup (k_pvoc_demix_az)
constexpr int kDemixCols = 4;               // columns a wave forms at a time
constexpr int kDemixNoColumn = 0x7fffffff;  // the u of a bin that enters no column

// the output pair of a bin, and what it adds to the profile: (u, mag), u = kDemixNoColumn where it adds nothing
struct DemixOut {
  cpx pair;
  int u;
  float mag;
};
__device__ __forceinline__ DemixOut demix_out(cpx a, cpx b, int P, bool inrange, DemixWindow w) {
  DemixOut o;
  DemixBin r;
  if (inrange) {
    r = demix_bin(a.x, b.x, P);
  } else {
    r.left = a.x > b.x;
    r.placed = false;
    r.u = 0;
    r.mag = 0.f;
  }
  const bool kept = r.placed && demix_inside(w, r.u);
  o.pair = mk(kept ? r.mag : 0.f, r.left ? a.y : b.y);   // the freq: the bits of the loud side's
  o.u = r.placed ? r.u : kDemixNoColumn;
  o.mag = r.placed ? r.mag : 0.f;
  return o;
}

}  // namespace

// item -> (channel, frame f, bin tile), the tile fastest.  par: F rows of (pos, width).  l and r may be one buffer
__global__ __launch_bounds__(kDemixWG) void k_pvoc_demix(const cpx *l, const cpx *r, cpx *__restrict__ out, const float *par,
                                                         long F, int M, int tiles, long items, int P, int lo, int hi) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long f, c;
    if (!pvoc_bin<kDemixWG>(item, tiles, F, M, k, f, c)) continue;
    const long e = (c * F + f) * (M + 1) + k;
    const DemixWindow w = demix_window(par[2 * f], par[2 * f + 1], P);
    out[e] = demix_out(l[e], r[e], P, k >= lo && k <= hi, w).pair;
  }
}

// grid-stride over the channels x F frames (frame index c * F + f; the frames are contiguous).  az: nframes x (2P + 1)
template <int LOGM>
__global__ __launch_bounds__(kDemixWG) void k_pvoc_demix_az(const cpx *l, const cpx *r, cpx *__restrict__ out, const float *par,
                                                            float *__restrict__ az, long F, long nframes, int P, int lo,
                                                            int hi) {
#pragma clang fp contract(off)
  constexpr int M = 1 << LOGM, B = M + 1, W = M < 256 ? M : 256, ROWS = M / W, Q = W >= 64 ? W / 64 : 1;
  static_assert(Q == 1 || Q == 2 || Q == 4, "positions of the tree a lane holds");
  __shared__ __attribute__((aligned(16))) int s_u[B + 3];
  __shared__ __attribute__((aligned(16))) float s_mag[B + 3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ncol = 2 * P + 1;
#pragma unroll 1
  for (long fr = blockIdx.x; fr < nframes; fr += gridDim.x) {
    const long f = fr % F;
    const DemixWindow w = demix_window(par[2 * f], par[2 * f + 1], P);
    // phase 1: the frames, and (u, mag) of every bin
#pragma unroll 1
    for (int k = tid; k <= M; k += kDemixWG) {
      const long e = fr * B + k;
      const DemixOut o = demix_out(l[e], r[e], P, k >= lo && k <= hi, w);
      out[e] = o.pair;
      s_u[k] = o.u;
      s_mag[k] = o.mag;
    }
    __syncthreads();
    // phase 2: the columns j0 .. j0 + 3 of this wave's blocks
    const bool holds = W >= 64 || lane < W;   // the lane holds positions of the tree
    const int un = s_u[M];
    const float magn = s_mag[M];
#pragma unroll 1
    for (int j0 = wave * kDemixCols; j0 < ncol; j0 += (kDemixWG / 64) * kDemixCols) {
      float acc[kDemixCols][Q];
#pragma unroll
      for (int i = 0; i < kDemixCols; i++)
#pragma unroll
        for (int q = 0; q < Q; q++) acc[i][q] = 0.f;
      // step 1 of the tree: p[Q lane + q] over the bins Q lane + q, + W, ... < M, ascending (0 + t = t: every t >= +0)
      if (holds) {
#pragma unroll 4
        for (int row = 0; row < ROWS; row++) {
          const int k0 = row * W + lane * Q;
          int u[Q];
          float m[Q];
          if constexpr (Q == 4) {
            const int4 uu = *(const int4 *)&s_u[k0];
            const float4 mm = *(const float4 *)&s_mag[k0];
            u[0] = uu.x, u[1] = uu.y, u[2] = uu.z, u[3] = uu.w;
            m[0] = mm.x, m[1] = mm.y, m[2] = mm.z, m[3] = mm.w;
          } else if constexpr (Q == 2) {
            const int2 uu = *(const int2 *)&s_u[k0];
            const float2 mm = *(const float2 *)&s_mag[k0];
            u[0] = uu.x, u[1] = uu.y;
            m[0] = mm.x, m[1] = mm.y;
          } else {
            u[0] = s_u[k0];
            m[0] = s_mag[k0];
          }
#pragma unroll
          for (int i = 0; i < kDemixCols; i++)
#pragma unroll
            for (int q = 0; q < Q; q++) acc[i][q] = acc[i][q] + (u[q] == j0 + i - P ? m[q] : 0.f);
        }
      }
      // step 2: adjacent pairs first.  The lane's own positions, then the lanes
      float V[kDemixCols];
#pragma unroll
      for (int i = 0; i < kDemixCols; i++) {
        if constexpr (Q == 4) {
          const float s01 = acc[i][0] + acc[i][1], s23 = acc[i][2] + acc[i][3];
          V[i] = s01 + s23;
        } else if constexpr (Q == 2) {
          V[i] = acc[i][0] + acc[i][1];
        } else {
          V[i] = acc[i][0];
        }
      }
      desc_fold<1, 4>(V, lane & 1);
      desc_fold<2, 2>(V, lane & 2);
      float v = V[0];   // of column j0 + bitrev2(lane & 3)
      v = v + desc_xor<4>(v);
      v = v + desc_xor<8>(v);
      v = v + desc_xor<16>(v);
      v = v + desc_xor<32>(v);
      // step 3: the Nyquist bin last
      const int j = j0 + desc_bitrev2(lane & 3);
      if (lane < kDemixCols && j < ncol) az[fr * ncol + j] = v + (un == j - P ? magn : 0.f);
    }
    __syncthreads();   // the frame is out of LDS before the next one lands there
  }
}

template <int LOGM>
static hipError_t launch_pvoc_demix_az(const PvocDemixArgs &a, const DeviceInfo &di, hipStream_t s) {
  constexpr int lds = 8 * ((1 << LOGM) + 4);   // bytes a workgroup: what fits a CU's 160 KiB, at most 8
  const int per_cu = 160 * 1024 / lds < 8 ? 160 * 1024 / lds : 8;
  const long nframes = (long)a.channels * a.F;
  const int grid = pvoc_grid(nframes, (long)di.num_cus * per_cu, a.grid_max);
  hipLaunchKernelGGL((k_pvoc_demix_az<LOGM>), dim3(grid), dim3(kDemixWG), 0, s, a.l, a.r, a.out, a.par, a.az, a.F, nframes,
                     a.points, a.lo, a.hi);
  return hipGetLastError();
}

hipError_t launch_pvoc_demix(const PvocDemixArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.lo < 0 || a.lo > a.hi || a.hi > a.M || a.points < 1 || a.points > kDemixPointsMax) return hipErrorInvalidValue;
  if (!a.az) {
    const PvocTiles t = pvoc_tiles(a.M, kDemixWG, (long)a.channels * a.F, di, 16, a.grid_max);
    hipLaunchKernelGGL(k_pvoc_demix, dim3(t.grid), dim3(kDemixWG), 0, s, a.l, a.r, a.out, a.par, a.F, a.M, t.tiles, t.items,
                       a.points, a.lo, a.hi);
    return hipGetLastError();
  }
  if (a.M != 1 << a.logn) return hipErrorInvalidValue;
  switch (a.logn) {
    case 5: return launch_pvoc_demix_az<5>(a, di, s);
    case 6: return launch_pvoc_demix_az<6>(a, di, s);
    case 7: return launch_pvoc_demix_az<7>(a, di, s);
    case 8: return launch_pvoc_demix_az<8>(a, di, s);
    case 9: return launch_pvoc_demix_az<9>(a, di, s);
    case 10: return launch_pvoc_demix_az<10>(a, di, s);
    case 11: return launch_pvoc_demix_az<11>(a, di, s);
    case 12: return launch_pvoc_demix_az<12>(a, di, s);
    case 13: return launch_pvoc_demix_az<13>(a, di, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clfa
