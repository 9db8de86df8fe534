// pvoc_desc.hip — per-frame descriptors of a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): magnitude,
// power, moment, centroid, flux and peak of a range of bins, eight float32 per frame.  The first parallel float sums of
// the Pvoc code: the header fixes their TREE SUM (which lanes' values meet in which addition), and the kernel is written
// to it, so the bits do not depend on the grid, on how the stream is cut into calls or on the run length.  No atomics, no
// waiting between workgroups.  The group kernels' item (which run a group of W lanes takes) and launch are
// pvoc_device.hpp's, shared with pvoc_trace.hip, and so are the in-wave moves and the fold of the tree (desc_dpp, desc_xor,
// desc_fold), shared with pvoc_demix.hip; the state's commit is pvoc_time.hip's k_pvoc_tail.
//
//   k_pvoc_desc<W>  W = min(M, 256) lanes form a group, lane j holding the tree's p[j]; 256 / W groups share a workgroup.
//                   A group takes a run of kDescRun = 4 consecutive frames of one channel and walks the bins outermost,
//                   k = j, j + W, ...: for each k it loads the run's amps and the amp of the frame before the run (from
//                   the input, or from the state for the call's first frame), so the input is read 5 / 4 times and the
//                   flux's prev lives in a register; 4 partial sums and a peak per frame stay in registers.  Bins outside
//                   the range are not loaded: their terms are +0.
//                   Then the tree.  A lane holds 16 partial sums (4 frames x 4 sums).  At the levels of 1, 2, 4 and 8
//                   lanes the lane and its partner (lane ^ 1, ^ 2, ^ 4, ^ 8) split what they hold: each keeps one half,
//                   sends the other and adds what it receives to what it keeps, so that 8 + 4 + 2 + 1 additions do what
//                   16 a level would, and after four levels lane l holds the sum over its row of 16 lanes of value
//                   number bitrev4(l & 15).  The additions are those of the tree: partial sums of adjacent groups of 1, 2,
//                   4, 8 lanes, and float addition is commutative.  The levels of 16 and 32 lanes and the 2 or 4 waves
//                   of a group (through LDS, 80 B a wave) then work on that one value, every lane ending up with the
//                   group's sum.  The four peaks are folded in the same way over the first two levels (a peak's order is
//                   total: larger amp, then lower bin, so any pairing gives the same answer).  Moves: quad_perm for ^ 1
//                   and ^ 2, ds_swizzle for ^ 4 and ^ 16, row_ror:8 for ^ 8, ds_bpermute for ^ 32.
//                   A quad then holds the four sums of one frame; lanes 0, 5, 10, 15 of the group take a frame each, add
//                   the Nyquist terms, divide, fetch the peak's pair and store the row.  The launch only reads the state.
//
// Every float32 step of the definition is rounded on its own: contraction is off in every function below.
// tests/pvoc_desc_model.py restates it.
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kDescWG = kGroupWG;   // lanes of a workgroup = the largest W
constexpr int kDescRun = 4;     // consecutive frames per run
constexpr int kDescSums = 4;    // mag, pow, mom, flux
constexpr int kDescVals = kDescRun * kDescSums;
static_assert(kDescRun == 4 && kDescVals == 16, "the fold below ends with a frame's four sums in a quad");

// a peak: bin k (-1: none yet) and its amp, never a NaN.  The better of two: the larger amp, the lower bin on a tie
struct DescPeak {
  float a;
  int k;
};
__device__ __forceinline__ DescPeak desc_better(DescPeak p, DescPeak o) {
  const bool take = o.k >= 0 && (p.k < 0 || o.a > p.a || (o.a == p.a && o.k < p.k));   // -0 == +0
  return take ? o : p;
}
using clfa::desc_xor;   // pvoc_device.hpp's, for a float: the overload below would hide it
template <int STEP>
__device__ __forceinline__ DescPeak desc_xor(DescPeak p) {
  DescPeak o;
  o.a = desc_xor<STEP>(p.a);
  o.k = desc_xor_bits<STEP>(p.k);
  return o;
}

// one level of the fold (pvoc_device.hpp's desc_fold, the sums') on the N peaks the lane still holds
using clfa::desc_fold;
template <int STEP, int N>
__device__ __forceinline__ void desc_fold(DescPeak (&P)[kDescRun], bool up) {
#pragma unroll
  for (int i = 0; i < N / 2; i++) {
    const DescPeak keep = up ? P[i + N / 2] : P[i], send = up ? P[i] : P[i + N / 2];
    P[i] = desc_better(keep, desc_xor<STEP>(send));
  }
}
// one level on a single value, every lane of the two groups ending up with their sum
template <int STEP>
__device__ __forceinline__ void desc_level(float &v, DescPeak &p) {
#pragma clang fp contract(off)
  v = v + desc_xor<STEP>(v);
  p = desc_better(p, desc_xor<STEP>(p));
}

}  // namespace

// item -> (channel c, group of G runs); group g of the workgroup takes run rg G + g.  last: channels x (M + 1) pairs,
// only the amps read.  desc: channels x F x 8
template <int W>
__global__ __launch_bounds__(kDescWG) void k_pvoc_desc(const cpx *__restrict__ in, const cpx *__restrict__ last,
                                                       float *__restrict__ desc, long F, int M, int lo, int hi, int rectify,
                                                       float cf, long runs, long rgroups, long items) {
#pragma clang fp contract(off)
  constexpr int R = kDescRun, WAVES = W > 64 ? W / 64 : 1;
  __shared__ float s_sum[kDescWG / 64][kDescVals];
  __shared__ DescPeak s_peak[kDescWG / 64][R];
  const int tid = threadIdx.x;
  const long row = M + 1;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int g, j;
    long r, c;
    pvoc_group_row<W>(item, rgroups, g, j, r, c);
    const long f0 = r * R;
    const int nf = r < runs ? (int)(F - f0 < R ? F - f0 : R) : 0;   // frames of the run; 0: the group idles along
    const float *ic = (const float *)(in + c * F * row);              // the channel's amps, 2 floats apart
    const float *lc = (const float *)(last + c * row);
    float V[kDescVals];   // V[q R + i]: sum q of frame f0 + i
    DescPeak P[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
      P[i].a = 0.f;
      P[i].k = -1;
    }
#pragma unroll
    for (int n = 0; n < kDescVals; n++) V[n] = 0.f;
    // step 1 of the tree: lane j's p[j] over the bins j, j + W, ... < M, ascending
#pragma unroll 1
    for (int k = j; k < M; k += W) {
      const bool sel = k >= lo && k <= hi;
      float a[R + 1];   // a[0]: the frame before the run; what is not loaded is +0, and so are its terms
      a[0] = 0.f;
      if (sel && nf > 0) a[0] = f0 > 0 ? ic[2 * ((f0 - 1) * row + k)] : lc[2 * k];
#pragma unroll
      for (int i = 0; i < R; i++) {
        a[i + 1] = 0.f;
        if (sel && i < nf) a[i + 1] = ic[2 * ((f0 + i) * row + k)];
      }
      const float w = (float)k * cf;
      const bool first = k == j;
#pragma unroll
      for (int i = 0; i < R; i++) {
        const float x = a[i + 1];
        float d = x - a[i];
        if (rectify) d = d > 0.f ? d : 0.f;   // a NaN is dropped
        const float t[kDescSums] = {x, x * x, x * w, d * d};
#pragma unroll
        for (int q = 0; q < kDescSums; q++) {
          const float sum = V[q * R + i] + t[q];
          V[q * R + i] = first ? t[q] : sum;
        }
        if (sel && x == x && (P[i].k < 0 || x > P[i].a)) {   // ascending k: a tie keeps the lower bin
          P[i].a = x;
          P[i].k = k;
        }
      }
    }
    // step 2: adjacent pairs first.  After the four folds lane l holds, of its row of 16 lanes, sum bitrev2(l & 3) of
    // frame bitrev2((l >> 2) & 3); after the two folds of the peaks, the peak of frame bitrev2(l & 3) of its quad
    desc_fold<1, 16>(V, tid & 1);
    desc_fold<2, 8>(V, tid & 2);
    desc_fold<4, 4>(V, tid & 4);
    desc_fold<8, 2>(V, tid & 8);
    desc_fold<1, 4>(P, tid & 1);
    desc_fold<2, 2>(P, tid & 2);
    float v = V[0];
    DescPeak p = P[0];
    p = desc_better(p, desc_xor<4>(p));
    p = desc_better(p, desc_xor<8>(p));
    desc_level<16>(v, p);
    if constexpr (W >= 64) desc_level<32>(v, p);
    if constexpr (WAVES > 1) {
      const int wave = tid / 64, l = tid & 63;
      if (l < kDescVals) s_sum[wave][l] = v;
      if (l < R) s_peak[wave][l] = p;
      __syncthreads();
      const int b = g * WAVES;   // the group's first wave
      const float s01 = s_sum[b][tid & 15] + s_sum[b + 1][tid & 15];
      p = desc_better(s_peak[b][tid & 3], s_peak[b + 1][tid & 3]);
      if constexpr (WAVES == 4) {
        const float s23 = s_sum[b + 2][tid & 15] + s_sum[b + 3][tid & 15];
        v = s01 + s23;
        p = desc_better(p, desc_better(s_peak[b + 2][tid & 3], s_peak[b + 3][tid & 3]));
      } else {
        v = s01;
      }
      __syncthreads();   // the exchange is read before the next item's lands in it
    }
    // a quad holds the four sums of its frame: mag at its lane 0, mom at 1, pow at 2, flux at 3
    const float smag = __builtin_bit_cast(float, desc_dpp<0x00>(__builtin_bit_cast(int, v)));
    const float smom = __builtin_bit_cast(float, desc_dpp<0x55>(__builtin_bit_cast(int, v)));
    const float spow = __builtin_bit_cast(float, desc_dpp<0xAA>(__builtin_bit_cast(int, v)));
    const float sflux = __builtin_bit_cast(float, desc_dpp<0xFF>(__builtin_bit_cast(int, v)));
    // step 3 and the row: the lane of quad m at position m holds the sums and the peak of frame bitrev2(m)
    const int fi = desc_bitrev2(j & 3);
    if (j < 16 && (j >> 2) == (j & 3) && fi < nf) {
      const long f = f0 + fi;
      float x = 0.f, d = 0.f;   // the Nyquist bin's terms, +0 outside the range
      if (hi == M) {
        x = ic[2 * (f * row + M)];
        d = x - (f > 0 ? ic[2 * ((f - 1) * row + M)] : lc[2 * M]);
        if (rectify) d = d > 0.f ? d : 0.f;
        if (x == x && (p.k < 0 || x > p.a)) {
          p.a = x;
          p.k = M;
        }
      }
      const float w = (float)M * cf;
      const float mag = smag + x, pw = spow + x * x, mom = smom + x * w, flux = sflux + d * d;
      const float q = mom / mag;
      float *orow = desc + (c * F + f) * 8;
      orow[0] = mag;
      orow[1] = pw;
      orow[2] = mom;
      orow[3] = mag == 0.f ? 0.f : q;
      orow[4] = flux;
      const float *pair = ic + 2 * (f * row + (p.k < 0 ? 0 : p.k));
      orow[5] = p.k < 0 ? 0.f : pair[0];   // the bits of the peak's pair
      orow[6] = p.k < 0 ? 0.f : pair[1];
      orow[7] = (float)p.k;
    }
  }
}

template <int W>
static hipError_t launch_pvoc_desc_w(const PvocDescArgs &a, const DeviceInfo &di, hipStream_t s) {
  const long runs = (a.F + kDescRun - 1) / kDescRun;
  const PvocGroups q = pvoc_groups<W>(runs, a.channels, di, a.grid_max);
  hipLaunchKernelGGL((k_pvoc_desc<W>), dim3(q.grid), dim3(kDescWG), 0, s, a.in, a.last, a.desc, a.F, a.M, a.lo, a.hi,
                     a.rectify, a.cf, runs, q.rgroups, q.items);
  return hipGetLastError();
}

hipError_t launch_pvoc_desc(const PvocDescArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.lo < 0 || a.lo > a.hi || a.hi > a.M) return hipErrorInvalidValue;
  hipError_t e;
  switch (pvoc_group_lanes(a.M)) {
    case 32: e = launch_pvoc_desc_w<32>(a, di, s); break;
    case 64: e = launch_pvoc_desc_w<64>(a, di, s); break;
    case 128: e = launch_pvoc_desc_w<128>(a, di, s); break;
    case 256: e = launch_pvoc_desc_w<256>(a, di, s); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  // the state's commit, on the same stream: the amps (and freqs) of the call's last frame, every bin
  return launch_pvoc_time_last(a.in, a.F, a.last, a.channels, a.M, a.grid_max, di, s);
}

}  // namespace clfa
