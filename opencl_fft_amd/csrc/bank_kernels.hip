// bank_kernels.hip — the filter bank on a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): per frame a vector
// of band energies (mel, bark, any bank of weighted bands), their log, and a DCT of that (the cepstral coefficients).
// Many short sums of very different lengths per frame, each the header's S16 — the descriptors' TREE SUM at a width
// that fits a band — so the bits do not depend on the grid, on how the stream is cut into calls, on the run length or on
// which row of lanes takes which band.  No atomics, no waiting between workgroups.  The moves and the fold of the tree
// are tree_moves.hpp's, shared with pvoc_desc.hip and pvoc_demix.hip; nothing else is shared with those files.
//
//   k_pvoc_bands<R>  a workgroup of 256 lanes takes a run of R consecutive frames of one channel (R = 8 up to M = 512,
//                    then 4, 2, 1: about 16 KiB of LDS, 32 KiB at M = 8192, several workgroups a CU) and puts their amps
//                    — squared where POWER is set, the freq column dropped on the way in — into LDS, a frame after the
//                    other.  The workgroup is sixteen rows of 16 lanes; a row takes a band at a time, by the schedule
//                    the setup computed (bank_plan.hpp: longest first, so the four rows of a wave walk bands of similar
//                    length; the workgroup copies the bands into LDS in that order once, for all its items).  Lane j
//                    of the row walks i = j, j + 16, ...: one weight from cache for the whole run, R
//                    amps from LDS, R accumulators — p[j] of the R sums.  The rows of a half wave read 16 neighbouring
//                    words each at unrelated offsets: a ds_read_b32 is served in halves of 32 lanes over 32 banks, so
//                    two rows share banks unless they lie 16 words apart, twice the cycles at worst.
//                    Then the tree: with R > 1 a lane and its partner split the R sums at the first log2 R levels
//                    (desc_fold), and the remaining levels work on the one value left; lane l < R of the row ends up
//                    with the sum of frame bitrev(l).  E goes to LDS; after a barrier the log (in place), and either
//                    the row's store or, after another barrier, the DCT: a lane per (frame, q), a serial sum over b
//                    with v from LDS (a broadcast) and D, stored transposed, from cache.
//
// Every float32 step of the definition is rounded on its own: contraction is off in every function below.
// tests/pvoc_bank_model.py restates it.
#include "bank_launch.hpp"
#include "tree_moves.hpp"

namespace clfa {

namespace {

constexpr int kBankWG = 256;     // lanes of a workgroup
constexpr int kBankRows = 16;    // rows of kBankLanes lanes (bank_plan.hpp's)
constexpr int kBankLanes = 16;

// The tree of S16 on the R partial sums a lane holds (V[i]: p[j] of frame i of the run).  Returns the row's sum of frame
// `frame`, which every lane of the row with the same low log2 R bits holds
template <int R>
__device__ __forceinline__ float bank_tree(float (&V)[R], int lane, int &frame) {
#pragma clang fp contract(off)
  static_assert(R == 1 || R == 2 || R == 4 || R == 8, "a run");
  float v;
  if constexpr (R == 8) {
    desc_fold<1, 8>(V, lane & 1);
    desc_fold<2, 4>(V, lane & 2);
    desc_fold<4, 2>(V, lane & 4);
    v = V[0];
    frame = ((lane & 1) << 2) | (lane & 2) | ((lane >> 2) & 1);
  } else if constexpr (R == 4) {
    desc_fold<1, 4>(V, lane & 1);
    desc_fold<2, 2>(V, lane & 2);
    v = V[0];
    v = v + desc_xor<4>(v);
    frame = desc_bitrev2(lane & 3);
  } else if constexpr (R == 2) {
    desc_fold<1, 2>(V, lane & 1);
    v = V[0];
    v = v + desc_xor<2>(v);
    v = v + desc_xor<4>(v);
    frame = lane & 1;
  } else {
    v = V[0];
    v = v + desc_xor<1>(v);
    v = v + desc_xor<2>(v);
    v = v + desc_xor<4>(v);
    frame = 0;
  }
  return v + desc_xor<8>(v);
}

}  // namespace

// what the kernel is handed: BankArgs with the run's counts
struct BankKernelArgs {
  const cpx *in;
  float *out;
  const int4 *bands;
  const int *sched;
  const float *weights, *dct_t;
  long F, runs, items;
  int M, B, steps, power, log, dct, ncoef;
  float floor;
};

// item -> (channel c, run r of R frames).  Dynamic LDS: the B bands in the schedule's order (16 bytes each), R (M + 1)
// floats of amps, then R B floats of E / v
template <int R>
__global__ __launch_bounds__(kBankWG) void k_pvoc_bands(const BankKernelArgs a) {
#pragma clang fp contract(off)
  extern __shared__ int4 s_meta[];   // the bands in the schedule's order: first, count, woff, band number
  const int tid = threadIdx.x, row_id = tid / kBankLanes, j = tid & (kBankLanes - 1);
  const int row = a.M + 1, B = a.B;
  float *s_x = (float *)(s_meta + B), *s_e = s_x + R * row;
  const int n0 = a.sched[row_id], n1 = a.sched[row_id + 1];   // the row's bands
  // once per workgroup: what the passes below would else fetch from memory in a chain (list -> band -> weights) per item
  for (int n = tid; n < B; n += kBankWG) {
    const int b = a.sched[kBankRows + 1 + n];
    int4 m = a.bands[b];
    m.w = b;
    s_meta[n] = m;
  }
#pragma unroll 1
  for (long item = blockIdx.x; item < a.items; item += gridDim.x) {
    const long c = item / a.runs, r = item - c * a.runs;
    const long f0 = r * R;
    const int nf = (int)(a.F - f0 < R ? a.F - f0 : R);   // frames of the run, >= 1
    const cpx *ic = a.in + (c * a.F + f0) * row;
    // the amps of the run (their squares with POWER); +0 for the frames a ragged run lacks
#pragma unroll
    for (int i = 0; i < R; i++) {
      if (i < nf) {
#pragma unroll 4
        for (int k = tid; k < row; k += kBankWG) {
          const float x = ic[(long)i * row + k].x;
          s_x[i * row + k] = a.power ? x * x : x;
        }
      } else {
        for (int k = tid; k < row; k += kBankWG) s_x[i * row + k] = 0.f;
      }
    }
    __syncthreads();
    // the bands: every row makes a.steps passes (the longest list), idling where its own list has ended, so the moves
    // of the tree are made by whole waves
#pragma unroll 1
    for (int n = 0; n < a.steps; n++) {
      const bool has = n0 + n < n1;
      const int4 band = s_meta[has ? n0 + n : 0];
      const int b = band.w, count = has ? band.y : 0;
      const float *w = a.weights + band.z;
      const float *x = s_x + band.x;
      float V[R];
#pragma unroll
      for (int f = 0; f < R; f++) V[f] = 0.f;
      if (j < count) {   // p[j] starts as t[j], the bits: -0 stays -0
        const float wj = w[j];
#pragma unroll
        for (int f = 0; f < R; f++) V[f] = x[f * row + j] * wj;
      }
#pragma unroll 4
      for (int i = j + kBankLanes; i < count; i += kBankLanes) {
        const float wi = w[i];
#pragma unroll
        for (int f = 0; f < R; f++) {
          const float t = x[f * row + i] * wi;
          V[f] = V[f] + t;
        }
      }
      int frame;
      const float e = bank_tree<R>(V, j, frame);
      if (has && j < R) s_e[frame * B + b] = e;
    }
    __syncthreads();
    float *orow = a.out + (c * a.F + f0) * (a.dct ? a.ncoef : B);
    if (!a.dct) {
#pragma unroll 1
      for (int e = tid; e < nf * B; e += kBankWG) {
        float v = s_e[e];
        if (a.log) v = logf(fmaxf(v, a.floor));   // a NaN takes the floor
        orow[e] = v;
      }
    } else {
      if (a.log) {
#pragma unroll 1
        for (int e = tid; e < nf * B; e += kBankWG) s_e[e] = logf(fmaxf(s_e[e], a.floor));
        __syncthreads();
      }
#pragma unroll 1
      for (int e = tid; e < nf * a.ncoef; e += kBankWG) {
        const int f = e / a.ncoef, q = e - f * a.ncoef;
        const float *v = s_e + f * B;
        float acc = 0.f;
#pragma unroll 8
        for (int b = 0; b < B; b++) {
          const float t = a.dct_t[b * B + q] * v[b];
          acc = acc + t;
        }
        orow[e] = acc;
      }
    }
    __syncthreads();   // the run is read before the next item's lands in LDS
  }
}

template <int R>
static hipError_t launch_pvoc_bands_r(const BankArgs &a, const DeviceInfo &di, hipStream_t s) {
  BankKernelArgs k;
  k.in = a.in;
  k.out = a.out;
  k.bands = (const int4 *)a.bands;
  k.sched = a.sched;
  k.weights = a.weights;
  k.dct_t = a.dct_t;
  k.F = a.F;
  k.runs = (a.F + R - 1) / R;
  k.items = k.runs * a.channels;
  k.M = a.M;
  k.B = a.B;
  k.steps = a.steps;
  k.power = a.power;
  k.log = a.log;
  k.dct = a.dct;
  k.ncoef = a.ncoef;
  k.floor = a.floor;
  long cap = (long)di.num_cus * 8;
  if (a.grid_max > 0 && cap > a.grid_max) cap = a.grid_max;
  const int grid = (int)(k.items < cap ? k.items : cap);
  const size_t lds = sizeof(int4) * a.B + sizeof(float) * ((size_t)R * (a.M + 1) + (size_t)R * a.B);
  hipLaunchKernelGGL((k_pvoc_bands<R>), dim3(grid), dim3(kBankWG), lds, s, k);
  return hipGetLastError();
}

hipError_t launch_pvoc_bands(const BankArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.B < 1 || a.B > 256 || a.steps < 1 || a.M < 1 || (a.dct && (a.ncoef < 1 || a.ncoef > a.B))) return hipErrorInvalidValue;
  if (a.M <= 512) return launch_pvoc_bands_r<8>(a, di, s);
  if (a.M <= 1024) return launch_pvoc_bands_r<4>(a, di, s);
  if (a.M <= 2048) return launch_pvoc_bands_r<2>(a, di, s);
  return launch_pvoc_bands_r<1>(a, di, s);
}

}  // namespace clfa
