// pvoc_kernels.hip — phase vocoder on the packed spectra of Stft (clfa_pvoc, include/clfft_amd.h).
//
//   k_pvoc_analyze  one launch per call: a lane takes bin k of a run of kPvocRun consecutive frames of one channel; the
//                   frame before the run is read again (from cache: the neighbouring workgroup has just read it), the
//                   frame before the call's first comes from the state.  The lanes of frame 0 are the only ones that
//                   touch the state: they read it, then replace it with z of the call's last frame.
//   k_pvoc_sums     synthesis, launch 1: per (channel, chunk of kPvocChunk frames, bin) the sum of the frames' phase
//                   increments (uint32, units of 2^-32 turn);
//   k_pvoc_scan     launch 2, small: per (channel, bin) the chunks' sums become their bases in place (the state plus the
//                   sums of the chunks before), and the state takes the call's total: the scan of pvoc_device.hpp, which
//                   the oscillator bank shares (k_adsyn_scan, pvoc_adsyn.hip);
//   k_pvoc_walk     launch 3: every chunk starts from its base and walks its frames, writing spectra.
//
// The phases are integers, and integer addition is associative: the chunked sums are the bits of the serial sum, for every
// chunk length, sub-batch and split of a stream into calls.  No atomics, no waiting between workgroups.
//
// Every global access is a row of consecutive bins: 8 bytes per lane (a complex bin, or an (amp, freq) pair), 4 in the
// sums and bases.
#include "pvoc_analysis.hpp"
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kPvocWG = 256;    // lanes = bins per workgroup tile
constexpr int kPvocRun = 4;     // consecutive frames per lane of the analysis

// the phase increment of one frame in 2^-32 turn.  Every step rounds on its own: tests/pvoc_model.py restates it bit for
// bit.  The pragma is what keeps the product and the subtraction apart — HIP's __fmul_rn / __fsub_rn are plain operators,
// which hipcc's default contraction fuses into one fma.  r is a float in [-1/2, 1/2], so r * 2^32 is exact in double and
// |.| <= 2^31.
__device__ __forceinline__ unsigned pvoc_inc(float freq, float kf) {
#pragma clang fp contract(off)
  const float t = freq * kf;
  const float r = t - rintf(t);
  if (!(fabsf(r) <= 0.5f)) return 0u;   // a non-finite freq (or freq * kf): the phase stays
  return (unsigned)(long long)rint((double)r * 4294967296.0);
}

}  // namespace

__global__ __launch_bounds__(kPvocWG) void k_pvoc_analyze(const cpx *__restrict__ spec, float *__restrict__ frames,
                                                          cpx *prev, const cpx *__restrict__ etab, long F, int M,
                                                          long groups, int tiles, long items, float sh, float srs) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int tile;
    long g, c;
    pvoc_item(item, tiles, groups, tile, g, c);
    const int k = tile * kPvocWG + (int)threadIdx.x;
    if (k > M) continue;
    const long f0 = g * kPvocRun, f1 = f0 + kPvocRun < F ? f0 + kPvocRun : F;
    const cpx *rows = spec + c * F * M;
    cpx *state = prev + c * (M + 1) + k;
    const cpx e = etab[k];
    cpx zp = f0 == 0 ? *state : pvoc_bin(rows + (f0 - 1) * M, k, M);
    cpx *out = reinterpret_cast<cpx *>(frames) + (c * F + f0) * (M + 1) + k;
    for (long f = f0; f < f1; f++, out += M + 1) {
      const cpx z = pvoc_bin(rows + f * M, k, M);
#include "pvoc_analysis_bin.inc"   // amp and freq of bin k from z, zp and e: the one copy k_pvoc_tanal shares
      *out = mk(amp, freq);
      zp = z;
    }
    if (f0 == 0) *state = pvoc_bin(rows + (F - 1) * M, k, M);
  }
}

// frames: the sub-batch's first frame of channel 0 (channel c at c * cstride pairs); nf frames in nch chunks
__global__ __launch_bounds__(kPvocWG) void k_pvoc_sums(const cpx *__restrict__ frames, long cstride, long nf, int M,
                                                       long nch, int tiles, long items, float kf,
                                                       unsigned *__restrict__ sums) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int tile;
    long j, c;
    pvoc_item(item, tiles, nch, tile, j, c);
    const int k = tile * kPvocWG + (int)threadIdx.x;
    if (k > M) continue;
    const long f0 = j * kPvocChunk, f1 = f0 + kPvocChunk < nf ? f0 + kPvocChunk : nf;
    const cpx *in = frames + c * cstride + f0 * (M + 1) + k;
    unsigned s = 0;
    for (long f = f0; f < f1; f++, in += M + 1) s += pvoc_inc(in->y, kf);
    sums[(c * nch + j) * (M + 1) + k] = s;
  }
}

// one workgroup per (channel, tile of kScanBins bins), kScanBins x kScanSegs lanes
__global__ __launch_bounds__(kScanBins *kScanSegs) void k_pvoc_scan(unsigned *__restrict__ sums, unsigned *theta, int M,
                                                                    long nch, int tiles) {
  const long c = blockIdx.x / tiles;
  const int k = (int)(blockIdx.x - c * tiles) * kScanBins + (int)(threadIdx.x & (kScanBins - 1));
  pvoc_scan(sums + c * nch * (M + 1) + k, (long)(M + 1), nch, k <= M, theta + c * (M + 1) + k, [] {});
}

__global__ __launch_bounds__(kPvocWG) void k_pvoc_walk(const cpx *__restrict__ frames, long cstride, long nf, int M,
                                                       long nch, int tiles, long items, float kf,
                                                       const unsigned *__restrict__ bases, cpx *__restrict__ spec,
                                                       long sstride) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int tile;
    long j, c;
    pvoc_item(item, tiles, nch, tile, j, c);
    const int k = tile * kPvocWG + (int)threadIdx.x;
    if (k > M) continue;
    const long f0 = j * kPvocChunk, f1 = f0 + kPvocChunk < nf ? f0 + kPvocChunk : nf;
    const cpx *in = frames + c * cstride + f0 * (M + 1) + k;
    cpx *row = spec + c * sstride + f0 * M;
    unsigned th = bases[(c * nch + j) * (M + 1) + k];
    for (long f = f0; f < f1; f++, in += M + 1, row += M) {
      const cpx af = *in;
      th += pvoc_inc(af.y, kf);
      float sn, cs;
      sincospif((float)(int)th * 4.656612873077393e-10f, &sn, &cs);   // 2^-31: the phase in half turns, [-1, 1)
      const float re = af.x * cs, im = af.x * sn;
      // the packed layout: Re P[0] = Re z[0], Im P[0] = Re z[M], bin M/2 conjugated back
      if (k == 0) reinterpret_cast<float *>(row)[0] = re;
      else if (k == M) reinterpret_cast<float *>(row)[1] = re;
      else row[k] = mk(re, k == (M >> 1) ? -im : im);
    }
  }
}

hipError_t launch_pvoc_analyze(const PvocArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  const int tiles = (a.M + 1 + kPvocWG - 1) / kPvocWG;
  const long groups = (a.F + kPvocRun - 1) / kPvocRun, items = (long)a.channels * groups * tiles;
  hipLaunchKernelGGL(k_pvoc_analyze, dim3(pvoc_grid(items, (long)di.num_cus * 16, 0)), dim3(kPvocWG), 0, s, a.spec_in, a.frames_out, a.prev,
                     a.etab, a.F, a.M, groups, tiles, items, a.sh, a.srs);
  return hipGetLastError();
}

hipError_t launch_pvoc_synth(const PvocArgs &a, long f0, long nf, const DeviceInfo &di, hipStream_t s) {
  if (nf <= 0 || a.channels <= 0) return hipSuccess;
  const int tiles = (a.M + 1 + kPvocWG - 1) / kPvocWG;
  const long nch = (nf + kPvocChunk - 1) / kPvocChunk, items = (long)a.channels * nch * tiles;
  const long cstride = a.F * (a.M + 1), sstride = a.F * a.M;
  const cpx *frames = reinterpret_cast<const cpx *>(a.frames_in) + f0 * (a.M + 1);
  const int grid = pvoc_grid(items, (long)di.num_cus * 16, 0);
  hipLaunchKernelGGL(k_pvoc_sums, dim3(grid), dim3(kPvocWG), 0, s, frames, cstride, nf, a.M, nch, tiles, items, a.kf,
                     a.sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int stiles = (a.M + 1 + kScanBins - 1) / kScanBins;
  hipLaunchKernelGGL(k_pvoc_scan, dim3(stiles * a.channels), dim3(kScanBins * kScanSegs), 0, s, a.sums, a.theta, a.M, nch,
                     stiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_pvoc_walk, dim3(grid), dim3(kPvocWG), 0, s, frames, cstride, nf, a.M, nch, tiles, items, a.kf,
                     a.sums, a.spec_out + f0 * a.M, sstride);
  return hipGetLastError();
}

}  // namespace clfa
