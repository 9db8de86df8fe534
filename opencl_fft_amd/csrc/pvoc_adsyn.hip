// pvoc_adsyn.hip — oscillator-bank resynthesis of (amp, freq) frames straight to samples (clfa_pvoc_adsyn,
// include/clfft_amd.h).  The arithmetic is pvoc_adsyn_plan.hpp's: k_adsyn_sums calls adsyn_step (one frame of one
// oscillator), k_adsyn_osc spells the same sequence out in its pre-walk and its group loop (it measured slower with the
// call: DESIGN.md 4e).  Three launches per sub-batch, the shape of the synthesis in pvoc_kernels.hip:
//
//   k_adsyn_sums  per (channel, chunk of kPvocChunk frames, oscillator) the uint64 sum of the frames' phase advances.  The
//                 advance of a frame needs the endpoint of the frame before: read from the frames, or — for the
//                 sub-batch's first chunk — from the state, which these lanes also copy into the workspace (w0, a0): the
//                 scan replaces the state before the oscillators run.
//   k_adsyn_scan  the scan of pvoc_device.hpp (k_pvoc_scan's) on 64-bit words: per (channel, oscillator) the chunks' sums
//                 become their bases in place, P takes the total, W and A the endpoint of the sub-batch's last frame.
//   k_adsyn_osc   the hot loop.  A workgroup takes one chunk of one channel, or — where that would leave workgroups idle — a
//                 run of its frames (it then walks the chunk's earlier frames first: integers only, no samples).  Per
//                 tile of kAdsynTile oscillators (ascending) and group of G frames: lanes act per oscillator — they walk the group's frames from the phase they carry
//                 in registers and put (A0, A_f - A0, phase, D, W0) of every frame into LDS, 32 bytes each — then, after a
//                 barrier, per output sample: the lane keeps j and j (j + 1) / 2 and runs down the tile, every lane of a
//                 frame reading the same LDS address (a broadcast).  One accumulator per sample; between tiles it rests in
//                 the output row itself (the same lane writes and reads it back: plain loads and stores), and the last
//                 tile multiplies by the gain.  So the sum's order is the ascending selection, whatever the grid.
//
// No atomics, no waiting between workgroups, no scratch.  G = min(kAdsynGroupMax, ceil(256 / hop)) frames share the LDS
// (at most 64 KiB: two workgroups per CU and more), so that hops below 256 still fill the lanes of the sample stage.
#include "pvoc_adsyn_plan.hpp"
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kAdsynWG = kAdsynTile;
constexpr int kAdsynGroupMax = 8;
typedef unsigned long long u64;

struct alignas(16) AdsynOsc {
  float a0, da;   // A0, fl(A_f - A0)
  u64 base, d;    // the phase the frame starts from, the slope D
  int w0, pad;    // W0 after the start rule
};
static_assert(sizeof(AdsynOsc) == 32, "two 16-byte LDS reads per oscillator");

// the endpoint of the frame whose (amp, freq) pair of this bin is *fr; fm = that frame's entry of fmod (NULL: none)
__device__ __forceinline__ void adsyn_end_at(const cpx *__restrict__ fr, const float *__restrict__ fm, float ks, int &w,
                                             float &a) {
  const cpx af = *fr;
  int32_t ww;
  adsyn_endpoint(af.x, af.y, fm ? *fm : 1.f, fm != nullptr, ks, ww, a);
  w = ww;
}

}  // namespace

// frames / fmod: the sub-batch's first frame (channel 0; channel c at c * cstride pairs); nf frames in nch chunks
__global__ __launch_bounds__(kAdsynWG) void k_adsyn_sums(const cpx *__restrict__ frames, long cstride,
                                                         const float *__restrict__ fmod, long nf, int M, long nch,
                                                         int first, int nbins, int step, int hop, float ks, int tiles,
                                                         long items, const int *__restrict__ W, const float *__restrict__ A,
                                                         int *__restrict__ w0s, float *__restrict__ a0s,
                                                         u64 *__restrict__ sums) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int tile;
    long j, c;
    pvoc_item(item, tiles, nch, tile, j, c);
    const int i = tile * kAdsynWG + (int)threadIdx.x;
    if (i >= nbins) continue;
    const int k = first + i * step;
    const long f0 = j * kPvocChunk, f1 = f0 + kPvocChunk < nf ? f0 + kPvocChunk : nf;
    const cpx *in = frames + c * cstride + f0 * (M + 1) + k;
    int wp;
    float ap;
    if (j == 0) {
      wp = W[c * (M + 1) + k];
      ap = A[c * (M + 1) + k];
      w0s[c * nbins + i] = wp;
      a0s[c * nbins + i] = ap;
    } else {
      adsyn_end_at(in - (M + 1), fmod ? fmod + (f0 - 1) : nullptr, ks, wp, ap);
    }
    u64 s = 0;
    for (long f = f0; f < f1; f++, in += M + 1) {
      const cpx af = *in;
      int ws;
      uint64_t d;
      s += adsyn_step(wp, ap, af.x, af.y, fmod ? fmod[f] : 1.f, fmod != nullptr, ks, hop, ws, d);
    }
    sums[(c * nch + j) * nbins + i] = s;
  }
}

// one workgroup per (channel, tile of kScanBins oscillators); last: the sub-batch's last frame of channel 0, fm_last its
// entry of fmod (or NULL)
__global__ __launch_bounds__(kScanBins *kScanSegs) void k_adsyn_scan(u64 *__restrict__ sums, u64 *P, int *W, float *A,
                                                                     const cpx *__restrict__ last, long cstride,
                                                                     const float *__restrict__ fm_last, int M, long nch,
                                                                     int first, int nbins, int step, float ks, int tiles) {
  const long c = blockIdx.x / tiles;
  const int i = (int)(blockIdx.x - c * tiles) * kScanBins + (int)(threadIdx.x & (kScanBins - 1));
  const bool live = i < nbins;
  const int k = live ? first + i * step : 0;
  pvoc_scan(sums + c * nch * nbins + i, (long)nbins, nch, live, P + c * (M + 1) + k, [&] {
    int wf;
    float af;
    adsyn_end_at(last + c * cstride + k, fm_last, ks, wf, af);
    W[c * (M + 1) + k] = wf;
    A[c * (M + 1) + k] = af;
  });
}

// signal: the sub-batch's first sample of channel 0 (channel c at c * sstride floats); G frames per group, G * kAdsynTile
// entries of dynamic LDS
__global__ __launch_bounds__(kAdsynWG) void k_adsyn_osc(const cpx *__restrict__ frames, long cstride,
                                                        const float *__restrict__ fmod, long nf, int M, long nch, int first,
                                                        int nbins, int step, int hop, int G, float ks, float gain,
                                                        const u64 *__restrict__ bases, const int *__restrict__ w0s,
                                                        const float *__restrict__ a0s, const float *__restrict__ ramp,
                                                        float *signal, long sstride, int run, int nruns, long items) {
#pragma clang fp contract(off)
  extern __shared__ AdsynOsc s_osc[];
  const int lane = (int)threadIdx.x;
  const int tiles = (nbins + kAdsynTile - 1) / kAdsynTile;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const long cj = item / nruns, c = cj / nch, j = cj - c * nch;
    const long f0 = j * kPvocChunk, fs = f0 + (item - cj * nruns) * run;
    const long f1 = fs + run < nf ? fs + run : nf;   // (run divides the chunk: a run never crosses into the next one)
    if (fs >= f1) continue;   // (the whole workgroup: the chunk ends before this run)
    float *out = signal + c * sstride + fs * hop;
#pragma unroll 1
    for (int tile = 0; tile < tiles; tile++) {
      const int i = tile * kAdsynTile + lane;
      const bool live = i < nbins;
      const int tb = nbins - tile * kAdsynTile < kAdsynTile ? nbins - tile * kAdsynTile : kAdsynTile;
      const bool last_tile = tile == tiles - 1;
      const cpx *in = frames + c * cstride + f0 * (M + 1) + (live ? first + i * step : 0);
      u64 ph = 0;
      int wp = 0;
      float ap = 0.f;
      if (live) {
        ph = bases[(c * nch + j) * nbins + i];
        if (j == 0) {
          wp = w0s[c * nbins + i];
          ap = a0s[c * nbins + i];
        } else {
          adsyn_end_at(in - (M + 1), fmod ? fmod + (f0 - 1) : nullptr, ks, wp, ap);
        }
        // a run that starts inside the chunk walks the chunk's earlier frames first: a few integer steps per
        // oscillator, against hop samples per frame of its own
        for (long f = f0; f < fs; f++, in += M + 1) {
          int wf;
          float af;
          adsyn_end_at(in, fmod ? fmod + f : nullptr, ks, wf, af);
          const int ws = adsyn_start(ap, wp, wf);
          ph += adsyn_advance(ws, adsyn_slope(ws, wf, hop), hop);
          wp = wf;
          ap = af;
        }
      }
#pragma unroll 1
      for (long fg = fs; fg < f1; fg += G) {
        const int ng = f1 - fg < G ? (int)(f1 - fg) : G;
        if (live) {
          for (int g = 0; g < ng; g++, in += M + 1) {
            int wf;
            float af;
            adsyn_end_at(in, fmod ? fmod + (fg + g) : nullptr, ks, wf, af);
            const int ws = adsyn_start(ap, wp, wf);
            const u64 d = adsyn_slope(ws, wf, hop);
            AdsynOsc e;
            e.a0 = ap;
            e.da = af - ap;
            e.base = ph;
            e.d = d;
            e.w0 = ws;
            e.pad = 0;
            s_osc[g * kAdsynTile + lane] = e;
            ph += adsyn_advance(ws, d, hop);
            wp = wf;
            ap = af;
          }
        }
        __syncthreads();
        const int ns = ng * hop;
        float *o = out + (fg - fs) * hop;
#pragma unroll 1
        for (int n = lane; n < ns; n += kAdsynWG) {
          const int g = n / hop;
          const unsigned jj = (unsigned)(n - g * hop) + 1u;
          const unsigned tri = adsyn_tri(jj);
          const float wj = ramp[jj - 1];
          const AdsynOsc *e = s_osc + g * kAdsynTile;
          float acc = tile ? o[n] : 0.f;
#pragma unroll 4
          for (int b = 0; b < tb; b++) {
            const AdsynOsc v = e[b];
            const unsigned hi = adsyn_phase_hi(v.base, v.w0, v.d, jj, tri);
            const float cs = cospif((float)(int)hi * 4.656612873077393e-10f);   // 2^-31: half turns, [-1, 1]
            const float a = v.a0 + v.da * wj;
            acc = acc + a * cs;
          }
          o[n] = last_tile ? gain * acc : acc;
        }
        __syncthreads();
      }
    }
  }
}

hipError_t launch_pvoc_adsyn(const PvocAdsynArgs &a, long f0, long nf, const DeviceInfo &di, hipStream_t s) {
  if (nf <= 0 || a.channels <= 0 || a.nbins <= 0) return hipSuccess;
  const long nch = (nf + kPvocChunk - 1) / kPvocChunk, cstride = a.F * (a.M + 1);
  const cpx *frames = reinterpret_cast<const cpx *>(a.frames) + f0 * (a.M + 1);
  const float *fmod = a.fmod ? a.fmod + f0 : nullptr;
  const int tiles = (a.nbins + kAdsynWG - 1) / kAdsynWG;
  const long sitems = (long)a.channels * nch * tiles;
  hipLaunchKernelGGL(k_adsyn_sums, dim3(pvoc_grid(sitems, (long)di.num_cus * 16, a.grid_max)), dim3(kAdsynWG), 0, s, frames,
                     cstride, fmod, nf, a.M, nch, a.first, a.nbins, a.step, a.hop, a.ks, tiles, sitems, a.w, a.amp, a.w0,
                     a.a0, a.sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int stiles = (a.nbins + kScanBins - 1) / kScanBins;
  hipLaunchKernelGGL(k_adsyn_scan, dim3((unsigned)(stiles * a.channels)), dim3(kScanBins * kScanSegs), 0, s,
                     a.sums, a.phase, a.w, a.amp, frames + (nf - 1) * (a.M + 1), cstride,
                     fmod ? fmod + (nf - 1) : nullptr, a.M, nch, a.first, a.nbins, a.step, a.ks, stiles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // the frames that share the LDS: enough to fill the lanes of the sample stage at small hops
  int G = (kAdsynWG + a.hop - 1) / a.hop;
  G = G > kAdsynGroupMax ? kAdsynGroupMax : G;
  long ocap = (long)di.num_cus * 8;
  if (a.grid_max > 0 && a.grid_max < ocap) ocap = a.grid_max;
  // a chunk in runs of `run` frames, one workgroup each: halved while the launch would leave workgroups idle, but not
  // below a group
  int run = kPvocChunk;
  while ((long)a.channels * nch * (kPvocChunk / run) < ocap && run / 2 >= G) run /= 2;
  const int nruns = kPvocChunk / run;
  const long oitems = (long)a.channels * nch * nruns;
  hipLaunchKernelGGL(k_adsyn_osc, dim3(pvoc_grid(oitems, ocap, 0)), dim3(kAdsynWG),
                     sizeof(AdsynOsc) * (size_t)G * kAdsynTile, s, frames, cstride, fmod, nf, a.M, nch, a.first, a.nbins,
                     a.step, a.hop, G, a.ks, a.gain, a.sums, a.w0, a.a0, a.ramp, a.signal + f0 * a.hop, a.sstride, run, nruns, oitems);
  return hipGetLastError();
}

}  // namespace clfa
