// pvoc_time.hip — operations along a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): moving average
// (blur), one-pole low-pass (smooth) and freeze.  Each carries a state from call to call.  An output value is a fixed
// sequence of single float32 roundings of the stream's values, so the bits do not depend on how the stream is cut into
// calls, on the grid or on the run length: there is no parallel float sum or scan here, no atomics and no waiting between
// workgroups.  The tile kernels' prologue and launch (pvoc_bin, pvoc_tiles) are pvoc_device.hpp's.
//
//   k_pvoc_blur    an item is (channel, run of kTimeRun consecutive frames, tile of 256 bins), a lane per bin.  The lane
//                  forms each output's sum in the defined order, oldest frame first: O(n) additions per output by
//                  definition (a running sum would change the bits).  Index t < 0 of the stream is the history's, t >= 0
//                  the input's.  The windows of a run overlap, so the lane walks their union once, oldest row first, and
//                  adds each row to the sum (kTimeRun pairs in registers) of every frame whose window holds it: n +
//                  kTimeRun - 1 loads per run instead of n kTimeRun.  The launch only reads the history.
//   k_pvoc_tail    the last `rows` frames of (history ++ frames) into another buffer.  The blur's commit: into the spare,
//                  which a device copy on the same stream then puts over the history, so that no launch both reads and
//                  writes the history and no ring position exists (on the host it would not advance under graph replay,
//                  on the device its update would race with its readers).  The freeze's commit: the output's last frame
//                  into held.  The descriptors' commit (pvoc_desc.hip, launch_pvoc_time_last): the input's last frame.
//                  The delay's commit (pvoc_delay.hip, launch_pvoc_time_tail): its two histories, as the blur's.
//   k_pvoc_smooth  the recurrence is serial along the frames: a lane owns one (channel, bin), reads its state first, walks
//                  the call's frames and writes the state last.  The loads do not depend on the recurrence: a group of
//                  kSmoothGroup frames is in flight in registers ahead of the arithmetic.  Workgroups of 64 lanes spread
//                  channels x (M + 1) lanes over the CUs; the kernel is bound by latency, not by bandwidth.
//   k_pvoc_freeze  an item as the blur's.  For the run's first frame the workgroup finds, per column, the last frame g
//                  whose flag is 0 by searching p (and q) backwards, 256 flags per step with a ballot per wave (LDS: the
//                  waves' answers, two buffers used in turn so that one barrier per step is enough); it then walks forward
//                  through the run.  A column with no unfrozen frame in the call reads held.  The launch only reads held.
//   k_pvoc_fill    frames of EMPTY bins: what the states start from.
//
// Every float32 step of the definitions is rounded on its own: the device functions switch contraction off.
// tests/pvoc_time_model.py restates them.
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kSmoothWG = 64;      // lanes = bins per workgroup tile of k_pvoc_smooth
constexpr int kSmoothGroup = 8;    // frames in flight ahead of the recurrence

// the blur's window length of a frame
__device__ __forceinline__ int pvoc_blur_n(float P, int max_frames) {
  return P >= 1.f ? (int)floorf(fminf(P, (float)max_frames)) : 1;   // a NaN compares false
}

__device__ __forceinline__ cpx pvoc_smooth_bin(cpx y, cpx x, float ca, float cf) {
  return mk(pvoc_morph(y.x, x.x, ca), pvoc_morph(y.y, x.y, cf));
}

}  // namespace

// item -> (channel, run r, bin tile), the tile fastest.  hist: channels x L frames (not read for L == 0)
__global__ __launch_bounds__(kTimeWG) void k_pvoc_blur(const cpx *in, cpx *__restrict__ out, const float *__restrict__ p,
                                                       const cpx *hist, long F, int M, int L, int max_frames, int tiles,
                                                       long runs, long items) {
#pragma clang fp contract(off)
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long r, c;
    if (!pvoc_bin<kTimeWG>(item, tiles, runs, M, k, r, c)) continue;
    const long f0 = r * kTimeRun, f1 = f0 + kTimeRun < F ? f0 + kTimeRun : F;
    const cpx *ic = in + c * F * (M + 1) + k;          // frame t >= 0 of the stream
    const cpx *hc = hist + (c * L + L) * (M + 1) + k;  // frame t < 0 (t >= -L: n <= max_frames)
    // the run's windows overlap: each row of their union is loaded once and goes into the sum of every frame whose
    // window holds it.  t ascends, so every sum takes its frames oldest first, as defined.
    int u0[kTimeRun], umin = 0;   // the windows' first rows and the union's, counted from f0 (<= 0)
    float rn[kTimeRun];
    cpx S[kTimeRun];
#pragma unroll
    for (int i = 0; i < kTimeRun; i++) {
      const int n = f0 + i < f1 ? pvoc_blur_n(p[f0 + i], max_frames) : 1;
      rn[i] = (float)(1.0 / (double)n);
      u0[i] = i - n + 1;
      umin = u0[i] < umin ? u0[i] : umin;
      S[i] = mk(0.f, 0.f);
    }
    const int uend = (int)(f1 - f0);
#pragma unroll 1
    for (int u = umin; u < uend; u++) {
      const long t = f0 + u;
      const cpx v = t < 0 ? hc[t * (M + 1)] : ic[t * (M + 1)];
#pragma unroll
      for (int i = 0; i < kTimeRun; i++) {
        if (u >= u0[i] && u <= i) {   // uniform over the workgroup
          const cpx sum = mk(S[i].x + v.x, S[i].y + v.y);
          S[i] = u == u0[i] ? v : sum;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kTimeRun; i++)
      if (f0 + i < f1) out[(c * F + f0 + i) * (M + 1) + k] = mk(S[i].x * rn[i], S[i].y * rn[i]);
  }
}

// dst (channels x rows frames) = frames F - rows .. F - 1 of the stream hist ++ src, per channel; hist: channels x L
// frames, read only where rows > F (then rows <= L)
__global__ __launch_bounds__(kTimeWG) void k_pvoc_tail(const cpx *hist, int L, const cpx *src, long F, cpx *__restrict__ dst,
                                                       int rows, int M, int tiles, long items) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long j, c;
    if (!pvoc_bin<kTimeWG>(item, tiles, rows, M, k, j, c)) continue;
    const long t = F - rows + j;
    dst[(c * rows + j) * (M + 1) + k] = t < 0 ? hist[(c * L + L + t) * (M + 1) + k] : src[(c * F + t) * (M + 1) + k];
  }
}

// item -> (channel, bin tile of 64).  y: channels x (M + 1), read first and written last by the lane that owns the bin
__global__ __launch_bounds__(kSmoothWG) void k_pvoc_smooth(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                           const float *__restrict__ p, const float *__restrict__ q,
                                                           cpx *y, long F, int M, int tiles, long items) {
  constexpr int G = kSmoothGroup;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long j, c;
    if (!pvoc_bin<kSmoothWG>(item, tiles, 1, M, k, j, c)) continue;
    const long row = M + 1;
    const cpx *x = in + c * F * row + k;
    cpx *o = out + c * F * row + k;
    cpx state = y[c * row + k];
    cpx cur[G], nxt[G];
#pragma unroll
    for (int i = 0; i < G; i++)
      if (i < F) cur[i] = x[i * row];
#pragma unroll 1
    for (long f0 = 0; f0 < F; f0 += G) {
#pragma unroll
      for (int i = 0; i < G; i++)   // the next group's loads, issued before this group's recurrence
        if (f0 + G + i < F) nxt[i] = x[(f0 + G + i) * row];
#pragma unroll
      for (int i = 0; i < G; i++) {
        if (f0 + i < F) {
          state = pvoc_smooth_bin(state, cur[i], pvoc_clamp01(p[f0 + i]), pvoc_clamp01(q[f0 + i]));
          o[(f0 + i) * row] = state;
        }
      }
#pragma unroll
      for (int i = 0; i < G; i++) cur[i] = nxt[i];
    }
    y[c * row + k] = state;
  }
}

// item -> (channel, run r, bin tile), the tile fastest.  held: channels x (M + 1), only read
__global__ __launch_bounds__(kTimeWG) void k_pvoc_freeze(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                         const float *__restrict__ p, const float *__restrict__ q,
                                                         const cpx *__restrict__ held, long F, int M, int tiles, long runs,
                                                         long items) {
  constexpr int WAVES = kTimeWG / 64;
  __shared__ long s_found[2][2][WAVES];   // [buffer][column][wave]: the newest unfrozen frame a wave saw, or -1
  const int tid = threadIdx.x, wave = tid / 64;
  int buf = 0;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long r, c;
    const bool in_row = pvoc_bin<kTimeWG>(item, tiles, runs, M, k, r, c);
    const long f0 = r * kTimeRun, f1 = f0 + kTimeRun < F ? f0 + kTimeRun : F;
    // g of frame f0, per column: every lane of the workgroup takes part and ends with the same answers
    long ga = -1, gf = -1;
    bool da = false, df = false;
#pragma unroll 1
    for (long base = f0; base >= 0 && !(da && df); base -= kTimeWG, buf ^= 1) {
      const long g = base - tid;   // lane 0 of wave 0 looks at the newest frame
      const unsigned long long ma = __ballot(!da && g >= 0 && p[g >= 0 ? g : 0] == 0.f);
      const unsigned long long mf = __ballot(!df && g >= 0 && q[g >= 0 ? g : 0] == 0.f);
      if ((tid & 63) == 0) {
        s_found[buf][0][wave] = ma ? base - wave * 64 - __builtin_ctzll(ma) : -1;
        s_found[buf][1][wave] = mf ? base - wave * 64 - __builtin_ctzll(mf) : -1;
      }
      __syncthreads();
      for (int w = 0; w < WAVES && !da; w++) {
        const long v = s_found[buf][0][w];
        if (v >= 0) ga = v, da = true;
      }
      for (int w = 0; w < WAVES && !df; w++) {
        const long v = s_found[buf][1][w];
        if (v >= 0) gf = v, df = true;
      }
    }
    if (!in_row) continue;   // only now: every lane took part in the search
    const cpx *ic = in + c * F * (M + 1) + k;
    const cpx h = held[c * (M + 1) + k];
#pragma unroll 1
    for (long f = f0; f < f1; f++) {
      if (f > f0) {
        if (p[f] == 0.f) ga = f;
        if (q[f] == 0.f) gf = f;
      }
      const cpx va = ga < 0 ? h : ic[ga * (M + 1)];
      const cpx vf = gf == ga ? va : (gf < 0 ? h : ic[gf * (M + 1)]);
      out[(c * F + f) * (M + 1) + k] = mk(va.x, vf.y);
    }
  }
}

__global__ __launch_bounds__(kTimeWG) void k_pvoc_fill(cpx *__restrict__ dst, int M, float cf, int tiles, long items) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const long row = item / tiles;
    const int k = (int)(item - row * tiles) * kTimeWG + (int)threadIdx.x;
    if (k <= M) dst[row * (M + 1) + k] = pvoc_empty(k, cf);
  }
}

static hipError_t launch_pvoc_tail(const PvocTimeArgs &a, const cpx *hist, int L, const cpx *src, cpx *dst, int rows,
                                   const DeviceInfo &di, hipStream_t s) {
  const PvocTiles t = pvoc_tiles(a.M, kTimeWG, (long)a.channels * rows, di, 16, a.grid_max);
  hipLaunchKernelGGL(k_pvoc_tail, dim3(t.grid), dim3(kTimeWG), 0, s, hist, L, src, a.F, dst, rows, a.M, t.tiles, t.items);
  return hipGetLastError();
}

hipError_t launch_pvoc_time_tail(const cpx *hist, int L, const cpx *src, long F, cpx *dst, int rows, int channels, int M,
                                 int grid_max, const DeviceInfo &di, hipStream_t s) {
  if (rows <= 0 || channels <= 0) return hipSuccess;
  PvocTimeArgs a;
  a.M = M;
  a.channels = channels;
  a.F = F;
  a.grid_max = grid_max;
  return launch_pvoc_tail(a, hist, L, src, dst, rows, di, s);
}

hipError_t launch_pvoc_time_last(const cpx *src, long F, cpx *dst, int channels, int M, int grid_max, const DeviceInfo &di,
                                 hipStream_t s) {
  if (F <= 0) return hipSuccess;
  return launch_pvoc_time_tail(nullptr, 0, src, F, dst, 1, channels, M, grid_max, di, s);
}

hipError_t launch_pvoc_time(const PvocTimeArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.op == PVOC_SMOOTH) {
    const PvocTiles t = pvoc_tiles(a.M, kSmoothWG, a.channels, di, 32, a.grid_max);
    hipLaunchKernelGGL(k_pvoc_smooth, dim3(t.grid), dim3(kSmoothWG), 0, s, a.in, a.out, a.p, a.q, a.state, a.F, a.M, t.tiles,
                       t.items);
    return hipGetLastError();
  }
  const long runs = (a.F + kTimeRun - 1) / kTimeRun;
  const PvocTiles t = pvoc_tiles(a.M, kTimeWG, a.channels * runs, di, 16, a.grid_max);
  if (a.op == PVOC_FREEZE) {
    hipLaunchKernelGGL(k_pvoc_freeze, dim3(t.grid), dim3(kTimeWG), 0, s, a.in, a.out, a.p, a.q, a.state, a.F, a.M, t.tiles, runs,
                       t.items);
    if (hipError_t e = hipGetLastError()) return e;
    return launch_pvoc_tail(a, nullptr, 0, a.out, a.state, 1, di, s);
  }
  if (a.op != PVOC_BLUR) return hipErrorInvalidValue;
  const int L = a.max_frames - 1;
  hipLaunchKernelGGL(k_pvoc_blur, dim3(t.grid), dim3(kTimeWG), 0, s, a.in, a.out, a.p, a.state, a.F, a.M, L, a.max_frames, t.tiles,
                     runs, t.items);
  if (hipError_t e = hipGetLastError()) return e;
  if (L == 0) return hipSuccess;
  if (hipError_t e = launch_pvoc_tail(a, a.state, L, a.in, a.spare, L, di, s)) return e;
  return hipMemcpyAsync(a.state, a.spare, sizeof(cpx) * (size_t)a.channels * L * (a.M + 1), hipMemcpyDeviceToDevice, s);
}

hipError_t launch_pvoc_time_fill(cpx *dst, long frames, int M, float cf, hipStream_t s) {
  if (frames <= 0) return hipSuccess;
  const int tiles = (M + 1 + kTimeWG - 1) / kTimeWG;
  const long items = frames * tiles;
  const int grid = (int)(items < 65536 ? items : 65536);
  hipLaunchKernelGGL(k_pvoc_fill, dim3(grid), dim3(kTimeWG), 0, s, dst, M, cf, tiles, items);
  return hipGetLastError();
}

}  // namespace clfa
