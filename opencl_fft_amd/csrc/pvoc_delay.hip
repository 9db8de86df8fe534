// pvoc_delay.hip — the per-bin delay with feedback along a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h):
// every bin reads the stream d = delays[bin] frames back, y[t] = x[t - d] + g y[t - d] with g = feedback[bin].  The object
// carries the last L input frames (xhist) and the last L output frames (yhist) from call to call, so the bits do not depend
// on how the stream is cut into calls; no atomics, no waiting between workgroups.  The item decoding and the launch
// (pvoc_bin, pvoc_tiles, kTimeWG, kTimeRun) are pvoc_device.hpp's, the commit (k_pvoc_tail) is pvoc_time.hip's.
//
//   k_pvoc_delay     feedback NULL: a gather, parallel over the frames.  An item is the blur's (channel, run of kTimeRun
//                    consecutive frames, tile of 256 bins), a lane per bin; frame f of the call reads frame f - d, from xhist
//                    where that is negative and from the input otherwise.  The run's loads are issued together.
//   k_pvoc_delay_fb  the recurrence is serial along the frames, with a lag: a lane owns one (channel, bin) and walks the
//                    call's frames in blocks of G = kDelayGroup.  The taps of xs do not depend on the recurrence: those of
//                    the next block are loaded while this block's recurrence runs.  The taps of ys:
//                      d <= G  they are among the last G outputs, which the lane keeps in registers (this block's and
//                              the block's before; at the start the reachable ones come from yhist): the tap is picked
//                              by d with selects, so the chain of a bin never goes through memory — with d = 1 a frame
//                              costs a multiply, an add and the selects, not a store and a load of the same address;
//                      d > G   they lie before the block, so the block's G frames do not depend on each other: their G
//                              loads are issued together at its start.  A tap t >= 0 is a row of frames_out that this
//                              lane stored in an earlier block, and the lane is its only reader: frames_out is a plain
//                              pointer here (no __restrict__, no non-temporal or read-only load), so single-thread
//                              program order is all that is relied on, and no row is read before the lane wrote it.
//                              With d >= 2 G the taps lie before the block before as well, so they are loaded a block
//                              ahead, like the taps of xs, and the block does not wait for them.
//                    Bins with d == 0 copy the input's frame in the same walk.  Lanes of one wave may hold any mix of
//                    delays: the block loop is the same for all, so no lane waits for another's shorter groups.
//
// Neither kernel writes a history.  The commit follows on the same stream: k_pvoc_tail puts the last L frames of xhist ++
// frames_in into the spare, a device copy puts the spare over xhist; then the same for yhist ++ frames_out.  No launch both
// reads and writes a history, and there is no ring position.
//
// Every float32 step of the definition is rounded on its own: the kernel switches contraction off.
// tests/pvoc_delay_model.py restates it.
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kDelayWG = 64;      // lanes = bins per workgroup tile of k_pvoc_delay_fb
constexpr int kDelayGroup = 8;    // frames per block of k_pvoc_delay_fb: the loads in flight, and the outputs kept in registers

// the device form's delay of a bin
__device__ __forceinline__ int pvoc_delay_d(int d, int L) { return d < 0 ? 0 : (d > L ? L : d); }

}  // namespace

// item -> (channel, run r, bin tile), the tile fastest.  xhist: channels x L frames (not read for L == 0)
__global__ __launch_bounds__(kTimeWG) void k_pvoc_delay(const cpx *__restrict__ in, cpx *__restrict__ out,
                                                        const int *__restrict__ delays, const cpx *__restrict__ xhist, long F,
                                                        int M, int L, int tiles, long runs, long items) {
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long r, c;
    if (!pvoc_bin<kTimeWG>(item, tiles, runs, M, k, r, c)) continue;
    const long row = M + 1;
    const long f0 = r * kTimeRun, f1 = f0 + kTimeRun < F ? f0 + kTimeRun : F;
    const int d = pvoc_delay_d(delays[k], L);
    const cpx *ic = in + c * F * row + k;          // frame t >= 0 of the stream
    const cpx *hc = xhist + (c * L + L) * row + k;  // frame t < 0 (t >= -L: d <= L)
    cpx v[kTimeRun];
#pragma unroll
    for (int i = 0; i < kTimeRun; i++) {
      const long t = f0 + i - d;
      if (f0 + i < f1) v[i] = t < 0 ? hc[t * row] : ic[t * row];
    }
#pragma unroll
    for (int i = 0; i < kTimeRun; i++)
      if (f0 + i < f1) out[(c * F + f0 + i) * row + k] = v[i];
  }
}

// item -> (channel, bin tile of 64).  out is read where this lane has written it: a plain pointer (see above)
__global__ __launch_bounds__(kDelayWG) void k_pvoc_delay_fb(const cpx *__restrict__ in, cpx *out, const int *__restrict__ delays,
                                                            const float *__restrict__ feedback, const cpx *__restrict__ xhist,
                                                            const cpx *__restrict__ yhist, long F, int M, int L, int tiles,
                                                            long items) {
#pragma clang fp contract(off)
  constexpr int G = kDelayGroup;
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int k;
    long j, c;
    if (!pvoc_bin<kDelayWG>(item, tiles, 1, M, k, j, c)) continue;
    const long row = M + 1;
    const int d = pvoc_delay_d(delays[k], L);
    const float g = feedback[k];
    const bool far = d > G;   // the taps of ys lie before the block: loaded; else they are the last G outputs, in registers
    const bool ahead = d >= 2 * G;   // ... and before the block before it: loaded a block ahead, as the taps of xs are
    const cpx *x = in + c * F * row + k;
    cpx *o = out + c * F * row + k;
    const cpx *xh = xhist + (c * L + L) * row + k;   // frame t < 0 of xs and of ys (t >= -L: d <= L)
    const cpx *yh = yhist + (c * L + L) * row + k;
    // xs[t] for the frames of a block; yp: the outputs of the block before, frames f0 - G .. f0 - 1 (d <= G: those a tap
    // can reach, t >= -d, come from yhist at the start), yo: those of this block; ym: the block's loaded taps of ys
    // (d > G), ymn: the next block's (d >= 2 G)
    cpx cur[G], nxt[G], yp[G], yo[G], ym[G], ymn[G];
#pragma unroll
    for (int i = 0; i < G; i++) {
      const long t = i - d;
      if (i < F) cur[i] = t < 0 ? xh[t * row] : x[t * row];
      yp[i] = mk(0.f, 0.f);
      if (!far && G - i <= d) yp[i] = yh[(i - G) * row];
      yo[i] = ym[i] = ymn[i] = nxt[i] = mk(0.f, 0.f);
      if (ahead && i < F) ym[i] = yh[t * row];   // block 0 of a lane that loads ahead: t <= i - 2 G < 0
    }
#pragma unroll 1
    for (long f0 = 0; f0 < F; f0 += G) {
#pragma unroll
      for (int i = 0; i < G; i++) {   // the next block's taps of xs, issued before this block's recurrence
        const long t = f0 + G + i - d;
        if (f0 + G + i < F) nxt[i] = t < 0 ? xh[t * row] : x[t * row];
        if (ahead && f0 + G + i < F) ymn[i] = t < 0 ? yh[t * row] : o[t * row];   // t < f0: stored in an earlier block
      }
      if (far && !ahead) {
#pragma unroll
        for (int i = 0; i < G; i++) {   // t < f0: a history row, or a row of out this lane stored in an earlier block
          const long t = f0 + i - d;
          if (f0 + i < F) ym[i] = t < 0 ? yh[t * row] : o[t * row];
        }
      }
#pragma unroll
      for (int i = 0; i < G; i++) {
        cpx tap = ym[i];
#pragma unroll
        for (int dd = 1; dd <= G; dd++) {   // d <= G: frame f0 + i - d of ys is yo[i - d], or yp[G + i - d] of the block before
          const cpx held = dd <= i ? yo[i - dd] : yp[G + i - dd];
          tap = d == dd ? held : tap;
        }
        const float a1 = cur[i].x;
        const float a2 = g * tap.x;
        const float amp = a1 + a2;
        const cpx y = mk(amp, fabsf(a2) > fabsf(a1) ? tap.y : cur[i].y);   // a NaN on either side: the input's freq
        yo[i] = d == 0 ? cur[i] : y;   // d == 0 is the input's frame itself: no loop without a delay
        if (f0 + i < F) o[(f0 + i) * row] = yo[i];
      }
#pragma unroll
      for (int i = 0; i < G; i++) cur[i] = nxt[i], yp[i] = yo[i], ym[i] = ymn[i];   // (ym: looked at by the far lanes only)
    }
  }
}

hipError_t launch_pvoc_delay(const PvocDelayArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.feedback) {
    const PvocTiles t = pvoc_tiles(a.M, kDelayWG, a.channels, di, 32, a.grid_max);
    hipLaunchKernelGGL(k_pvoc_delay_fb, dim3(t.grid), dim3(kDelayWG), 0, s, a.in, a.out, a.delays, a.feedback, a.xhist, a.yhist,
                       a.F, a.M, a.L, t.tiles, t.items);
  } else {
    const long runs = (a.F + kTimeRun - 1) / kTimeRun;
    const PvocTiles t = pvoc_tiles(a.M, kTimeWG, a.channels * runs, di, 16, a.grid_max);
    hipLaunchKernelGGL(k_pvoc_delay, dim3(t.grid), dim3(kTimeWG), 0, s, a.in, a.out, a.delays, a.xhist, a.F, a.M, a.L, t.tiles,
                       runs, t.items);
  }
  if (hipError_t e = hipGetLastError()) return e;
  if (a.L == 0) return hipSuccess;
  const size_t bytes = sizeof(cpx) * (size_t)a.channels * a.L * (a.M + 1);
  const cpx *src[2] = {a.in, a.out};
  cpx *hist[2] = {a.xhist, a.yhist};
  for (int i = 0; i < 2; i++) {
    if (hipError_t e = launch_pvoc_time_tail(hist[i], a.L, src[i], a.F, a.spare, a.L, a.channels, a.M, a.grid_max, di, s)) return e;
    if (hipError_t e = hipMemcpyAsync(hist[i], a.spare, bytes, hipMemcpyDeviceToDevice, s)) return e;
  }
  return hipSuccess;
}

}  // namespace clfa
