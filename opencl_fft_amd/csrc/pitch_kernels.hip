// pitch_kernels.hip — the pitch of every frame of a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): Csound's
// pvspitch as subharmonic summation on the frame's spectral peaks, and the list of those peaks (amp, true freq) as an
// output of its own.  Stateless; one launch; no atomics, no waiting between workgroups.  The group kernels' item and
// launch are pvoc_group.hpp's, shared with pvoc_desc.hip and pvoc_trace.hip; the peak test and the score of one
// candidate are pvoc_pitch_score.hpp's, plain C++ that the CPU tests build too.  The launcher has a header of its own
// (pitch_launch.hpp), as the filter bank's has: nothing here depends on the launchers of the frame operations.
//
//   k_pvoc_pitch<W>  W = min(M, 256) lanes form a group that owns a (channel, frame); 256 / W groups share a workgroup.
//                    Row r of the frame is the W consecutive bins r W .. r W + W - 1 (the range ends below the Nyquist
//                    bin, so that bin has no row here).
//                    1. The walk over the rows that meet the range, in ascending bin order, kPitchRows rows at a time
//                       for W = 256 (one row is the whole frame for the smaller W): a lane loads its bin's pair and the
//                       two neighbouring amps (from L1 / L2: the lanes next to it load them as their own) and tests the
//                       bin.  A peak's place in the list is the number of peaks below it: ballots inside a segment of
//                       min(W, 64) lanes, the rows' segment counts through LDS (two copies, by the chunk's parity, so
//                       one barrier a chunk), the running total in a register.  The first npeaks peaks go to the
//                       group's list in LDS, and the walk stops once it has them (W = 256: the branch is the
//                       workgroup's; the smaller W have one chunk).
//                    2. The at most 8 L candidates t = 8 i + (m - 1) are dealt to the lanes, t = j, j + W, ...; a lane
//                       divides, tests fmin <= c <= fmax and scores its candidate serially over the list (the list and
//                       the weights are broadcast reads of LDS), keeping the best of its own by the BEST order.
//                    3. The best of the group: shuffles inside a segment, the segments' through LDS.  The order is total
//                       on (score, c) and two candidates equal in both give the same row, so any pairing does.
//                    4. Lane 0 sums the list's amps serially and stores the row; the lanes store the list's pairs.
//
// Every float32 step of the definition is rounded on its own: contraction is off in every function below.
// tests/pvoc_pitch_model.py restates it.
#include "pitch_launch.hpp"
#include "pvoc_group.hpp"
#include "pvoc_pitch_score.hpp"

namespace clfa {

namespace {

constexpr int kPitchRows = 4;   // rows of a chunk of the walk for W = 256: their loads are in flight together

// the best candidate so far: its score and c; s = -1 (below every score: the amps of a list are >= +0): none
struct PitchBest {
  float s, c;
};
// BEST: o beats p iff its score is higher, or the scores are equal and its c is
__device__ __forceinline__ PitchBest pitch_better(PitchBest p, PitchBest o) {
  const bool take = o.s > p.s || (o.s == p.s && o.c > p.c);
  return take ? o : p;
}

// the ballot of the lane's segment: the min(W, 64) lanes of its group that share its wave
template <int W>
__device__ __forceinline__ unsigned long long pitch_ballot(bool p) {
  unsigned long long b = __ballot(p);
  if constexpr (W == 32) b = (b >> (threadIdx.x & 32)) & 0xffffffffull;
  return b;
}

}  // namespace

// item -> (channel c, group of G frames); group g of the workgroup takes frame fg G + g.  in: pairs; rows: channels x F
// x 4; peaks: NULL, or channels x F x npeaks pairs.  1 <= lo <= hi <= M - 1, 1 <= npeaks <= 32
template <int W>
__global__ __launch_bounds__(kGroupWG) void k_pvoc_pitch(const float2 *__restrict__ in, float *__restrict__ rows,
                                                         float2 *__restrict__ peaks, PvocPitchWeights wt, long F, int M,
                                                         int lo, int hi, int npeaks, float thresh, float fmin, float fmax,
                                                         float tol, long fgroups, long items) {
#pragma clang fp contract(off)
  constexpr int G = kGroupWG / W, SEG = W < 64 ? W : 64, NSEG = W / SEG, RCH = W == kGroupWG ? kPitchRows : 1;
  __shared__ float s_w[kPitchHarm];
  __shared__ float s_A[G][kPitchPeaksMax], s_Q[G][kPitchPeaksMax];   // the group's list
  __shared__ int s_cnt[2][G][RCH][NSEG];                             // peaks of a row's segment, by the chunk's parity
  __shared__ PitchBest s_best[G][NSEG];
  const int tid = threadIdx.x;
  const long row = M + 1;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < kPitchHarm; i++) s_w[i] = wt.w[i];
  }
  __syncthreads();
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int g, j;
    long f, c;
    pvoc_group_row<W>(item, fgroups, g, j, f, c);
    const bool live = f < F;   // false: the group idles along (it finds no peak, stores nothing)
    const int ls = j & (SEG - 1), sg = j / SEG;
    const unsigned long long below = (1ull << ls) - 1ull;
    const float2 *fin = in + (c * F + (live ? f : 0)) * row;
    // 1. the walk: `run` peaks lie below the chunk (the same number in every lane of the group)
    int run = 0, par = 0;
    const int rlast = W == kGroupWG ? hi / W : 0;
#pragma unroll 1
    for (int r0 = W == kGroupWG ? lo / W : 0; r0 <= rlast; r0 += RCH) {
      float2 P[RCH];
      float al[RCH], ar[RCH];
      bool in_range[RCH];
#pragma unroll
      for (int i = 0; i < RCH; i++) {
        const int k = (r0 + i) * W + j;
        in_range[i] = live && k >= lo && k <= hi;   // so 1 <= k <= M - 1: both neighbours are bins of the frame
        P[i] = make_float2(0.f, 0.f);
        al[i] = ar[i] = 0.f;
        if (in_range[i]) {
          P[i] = fin[k];
          al[i] = fin[k - 1].x;
          ar[i] = fin[k + 1].x;
        }
      }
      bool pk[RCH];
      unsigned long long b[RCH];
#pragma unroll
      for (int i = 0; i < RCH; i++) {
        pk[i] = in_range[i] && pitch_is_peak(al[i], P[i].x, ar[i], P[i].y, thresh);
        b[i] = pitch_ballot<W>(pk[i]);
      }
      if constexpr (NSEG > 1) {
        if (ls == 0) {
#pragma unroll
          for (int i = 0; i < RCH; i++) s_cnt[par][g][i][sg] = __popcll(b[i]);
        }
        __syncthreads();
      }
      int at = run;
#pragma unroll
      for (int i = 0; i < RCH; i++) {
        int before = at;   // peaks below the lane's segment of this row
#pragma unroll
        for (int s = 0; s < NSEG; s++) {
          const int cnt = NSEG > 1 ? s_cnt[par][g][i][s] : __popcll(b[i]);
          if (s < sg) before += cnt;
          at += cnt;
        }
        const int pos = before + __popcll(b[i] & below);
        if (pk[i] && pos < npeaks) {
          s_A[g][pos] = P[i].x;
          s_Q[g][pos] = P[i].y;
        }
      }
      run = at;
      par ^= 1;
      if (W == kGroupWG && run >= npeaks) break;   // G == 1: the workgroup's branch
    }
    const int L = run < npeaks ? run : npeaks;
    __syncthreads();   // the list is written
    // 2. the candidates t = 8 i + (m - 1) of the lane
    const float *A = s_A[g], *Q = s_Q[g];
    PitchBest best;
    best.s = -1.f;
    best.c = 0.f;
    for (int t = j; t < kPitchDiv * L; t += W) {
      const float m = (float)((t & (kPitchDiv - 1)) + 1);
      const float cand = Q[t / kPitchDiv] / m;   // the correctly rounded division
      if (cand >= fmin && cand <= fmax) {
        PitchBest o;
        o.s = pitch_score(A, Q, L, cand, s_w, tol);
        o.c = cand;
        if (o.s == o.s) best = pitch_better(best, o);   // a NaN score is dropped
      }
    }
    // 3. the best of the group
#pragma unroll
    for (int d = SEG / 2; d >= 1; d >>= 1) {
      PitchBest o;
      o.s = __shfl_xor(best.s, d);
      o.c = __shfl_xor(best.c, d);
      best = pitch_better(best, o);
    }
    if constexpr (NSEG > 1) {
      if (ls == 0) s_best[g][sg] = best;
      __syncthreads();
      best = s_best[g][0];
#pragma unroll
      for (int s = 1; s < NSEG; s++) best = pitch_better(best, s_best[g][s]);
    }
    // 4. the row and the list
    if (live && j == 0) {
      float total = 0.f;
      for (int i = 0; i < L; i++) total = total + A[i];
      const bool any = best.s >= 0.f;
      const float conf = best.s / total;
      float *orow = rows + (c * F + f) * 4;
      orow[0] = any ? best.c : 0.f;
      orow[1] = any ? best.s : 0.f;
      orow[2] = !any || total == 0.f ? 0.f : conf;
      orow[3] = (float)L;
    }
    if (live && peaks) {
      float2 *prow = peaks + (c * F + f) * (long)npeaks;
      for (int i = j; i < npeaks; i += W) prow[i] = i < L ? make_float2(A[i], Q[i]) : make_float2(0.f, 0.f);
    }
    __syncthreads();   // the list and the exchange are read before the next item's land in them
  }
}

template <int W>
static hipError_t launch_pvoc_pitch_w(const PvocPitchArgs &a, const DeviceInfo &di, hipStream_t s) {
  const PvocGroups q = pvoc_groups<W>(a.F, a.channels, di, a.grid_max);
  hipLaunchKernelGGL((k_pvoc_pitch<W>), dim3(q.grid), dim3(kGroupWG), 0, s, (const float2 *)a.in, a.rows, (float2 *)a.peaks,
                     a.weights, a.F, a.M, a.lo, a.hi, a.npeaks, a.thresh, a.fmin, a.fmax, a.tol, q.rgroups, q.items);
  return hipGetLastError();
}

hipError_t launch_pvoc_pitch(const PvocPitchArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.lo < 1 || a.lo > a.hi || a.hi > a.M - 1 || a.npeaks < 1 || a.npeaks > kPitchPeaksMax) return hipErrorInvalidValue;
  switch (pvoc_group_lanes(a.M)) {
    case 32: return launch_pvoc_pitch_w<32>(a, di, s);
    case 64: return launch_pvoc_pitch_w<64>(a, di, s);
    case 128: return launch_pvoc_pitch_w<128>(a, di, s);
    case 256: return launch_pvoc_pitch_w<256>(a, di, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clfa
