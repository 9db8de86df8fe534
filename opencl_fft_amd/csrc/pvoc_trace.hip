// pvoc_trace.hip — the N loudest bins of every frame of a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h):
// Csound's pvstrace with an exact count, its complement (the residual) and the list of the bins kept.  The first Pvoc
// kernel that selects by rank: an exact order statistic per frame with the tie rule of the descriptors' peak (the lower
// bin wins).  Everything is done on the bits: no float arithmetic, no rounding.  Stateless; one launch; no atomics on
// global memory (the histograms are integer counters in LDS, whose sums do not depend on the order), no waiting between
// workgroups.  The group kernels' item and launch are pvoc_device.hpp's, shared with pvoc_desc.hip.
//
//   k_pvoc_trace<W>  W = min(M, 256) lanes form a group that owns a (channel, frame); 256 / W groups share a workgroup.
//                    Row r of the frame is the W consecutive bins r W .. r W + W - 1, the Nyquist bin a last row of one
//                    lane; lane j holds the KEYS of the bins j, j + W, ... in registers, at most 33.  A bin's key is the
//                    monotone uint32 image of its amp (-0 folded onto +0), 0 for a bin that is no candidate (outside the
//                    range, a NaN).  The frame comes from HBM once, for the keys; the output walk reads the pairs again,
//                    from L2 or the Infinity Cache (pairs kept in registers instead cost more than half of the waves).
//                    1. The group's candidates are counted (ballots; segment totals through LDS for W > 64) and N is
//                       clamped to them.  N == 0 and N == candidates need no select: the cut T is set above every key,
//                       or to 0.  The branch is the workgroup's (its barriers are).
//                    2. Otherwise a most-significant-digit radix select, four passes of 8 bits: the keys still live
//                       (those that share the digits found so far) are counted into the group's 256 LDS counters with
//                       integer atomicAdd (W / 32 copies of the counters, by lane, against the pile-up on a few words);
//                       lane j takes 256 / W consecutive counters (summed over the copies, and cleared for the next pass), a suffix scan across the lanes (shuffles inside a segment of min(W, 64) lanes, segment
//                       totals through LDS) finds the one lane whose counters hold the rank, and that lane the digit and
//                       what is left of the rank below it.  After four passes T is the key of the N-th loudest bin and
//                       `need` the number of bins with that key to keep.
//                    3. One walk over the rows in ascending bin order: ballots of "key > T" and "key == T" give the
//                       exclusive prefix counts inside a segment; for W > 64 the per-row, per-segment counts of both go
//                       through LDS once for the whole frame, and the running totals are carried in registers.  The ties
//                       kept are the first `need` in bin order, so a segment's count of selected bins follows from its
//                       two counts and no second exchange is needed.  A lane then knows whether its bin is selected and
//                       its place in the list, stores the pair and the list entry; the list's tail is filled with -1.
//
// tests/pvoc_trace_model.py restates the definition.
#include "pvoc_device.hpp"

namespace clfa {

namespace {

constexpr int kTraceAhead = 4;        // rows whose pairs are in flight at a time in the output walk
constexpr unsigned kTraceNone = 0u;   // the key of a bin that is no candidate: below every candidate's (-inf: 0x007fffff)

// the key of the amp bits u of a bin of the range
__device__ __forceinline__ unsigned trace_key(unsigned u) {
  const bool nan = (u & 0x7fffffffu) > 0x7f800000u;
  if (u == 0x80000000u) u = 0u;   // -0 == +0
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return nan ? kTraceNone : k;
}

// the ballot of the lane's segment: the min(W, 64) lanes of its group that share its wave
template <int W>
__device__ __forceinline__ unsigned long long trace_ballot(bool p) {
  unsigned long long b = __ballot(p);
  if constexpr (W == 32) b = (b >> (threadIdx.x & 32)) & 0xffffffffull;
  return b;
}

// v, anew: what is computed from the result is not kept from an earlier phase or item.  The range predicates of a lane's
// 33 rows and the rows' "r W <= M", hoisted out of the item loop as lane masks, spill the scalar registers
__device__ __forceinline__ int trace_fresh(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ int trace_fresh_uniform(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

__device__ __forceinline__ int trace_clamp(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

}  // namespace

// item -> (channel c, group of G frames); group g of the workgroup takes frame fg G + g.  in, out: pairs as two words
template <int W>
__global__ __launch_bounds__(kGroupWG) void k_pvoc_trace(const uint2 *__restrict__ in, uint2 *__restrict__ out,
                                                         const float *__restrict__ n, int *__restrict__ bins, int list_n,
                                                         long F, int M, int lo, int hi, int residual, long fgroups,
                                                         long items) {
  constexpr int G = kGroupWG / W, SEG = W < 64 ? W : 64, NSEG = W / SEG, CH = 256 / W;
  constexpr int ROWS = (W == kGroupWG ? 32 : 1) + 1;   // rows of W bins at the largest M, and the Nyquist bin's
  // a pass's counters, all 0 between the passes: REP copies of the 256, a lane counting into copy (lane mod REP), since
  // the amps of a frame share a few exponents and every lane's atomic of the first pass would land on the same few words;
  // the copies lie 8 banks apart
  constexpr int REP = W / 32, HSTRIDE = 256 + 8;
  __shared__ unsigned s_hist[G][REP][HSTRIDE];
  __shared__ int s_seg[G][NSEG];            // segment totals: of the candidates, then of each pass's scan
  __shared__ int2 s_res[G];                 // a pass's digit and what is left of the rank
  __shared__ int2 s_cnt[G][ROWS][NSEG];     // (bins with key == T, bins with key > T) of a row's segment
  const int tid = threadIdx.x;
  const long row = M + 1;
  const int nbins = hi - lo + 1;
  for (int i = tid; i < G * REP * HSTRIDE; i += kGroupWG) (&s_hist[0][0][0])[i] = 0u;
  __syncthreads();
#pragma unroll 1
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    int g, j;
    long f, c;
    pvoc_group_row<W>(item, fgroups, g, j, f, c);
    const bool live = f < F;   // false: the group idles along (it has no candidates, stores nothing)
    const int ls = j & (SEG - 1), sg = j / SEG;
    const unsigned long long below = (1ull << ls) - 1ull;
    const long base = (c * F + f) * row;
    const float nv = live ? n[f] : 0.f;   // asked for ahead of the amps: its latency hides behind theirs
    // the amps, as keys: every load is issued before the first key is looked at; what is not loaded (outside the range,
    // past the frame, an idle group) is a NaN, no candidate
    unsigned K[ROWS];
    // (loads without a branch: a lane that has no bin to load reads the frame's last one, or the stream's last frame's)
    const int j1 = trace_fresh(j), M1 = trace_fresh_uniform(M);
    const uint2 *fin = in + (c * F + (live ? f : F - 1)) * row;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      const int k = r * W + j1;
      K[r] = 0x7fffffffu;
      if (r * W <= M1) {
        const unsigned u = fin[k < M1 ? k : M1].x;
        K[r] = live && k >= lo && k <= hi ? u : 0x7fffffffu;
      }
    }
    // the candidates of the lane's segment
    int cand = 0;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      K[r] = trace_key(K[r]);
      if (r * W <= M1) cand += __popcll(trace_ballot<W>(K[r] != kTraceNone));
    }
    if constexpr (NSEG > 1) {
      if (ls == 0) s_seg[g][sg] = cand;
      __syncthreads();
      cand = 0;
#pragma unroll
      for (int s = 0; s < NSEG; s++) cand += s_seg[g][s];
    }
    // the count: N = 0 where n >= 0 does not hold, else floor(min(n, nbins)), and no more than there are candidates
    int N = nv >= 0.f ? (int)floorf(fminf(nv, (float)nbins)) : 0;
    N = N < cand ? N : cand;
    // the cut: the bins with key > T are selected, and the first `need` in bin order of those with key == T
    const bool select = N > 0 && N < cand;
    unsigned T = N == 0 ? 0xffffffffu : kTraceNone;   // nothing, or every candidate; no key is 0xffffffff (a NaN's image)
    int need = 0;
    if (__syncthreads_or(select)) {
      unsigned prefix = 0u;
      int rank = select ? N : 0;   // 0: no lane of the group finds it, and the group has nothing in its counters
#pragma unroll 1
      for (int shift = 24; shift >= 0; shift -= 8) {
        const int Mp = trace_fresh_uniform(M);
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          if (r * W <= Mp) {
            const unsigned key = K[r];
            const unsigned top = shift == 24 ? 0u : key >> (shift + 8);
            if (select && key != kTraceNone && top == prefix) atomicAdd(&s_hist[g][j & (REP - 1)][(key >> shift) & 255u], 1u);
          }
        }
        __syncthreads();
        // lane j: the counters of the digits j CH .. j CH + CH - 1, cleared for the next pass
        unsigned cn[CH];
        int own = 0;
#pragma unroll
        for (int i = 0; i < CH; i++) {
          cn[i] = 0u;
#pragma unroll
          for (int q = 0; q < REP; q++) {
            cn[i] += s_hist[g][q][j * CH + i];
            s_hist[g][q][j * CH + i] = 0u;
          }
          own += (int)cn[i];
        }
        // the keys in the digits of this lane and of the lanes above it
        int incl = own;
#pragma unroll
        for (int d = 1; d < SEG; d <<= 1) {
          const int t = __shfl_down(incl, d, SEG);
          if (ls + d < SEG) incl += t;
        }
        if constexpr (NSEG > 1) {
          if (ls == 0) s_seg[g][sg] = incl;
          __syncthreads();
#pragma unroll
          for (int s = 1; s < NSEG; s++)
            if (s > sg) incl += s_seg[g][s];
        }
        int above = incl - own;
        if (above < rank && rank <= incl) {   // one lane of the group
          int digit = j * CH;
          bool found = false;
#pragma unroll
          for (int i = CH - 1; i >= 0; i--) {
            if (!found) {
              if (above + (int)cn[i] >= rank) {
                digit = j * CH + i;
                found = true;
              } else {
                above += (int)cn[i];
              }
            }
          }
          s_res[g] = make_int2(digit, rank - above);
        }
        __syncthreads();
        if (select) {
          const int2 res = s_res[g];
          prefix = (prefix << 8) | (unsigned)res.x;
          rank = res.y;
        }
      }
      if (select) {
        T = prefix;
        need = rank;
      }
    }
    // the rows' counts of ties and of louder bins, per segment
    if constexpr (NSEG > 1) {
      const int Mc = trace_fresh_uniform(M);
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        if (r * W <= Mc) {
          const int e = __popcll(trace_ballot<W>(K[r] == T)), q = __popcll(trace_ballot<W>(K[r] > T));
          if (ls == 0) s_cnt[g][r][sg] = make_int2(e, q);
        }
      }
      __syncthreads();
    }
    // the walk in ascending bin order: eq_run ties and sel_run selected bins lie below the row
    int eq_run = 0, sel_run = 0;
    int *brow = bins ? bins + (c * F + f) * (long)list_n : nullptr;
#pragma unroll
    for (int r0 = 0; r0 < ROWS; r0 += kTraceAhead) {
      // the pairs of kTraceAhead rows, the second time the frame is read: from L2 or the Infinity Cache
      uint2 P[kTraceAhead];
      const int j2 = trace_fresh(j), M2 = trace_fresh_uniform(M);
#pragma unroll
      for (int i = 0; i < kTraceAhead; i++) {
        const int k = (r0 + i) * W + j2;
        P[i] = make_uint2(0u, 0u);
        if (r0 + i < ROWS && (r0 + i) * W <= M2) P[i] = fin[k < M2 ? k : M2];
      }
#pragma unroll
      for (int i = 0; i < kTraceAhead; i++) {
        const int r = r0 + i;
        if (r < ROWS && r * W <= M2) {
          const int k = r * W + j2;
          unsigned key = K[r];
          asm volatile("" : "+v"(key));   // the ballots anew: kept from the counting above they cost 132 SGPRs, and spill
          const bool eq = key == T, gt = key > T;
          const unsigned long long be = trace_ballot<W>(eq), bg = trace_ballot<W>(gt);
          int eq_at = 0, sel_at = 0;   // ties and selected bins below the lane's segment
#pragma unroll
          for (int s = 0; s < NSEG; s++) {
            if (s == sg) {
              eq_at = eq_run;
              sel_at = sel_run;
            }
            const int2 cnt = NSEG > 1 ? s_cnt[g][r][s] : make_int2(__popcll(be), __popcll(bg));
            sel_run += cnt.y + trace_clamp(need - eq_run, cnt.x);
            eq_run += cnt.x;
          }
          const int eq_low = __popcll(be & below);   // ties in the lower lanes of the segment
          const bool sel = gt || (eq && eq_at + eq_low < need);
          const int pos = sel_at + __popcll(bg & below) + trace_clamp(need - eq_at, eq_low);
          if (live && k <= M2) {
            const bool keep = k < lo || k > hi || (sel != (residual != 0));
            out[base + k] = make_uint2(keep ? P[i].x : 0u, P[i].y);
            if (brow && sel && pos < list_n) brow[pos] = k;
          }
        }
      }
    }
    if (brow && live)
      for (long i = (long)sel_run + j; i < list_n; i += W) brow[i] = -1;
  }
}

template <int W>
static hipError_t launch_pvoc_trace_w(const PvocTraceArgs &a, const DeviceInfo &di, hipStream_t s) {
  const PvocGroups q = pvoc_groups<W>(a.F, a.channels, di, a.grid_max);
  hipLaunchKernelGGL((k_pvoc_trace<W>), dim3(q.grid), dim3(kGroupWG), 0, s, (const uint2 *)a.in, (uint2 *)a.out, a.n,
                     a.bins, a.list_n, a.F, a.M, a.lo, a.hi, a.residual, q.rgroups, q.items);
  return hipGetLastError();
}

hipError_t launch_pvoc_trace(const PvocTraceArgs &a, const DeviceInfo &di, hipStream_t s) {
  if (a.F <= 0 || a.channels <= 0) return hipSuccess;
  if (a.lo < 0 || a.lo > a.hi || a.hi > a.M || (a.bins && a.list_n < 1)) return hipErrorInvalidValue;
  switch (pvoc_group_lanes(a.M)) {
    case 32: return launch_pvoc_trace_w<32>(a, di, s);
    case 64: return launch_pvoc_trace_w<64>(a, di, s);
    case 128: return launch_pvoc_trace_w<128>(a, di, s);
    case 256: return launch_pvoc_trace_w<256>(a, di, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clfa
