// stft_plan.hpp — the index arithmetic of the overlap-add synthesis (k_stft_synth, stft_kernels.hip): the window
// envelope's table and lookup, and the split of a channel's frames into runs.  Plain functions of plain arguments, for
// the host and the device alike: tests/test_stft_plan_cpu.py builds them with g++ and checks them exhaustively.
#pragma once

#if defined(__HIPCC__)
#define CLFA_PLAN_HD __host__ __device__
#else
#define CLFA_PLAN_HD
#endif

namespace clfa {

// frames a workgroup of the Stft kernels holds at once (LdsGeom<log2(size / 2)>::FPW)
CLFA_PLAN_HD constexpr int stft_fpw(int size) { return size >= 8192 ? 1 : 8192 / size; }

// ---- envelope: env[p] = sum of w[p - f hop]^2 over the frames f of the call that cover sample p ----------------------
// cum = [lo | hi], 2 * size doubles: lo[d] = sum_k w[d - k hop]^2, hi[d] = sum_k w[d + k hop]^2 (k >= 0, inside the
// window).  A float squared is exact in double, and a term of 0 leaves the running sum's bits alone.
inline void stft_env_table(const float *w, int size, int hop, double *cum) {
  double *lo = cum, *hi = cum + size;
  for (int d = 0; d < size; d++) lo[d] = (double)w[d] * w[d] + (d >= hop ? lo[d - hop] : 0.0);
  for (int d = size - 1; d >= 0; d--) hi[d] = (double)w[d] * w[d] + (d + hop < size ? hi[d + hop] : 0.0);
}

// The frames that cover p sit at window positions dl, dl + hop, .., dh.  Returns which form the lookup takes:
//   1  no frame is cut off above (dh + hop >= size): the tail sum from dl, hi[dl];
//   2  none is cut off below (dl < hop): the head sum up to dh, lo[dh];
//   3  both (a call of fewer frames than size / hop): a difference of two running sums.
CLFA_PLAN_HD inline int stft_env_span(int size, int hop, int F, long p, int &dl, int &dh) {
  const long fh = p / hop < F - 1 ? p / hop : F - 1;
  const long fl = p < size ? 0 : (p - size) / hop + 1;
  dl = (int)(p - fh * hop);
  dh = (int)(p - fl * hop);
  if (dh + hop >= size) return 1;
  if (dl < hop) return 2;
  return 3;
}

// The envelope at p, rounded once to float.  Forms 1 and 2 round a table entry.  Form 3 subtracts in double, from the
// side of the window whose running sums are the shorter ones: lo[dh] - lo[dl - hop] where the span lies nearer the
// window's start, hi[dl] - hi[dh + hop] otherwise.  The difference carries the rounding of at most min(dh, size - dl)
// / hop double additions of terms no larger than the sums themselves, far below the one float rounding that follows;
// over a stretch of zeros both sums are the same bits and the difference is exactly 0.
CLFA_PLAN_HD inline float stft_env_at(const double *cum, int size, int hop, int F, long p) {
  int dl, dh;
  switch (stft_env_span(size, hop, F, p, dl, dh)) {
    case 1: return (float)cum[size + dl];
    case 2: return (float)cum[dh];
    default:
      return dh < size - dl ? (float)(cum[dh] - cum[dl - hop]) : (float)(cum[size + dl] - cum[size + dh + hop]);
  }
}

// ---- runs: a channel's F frames in `runs` runs of nf frames (the last one shorter) ------------------------------------
// nf: about one run per resident workgroup (`slots`), but at least 8 x the frames re-transformed at a run's start
// (overhead <= 1/8), at least one group of fpw frames, at most the channel
CLFA_PLAN_HD inline int stft_run_frames(long nframes, long slots, int size, int hop, int fpw, int F) {
  const int warm = (size + hop - 1) / hop;   // frames re-transformed at the start of a run, + 1
  long nf = (nframes + slots - 1) / slots;
  if (nf < 8L * warm) nf = 8L * warm;
  if (nf < fpw) nf = fpw;
  if (nf > F) nf = F;
  return (int)nf;
}

CLFA_PLAN_HD inline int stft_runs(int F, int nf) { return (int)(((long)F + nf - 1) / nf); }

// Run r holds the frames [s, e_end) and owns the output samples [own_lo, e_end hop) (the channel's last run: up to L).
// It transforms from frame fw, the first one that reaches sample own_lo (fw hop + size > own_lo), and discards what
// those warm-up frames sum below own_lo.
struct StftRun {
  int s, e_end, fw;
  long own_lo;
};

CLFA_PLAN_HD inline StftRun stft_run(int r, int nf, int F, int size, int hop) {
  StftRun u;
  u.s = (int)((long)r * nf);
  u.e_end = (long)u.s + nf < F ? u.s + nf : F;
  u.own_lo = (long)u.s * hop;
  u.fw = u.own_lo >= size ? (int)((u.own_lo - size) / hop + 1) : 0;
  return u;
}

}  // namespace clfa
