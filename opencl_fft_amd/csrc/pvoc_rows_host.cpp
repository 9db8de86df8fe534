// pvoc_rows_host.cpp — C ABI of the phase vocoder (include/clfft_amd.h), the calls from frames to rows of values per frame:
// desc (with its carried state), bands (with the bank's set-up) and pitch.  Over pvoc_host.hpp's pvoc_call,
// pvoc_family_setup and pvoc_read_state; the rows are staged in one slot, pitch's peak list in the output list's.
#include "bank_launch.hpp"
#include "bank_plan.hpp"
#include "pitch_launch.hpp"
#include "pvoc_host.hpp"
#include "pvoc_launch.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// frames -> eight descriptors per frame, with carried state (pvoc_desc.hip)
// ---------------------------------------------------------------------------------

static int pvoc_desc_call(clfa_pvoc *p, bool blocking, const void *in, void *desc, long F, int first_bin, int nbins,
                          int rectify, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M && (rectify == 0 || rectify == 1);
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::stage_in},
                              {desc, 8 * sizeof(float) * (size_t)p->channels * (size_t)F, 4, true, &clfa_pvoc::stage_out_rows}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    PvocDescArgs a;
    pvoc_frames_args(p, F, a);
    a.in = (const cpx *)d[0];
    a.desc = (float *)d[1];
    a.last = (cpx *)p->desc.last.p;
    a.lo = first_bin;
    a.hi = first_bin + nbins - 1;
    a.rectify = rectify;
    a.cf = p->srs;
    return launch_pvoc_desc(a, p->di, s);
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, pvoc_no_values, launch);
}

extern "C" {

int clfa_pvoc_desc_dev(clfa_pvoc *p, const void *frames_in, void *desc, long F, int first_bin, int nbins, int rectify,
                       void *stream) {
  return pvoc_desc_call(p, false, frames_in, desc, F, first_bin, nbins, rectify, stream);
}
int clfa_pvoc_desc(clfa_pvoc *p, const float *frames_in, float *desc, long F, int first_bin, int nbins, int rectify) {
  return pvoc_desc_call(p, true, frames_in, desc, F, first_bin, nbins, rectify, nullptr);
}

// the amps of the previous frame: the first of every pair the device holds.  The object's error is asked here as well as
// on the shared path: the pairs' count is the object's, which only a good object has
int clfa_pvoc_desc_read_state(clfa_pvoc *p, float *host) {
  if (int e = obj_error(p)) return e;
  if (!host) return CLFA_INVALID_VALUE;
  std::vector<cpx> pairs(pvoc_bins(p));
  if (int e = pvoc_read_state(p, CLFA_SUCCESS, {{pairs.data(), &p->desc.last, sizeof(cpx) * pairs.size()}})) return e;
  for (size_t i = 0; i < pairs.size(); i++) host[i] = pairs[i].x;
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_desc_state_bytes(const clfa_pvoc *p) { return p ? p->desc.last.bytes : 0; }
const char *clfa_pvoc_desc_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_desc"; }

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> band energies, their log, a DCT of that (bank_kernels.hip)
// ---------------------------------------------------------------------------------

// whether the bank has been set up: asked after the arguments
static int pvoc_bank_ready(const clfa_pvoc *p) { return p->bank.B < 0 ? CLFA_INVALID_OPERATION : CLFA_SUCCESS; }

// floor is looked at with LOG only; ncoef is 1..B with DCT (before the setup: 1..256, what a setup can make valid), else 0.
// The output rows hold ncoef values with DCT, else B (before the setup the check takes rows of one value).
static int pvoc_bands_call(clfa_pvoc *p, bool blocking, const void *in, void *out, long F, int flags, int ncoef, float floor,
                           void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const int all = CLFA_PVOC_BANDS_POWER | CLFA_PVOC_BANDS_LOG | CLFA_PVOC_BANDS_DCT;
  const bool lg = flags & CLFA_PVOC_BANDS_LOG, dct = flags & CLFA_PVOC_BANDS_DCT;
  const clfa_pvoc::Bank &k = p->bank;
  const bool scalars_ok = !(flags & ~all) && (!lg || (std::isfinite(floor) && floor > 0.f)) &&
                          (dct ? ncoef >= 1 && ncoef <= (k.B >= 0 ? k.B : kBankMax) : ncoef == 0);
  const size_t N = dct ? (size_t)(ncoef > 0 ? ncoef : 0) : (size_t)(k.B > 0 ? k.B : 1);
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::stage_in},
                              {out, sizeof(float) * (size_t)p->channels * (size_t)F * N, 4, true, &clfa_pvoc::stage_out_rows}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    BankArgs a;
    a.M = p->M;
    a.channels = p->channels;
    a.F = F;
    a.in = (const cpx *)d[0];
    a.out = (float *)d[1];
    a.B = k.B;
    a.steps = k.steps;
    a.bands = (const int *)k.bands.p;
    a.sched = (const int *)k.sched.p;
    a.weights = (const float *)k.weights.p;
    a.dct_t = (const float *)k.dct.p;
    a.power = (flags & CLFA_PVOC_BANDS_POWER) != 0;
    a.log = lg;
    a.dct = dct;
    a.ncoef = ncoef;
    a.floor = floor;
    a.grid_max = p->ops_grid_max;
    return launch_pvoc_bands(a, p->di, s);
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, pvoc_bank_ready(p), pvoc_no_values, launch);
}

extern "C" {

int clfa_pvoc_bank_setup(clfa_pvoc *p, int nbands, const int *first, const int *count, const float *weights) {
  int steps = 0;
  return pvoc_family_setup<4>(
      p, [&] { return bank_ok(p->M, nbands, first, count, weights); },
      [&](DevBuf(&fresh)[4]) {   // the bands, the schedule, the weights, the DCT table
        const std::vector<BankBand> bands = bank_bands(nbands, first, count);
        const std::vector<int> sched = bank_schedule(nbands, count);
        const std::vector<float> D = bank_dct(nbands);
        std::vector<float> Dt(D.size());   // the kernel's lanes of neighbouring q read neighbouring words
        for (int q = 0; q < nbands; q++)
          for (int b = 0; b < nbands; b++) Dt[(size_t)b * nbands + q] = D[(size_t)q * nbands + b];
        const size_t nweights = (size_t)bands.back().woff + bands.back().count;
        for (int r = 0; r < kBankRows; r++) steps = std::max(steps, sched[r + 1] - sched[r]);
        const void *src[4] = {bands.data(), sched.data(), weights, Dt.data()};
        const size_t bytes[4] = {sizeof(BankBand) * bands.size(), sizeof(int) * sched.size(), sizeof(float) * nweights,
                                 sizeof(float) * Dt.size()};
        for (int i = 0; i < 4; i++)
          if (int e = upload(fresh[i], src[i], bytes[i])) return e;
        return CLFA_SUCCESS;
      },
      [&](DevBuf(&fresh)[4]) {
        DevBuf *const mine[4] = {&p->bank.bands, &p->bank.sched, &p->bank.weights, &p->bank.dct};
        for (int i = 0; i < 4; i++) mine[i]->swap(fresh[i]);
        p->bank.B = nbands;
        p->bank.steps = steps;
      });
}

int clfa_pvoc_bank_bands(const clfa_pvoc *p) { return p ? p->bank.B : -1; }

// the table the device uses, D[q][b]: the device keeps it transposed
int clfa_pvoc_bank_read_dct(clfa_pvoc *p, float *host) {
  if (!p || !host) return CLFA_INVALID_VALUE;
  const size_t B = p->bank.B > 0 ? p->bank.B : 0;
  std::vector<float> Dt(B ? B * B : 1);   // never empty: before the set-up the shared path answers, not a NULL array
  if (int e = pvoc_read_state(p, pvoc_bank_ready(p), {{Dt.data(), &p->bank.dct, sizeof(float) * B * B}})) return e;
  for (size_t q = 0; q < B; q++)
    for (size_t b = 0; b < B; b++) host[q * B + b] = Dt[b * B + q];
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_bank_state_bytes(const clfa_pvoc *p) {
  return p ? p->bank.bands.bytes + p->bank.sched.bytes + p->bank.weights.bytes + p->bank.dct.bytes : 0;
}

int clfa_pvoc_bands_dev(clfa_pvoc *p, const void *frames_in, void *out, long F, int flags, int ncoef, float floor, void *stream) {
  return pvoc_bands_call(p, false, frames_in, out, F, flags, ncoef, floor, stream);
}
int clfa_pvoc_bands(clfa_pvoc *p, const float *frames_in, float *out, long F, int flags, int ncoef, float floor) {
  return pvoc_bands_call(p, true, frames_in, out, F, flags, ncoef, floor, nullptr);
}
const char *clfa_pvoc_bands_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_bands"; }

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> four values per frame: the pitch from the frame's spectral peaks, and the peak list (pitch_kernels.hip)
// ---------------------------------------------------------------------------------

// A call with two outputs: the rows, and the list where `peaks` is given.  All its parameters are scalars, so the
// blocking form has no values to refuse.  The negated comparisons refuse a NaN.
static int pvoc_pitch_call(clfa_pvoc *p, bool blocking, const void *in, void *rows, void *peaks, long F, int first_bin,
                           int nbins, int npeaks, float thresh, float fmin, float fmax, float tol, float decay, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = first_bin >= 1 && nbins >= 1 && (long)first_bin + nbins <= p->M && npeaks >= 1 &&
                          npeaks <= CLFA_PVOC_PITCH_PEAKS_MAX && thresh >= 0.f && std::isfinite(thresh) &&
                          std::isnormal(fmin) && fmin > 0.f && std::isfinite(fmax) && fmin <= fmax && tol >= 0.f &&
                          tol <= 0.5f && decay > 0.f && decay <= 1.f;
  const size_t frames = (size_t)p->channels * (size_t)(F > 0 ? F : 0);
  const size_t pbytes = peaks && scalars_ok ? 2 * sizeof(float) * frames * (size_t)npeaks : 0;
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::stage_in},
                              {rows, 4 * sizeof(float) * frames, 4, true, &clfa_pvoc::stage_out_rows},
                              {peaks, pbytes, 8, true, &clfa_pvoc::stage_out_list, peaks != nullptr}};
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, pvoc_no_values, [&](const void *const *d, hipStream_t s) {
    PvocPitchArgs a;
    a.M = p->M;
    a.channels = p->channels;
    a.F = F;
    a.grid_max = p->ops_grid_max;
    a.in = (const cpx *)d[0];
    a.rows = (float *)d[1];
    a.peaks = (cpx *)d[2];
    a.npeaks = npeaks;
    a.lo = first_bin;
    a.hi = first_bin + nbins - 1;
    a.thresh = thresh;
    a.fmin = fmin;
    a.fmax = fmax;
    a.tol = tol;
    for (int h = 1; h <= CLFA_PVOC_PITCH_HARM; h++) a.weights.w[h - 1] = (float)pow((double)decay, h - 1);
    return launch_pvoc_pitch(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_pitch_dev(clfa_pvoc *p, const void *frames_in, void *rows, void *peaks, long F, int first_bin, int nbins,
                        int npeaks, float thresh, float fmin, float fmax, float tol, float decay, void *stream) {
  return pvoc_pitch_call(p, false, frames_in, rows, peaks, F, first_bin, nbins, npeaks, thresh, fmin, fmax, tol, decay, stream);
}
int clfa_pvoc_pitch(clfa_pvoc *p, const float *frames_in, float *rows, float *peaks, long F, int first_bin, int nbins,
                    int npeaks, float thresh, float fmin, float fmax, float tol, float decay) {
  return pvoc_pitch_call(p, true, frames_in, rows, peaks, F, first_bin, nbins, npeaks, thresh, fmin, fmax, tol, decay, nullptr);
}
const char *clfa_pvoc_pitch_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_pitch"; }

}  // extern "C"
