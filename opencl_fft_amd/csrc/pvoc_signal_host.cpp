// pvoc_signal_host.cpp — C ABI of the phase vocoder (include/clfft_amd.h), the calls with samples on one side: tanal (a
// stored signal -> frames) and adsyn (frames -> samples, the oscillator bank with its state).  Over pvoc_host.hpp's
// pvoc_call; both stage their signal rows, packed, in the signal's slot.
#include "pvoc_host.hpp"
#include "pvoc_launch.hpp"
#include "tanal_launch.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// a stored signal -> frames at given time points (tanal_kernels.hip)
// ---------------------------------------------------------------------------------

// signal: channels rows of `samples` floats, signal_stride floats apart at the caller's (the overlap rule takes the rows
// and the gaps between them as one span), packed where the blocking form stages them.  Every start has a meaning, so the
// blocking form has no values to refuse.
static int pvoc_tanal_call(clfa_pvoc *p, bool blocking, const void *signal, long signal_stride, long samples,
                           const void *window, const void *starts, void *out, long Fout, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = samples >= 1 && samples <= 0x7fffffffL && signal_stride >= samples;
  const size_t row = sizeof(float) * (size_t)(samples > 0 ? samples : 0), pitch = sizeof(float) * (size_t)(signal_stride > 0 ? signal_stride : 0);
  const PvocArray arrays[] = {{signal, row, 4, false, &clfa_pvoc::stage_signal, true, (size_t)p->channels, pitch},
                              {out, pvoc_frame_bytes(p, Fout), 8, true, &clfa_pvoc::stage_out},
                              {window, sizeof(float) * (size_t)p->size, 4, false, &clfa_pvoc::stage_table},
                              {starts, sizeof(int) * (size_t)Fout, 4, false, &clfa_pvoc::stage_itable}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    PvocTanalArgs a;
    a.logn = ilog2(p->M);
    a.M = p->M;
    a.channels = p->channels;
    a.hop = p->hop;
    a.Fout = Fout;
    a.samples = samples;
    a.stride = blocking ? samples : signal_stride;
    a.signal = (const float *)d[0];
    a.out = (cpx *)d[1];
    a.window = (const float *)d[2];
    a.starts = (const int *)d[3];
    a.etab = (const cpx *)p->etab.p;
    a.half = (const cpx *)p->half.p;
    a.w2 = (const cpx *)p->w2.p;
    a.sh = p->sh;
    a.srs = p->srs;
    a.grid_max = p->ops_grid_max;
    return launch_pvoc_tanal(a, p->di, s);
  };
  return pvoc_call(p, blocking, stream, scalars_ok, Fout, arrays, CLFA_SUCCESS, pvoc_no_values, launch);
}

extern "C" {

int clfa_pvoc_tanal_dev(clfa_pvoc *p, const void *signal, long signal_stride, long samples, const void *window,
                        const void *starts, void *frames_out, long Fout, void *stream) {
  return pvoc_tanal_call(p, false, signal, signal_stride, samples, window, starts, frames_out, Fout, stream);
}
int clfa_pvoc_tanal(clfa_pvoc *p, const float *signal, long signal_stride, long samples, const float *window,
                    const int *starts, float *frames_out, long Fout) {
  return pvoc_tanal_call(p, true, signal, signal_stride, samples, window, starts, frames_out, Fout, nullptr);
}
const char *clfa_pvoc_tanal_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_tanal"; }

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> samples: the oscillator bank (pvoc_adsyn.hip)
// ---------------------------------------------------------------------------------

static size_t pvoc_adsyn_ws_bytes(const clfa_pvoc *p) {
  return sizeof(unsigned long long) * pvoc_bins(p) * (size_t)p->adsyn.cap + (sizeof(int) + sizeof(float)) * pvoc_bins(p);
}

// signal: channels rows of F hop floats, signal_stride floats apart at the caller's (the overlap rule takes the rows and
// the gaps between them as one span), packed where the blocking form stages them.  A NULL fmod is none.
static int pvoc_adsyn_call(clfa_pvoc *p, bool blocking, const void *frames, long F, const void *fmod, int first_bin, int nbins,
                           int step, float gain, void *signal, long signal_stride, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = step >= 1 && nbins >= 1 && first_bin >= 0 && (long)first_bin + ((long)nbins - 1) * step <= p->M &&
                          pvoc_count_ok(F) && signal_stride >= F * p->hop;
  const size_t row = sizeof(float) * (size_t)F * p->hop, pitch = sizeof(float) * (size_t)signal_stride;
  const PvocArray arrays[] = {{frames, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::stage_in},
                              {signal, row, 4, true, &clfa_pvoc::stage_signal, true, (size_t)p->channels, pitch},
                              {fmod, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::stage_fmod, fmod != nullptr}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    clfa_pvoc::Adsyn &o = p->adsyn;
    const long held = o.cap;   // the whole workspace at the first need: its address never changes afterwards
    if (int e = ensure_workspaces({{&o.ws, pvoc_adsyn_ws_bytes(p)}}, s)) return e;
    PvocAdsynArgs a;
    a.M = p->M;
    a.channels = p->channels;
    a.hop = p->hop;
    a.F = F;
    a.frames = (const float *)d[0];
    a.fmod = (const float *)d[2];
    a.first = first_bin;
    a.nbins = nbins;
    a.step = step;
    a.gain = gain;
    a.ks = o.ks;
    a.phase = (unsigned long long *)o.phase.p;
    a.w = (int *)o.w.p;
    a.amp = (float *)o.amp.p;
    a.sums = (unsigned long long *)o.ws.p;
    a.w0 = (int *)(a.sums + pvoc_bins(p) * (size_t)held);
    a.a0 = (float *)(a.w0 + pvoc_bins(p));
    a.ramp = (const float *)o.ramp.p;
    a.signal = (float *)d[1];
    a.sstride = blocking ? F * p->hop : signal_stride;
    a.grid_max = o.grid_max;
    return pvoc_subbatches(F, held * kPvocChunk, [&](long f0, long nf) { return launch_pvoc_adsyn(a, f0, nf, p->di, s); });
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, pvoc_no_values, launch);
}

extern "C" {

int clfa_pvoc_adsyn_dev(clfa_pvoc *p, const void *frames, long F, const void *fmod, int first_bin, int nbins, int step,
                        float gain, void *signal, long signal_stride, void *stream) {
  return pvoc_adsyn_call(p, false, frames, F, fmod, first_bin, nbins, step, gain, signal, signal_stride, stream);
}
int clfa_pvoc_adsyn(clfa_pvoc *p, const float *frames, long F, const float *fmod, int first_bin, int nbins, int step,
                    float gain, float *signal, long signal_stride) {
  return pvoc_adsyn_call(p, true, frames, F, fmod, first_bin, nbins, step, gain, signal, signal_stride, nullptr);
}

int clfa_pvoc_adsyn_read_state(clfa_pvoc *p, unsigned long long *phase, int *w, float *amp) {
  if (!p) return CLFA_INVALID_VALUE;
  const size_t bins = pvoc_bins(p);
  return pvoc_read_state(p, CLFA_SUCCESS, {{phase, &p->adsyn.phase, sizeof(unsigned long long) * bins},
                                           {w, &p->adsyn.w, sizeof(int) * bins},
                                           {amp, &p->adsyn.amp, sizeof(float) * bins}});
}

size_t clfa_pvoc_adsyn_workspace_bytes(const clfa_pvoc *p) { return p ? p->adsyn.ws.bytes : 0; }
int clfa_pvoc_adsyn_tile_bins(void) { return kAdsynTile; }
const char *clfa_pvoc_adsyn_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_adsyn_osc"; }

}  // extern "C"
