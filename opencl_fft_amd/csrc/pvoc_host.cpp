// pvoc_host.cpp — C ABI of the phase vocoder on the Stft spectra (see include/clfft_amd.h): Pvoc, the object — set-up, the
// states' initial values, create / destroy / reset / error / log — and spectra <-> frames.  What every call shares:
// pvoc_host.hpp; the families of calls: pvoc_frames_host.cpp, pvoc_stream_host.cpp, pvoc_rows_host.cpp,
// pvoc_signal_host.cpp.
#include "fft_route.hpp"
#include "pvoc_host.hpp"
#include "pvoc_launch.hpp"

using namespace clfa;

// the states as at creation: prev = (1, 0), theta = 0, the oscillator bank's P = W = A = 0, EMPTY bins in the smoothing's
// y, the freeze's held, the blur's history, the delay's two histories and the descriptors' previous frame (on p->stream,
// blocking).  The histories are refilled at their current length; the bank is configuration and is left alone.
static int pvoc_init_state(clfa_pvoc *p) {
  std::vector<cpx> one(pvoc_bins(p), mk(1.f, 0.f));
  HIP_TRY(hipMemcpyAsync(p->scan.prev.p, one.data(), sizeof(cpx) * one.size(), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemsetAsync(p->scan.theta.p, 0, sizeof(unsigned) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->adsyn.phase.p, 0, sizeof(unsigned long long) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->adsyn.w.p, 0, sizeof(int) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->adsyn.amp.p, 0, sizeof(float) * pvoc_bins(p), p->stream));
  const auto fill = [&](const DevBuf &b, long frames) {
    return launch_pvoc_time_fill((cpx *)b.p, (long)p->channels * frames, p->M, p->srs, p->stream);
  };
  HIP_TRY(fill(p->time.smooth, 1));
  HIP_TRY(fill(p->time.held, 1));
  HIP_TRY(fill(p->desc.last, 1));
  HIP_TRY(fill(p->time.hist, p->time.blur_max > 0 ? p->time.blur_max - 1 : 0));
  HIP_TRY(fill(p->delay.xhist, p->delay.max > 0 ? p->delay.max : 0));
  HIP_TRY(fill(p->delay.yhist, p->delay.max > 0 ? p->delay.max : 0));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

static int pvoc_setup(clfa_pvoc *p, int device, int size, int hop, double sr, int channels) {
  p->size = size;
  p->hop = hop;
  p->sr = sr;
  p->channels = channels;
  p->log[0] = 0;
  if (!is_pow2(size) || size < 64 || size > (2 << kLdsMaxLog)) {
    snprintf(p->log, sizeof(p->log), "size must be a power of two, 64..%d (got %d)", 2 << kLdsMaxLog, size);
    return CLFA_INVALID_VALUE;
  }
  if (hop < 1 || hop > size) {
    snprintf(p->log, sizeof(p->log), "hop must be 1..size (got %d)", hop);
    return CLFA_INVALID_VALUE;
  }
  if (!(sr > 0) || !std::isfinite(sr)) {
    snprintf(p->log, sizeof(p->log), "sr must be positive and finite (got %g)", sr);
    return CLFA_INVALID_VALUE;
  }
  if (channels < 1) {
    snprintf(p->log, sizeof(p->log), "channels must be >= 1 (got %d)", channels);
    return CLFA_INVALID_VALUE;
  }
  p->M = size / 2;
  p->sh = (float)((double)size / hop);
  p->srs = (float)(sr / size);
  p->kf = (float)(hop / sr);
  p->bpf = (float)(size / sr);
  p->adsyn.ks = (float)(1.0 / sr);
  p->scan.cap = pvoc_chunks_cap(p, sizeof(unsigned));              // the synthesis' chunk sums are 4 bytes each,
  p->adsyn.cap = pvoc_chunks_cap(p, sizeof(unsigned long long));   // the oscillator bank's 8
  p->ops_grid_max = (int)env_long("CLFA_PVOC_OPS_GRID_MAX", 0, 0x7fffffffL);
  p->adsyn.grid_max = (int)env_long("CLFA_PVOC_ADSYN_GRID_MAX", 0, 0x7fffffffL);
  int e = device_info(device, p->di);
  if (e) return e;
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  if ((e = upload_half(p->half, p->M)) || (e = upload_w2(p->w2, p->M, -1.f))) return e;
  std::vector<cpx> tab(p->M + 1);
  for (int k = 0; k <= p->M; k++) {
    const double a = -2 * kPI * (double)(((long)k * hop) % size) / size;
    tab[k] = mk((float)cos(a), (float)sin(a));
  }
  if ((e = upload(p->etab, tab.data(), sizeof(cpx) * tab.size()))) return e;
  const size_t bins = pvoc_bins(p);
  if ((e = p->scan.prev.ensure(sizeof(cpx) * bins)) || (e = p->scan.theta.ensure(sizeof(unsigned) * bins))) return e;
  std::vector<float> ramp(hop);
  for (int j = 1; j <= hop; j++) ramp[j - 1] = (float)((double)j / hop);
  if ((e = upload(p->adsyn.ramp, ramp.data(), sizeof(float) * ramp.size()))) return e;
  if ((e = p->adsyn.phase.ensure(sizeof(unsigned long long) * bins)) || (e = p->adsyn.w.ensure(sizeof(int) * bins)) ||
      (e = p->adsyn.amp.ensure(sizeof(float) * bins)))
    return e;
  if ((e = p->time.smooth.ensure(sizeof(cpx) * bins)) || (e = p->time.held.ensure(sizeof(cpx) * bins))) return e;
  if ((e = p->desc.last.ensure(sizeof(cpx) * bins))) return e;
  return pvoc_init_state(p);
}

// ---------------------------------------------------------------------------------
// spectra <-> (amp, freq) frames (pvoc_kernels.hip).  Unlike the frame operations, both directions answer with the
// object's own error before they look at an argument, and their blocking forms do not apply the overlap rule to the host
// arrays: a path of their own beside pvoc_call.
// ---------------------------------------------------------------------------------

using PvocConvert = HostArrays<clfa_pvoc, 2>;   // the spectra, the frames
static PvocConvert pvoc_convert(const clfa_pvoc *p, const void *spectra, const void *frames, long F, bool synthesis) {
  return {{{spectra, pvoc_spec_bytes(p, F), 8, synthesis, &clfa_pvoc::stage_spectra},
           {frames, pvoc_frame_bytes(p, F), 8, !synthesis, synthesis ? &clfa_pvoc::stage_in : &clfa_pvoc::stage_out}}};
}

// the argument rules of the two device forms; 1 = a successful no-op
static int pvoc_check(const PvocConvert &c, long F) {
  if (!pvoc_count_ok(F) || (F > 0 && !arrays_ok(c.a, true))) return CLFA_INVALID_VALUE;
  return F == 0;
}

// the blocking forms: NULL arrays are invalid values, then copies around dev(spectra, frames) on the staged arrays
template <class Dev>
static int pvoc_convert_host(clfa_pvoc *p, const void *spectra, const void *frames, long F, bool synthesis, Dev dev) {
  if (int e = obj_error(p)) return e;
  const PvocConvert c = pvoc_convert(p, spectra, frames, F, synthesis);
  if (!pvoc_count_ok(F) || (F > 0 && (!c.a[0].ptr || !c.a[1].ptr))) return CLFA_INVALID_VALUE;
  if (F == 0) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  return staged_call(p, c.a, [&](const void *const *d) { return dev(const_cast<void *>(d[0]), const_cast<void *>(d[1])); });
}

static PvocArgs pvoc_args(clfa_pvoc *p, long F) {
  PvocArgs a;
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.prev = (cpx *)p->scan.prev.p;
  a.etab = (const cpx *)p->etab.p;
  a.theta = (unsigned *)p->scan.theta.p;
  a.sums = (unsigned *)p->scan.ws.p;
  a.sh = p->sh;
  a.srs = p->srs;
  a.kf = p->kf;
  return a;
}

extern "C" {

int clfa_pvoc_create(clfa_pvoc **pv, int device, int size, int hop, double sr, int channels) {
  return create_object(pv, [&](clfa_pvoc *p) { return pvoc_setup(p, device, size, hop, sr, channels); });
}

void clfa_pvoc_destroy(clfa_pvoc *p) { destroy_object(p); }

int clfa_pvoc_get_error(const clfa_pvoc *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_pvoc_get_log(const clfa_pvoc *p) { return p ? p->log : ""; }
size_t clfa_pvoc_workspace_bytes(const clfa_pvoc *p) { return p ? p->scan.ws.bytes : 0; }
int clfa_pvoc_scan_chunk(void) { return kPvocChunk; }
const char *clfa_pvoc_kernel_name(const clfa_pvoc *p, int synthesis) {
  return !p || p->err ? "" : (synthesis ? "k_pvoc_walk" : "k_pvoc_analyze");
}

int clfa_pvoc_reset(clfa_pvoc *p) {
  if (int e = obj_error(p)) return e;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  return pvoc_init_state(p);
}

int clfa_pvoc_read_phase(clfa_pvoc *p, unsigned *host) {
  if (!p) return CLFA_INVALID_VALUE;
  return pvoc_read_state(p, CLFA_SUCCESS, {{host, &p->scan.theta, sizeof(unsigned) * pvoc_bins(p)}});
}

int clfa_pvoc_read_prev(clfa_pvoc *p, float *host) {
  if (!p) return CLFA_INVALID_VALUE;
  return pvoc_read_state(p, CLFA_SUCCESS, {{host, &p->scan.prev, sizeof(cpx) * pvoc_bins(p)}});
}

int clfa_pvoc_analyze_dev(clfa_pvoc *p, const void *spectra, void *frames_out, long F, void *stream) {
  if (int e = obj_error(p)) return e;
  return pvoc_dev_form(p, pvoc_check(pvoc_convert(p, spectra, frames_out, F, false), F), stream, [&](hipStream_t s) {
    PvocArgs a = pvoc_args(p, F);
    a.spec_in = (const cpx *)spectra;
    a.frames_out = (float *)frames_out;
    return launch_pvoc_analyze(a, p->di, s);
  });
}

int clfa_pvoc_synthesize_dev(clfa_pvoc *p, const void *frames, void *spectra_out, long F, void *stream) {
  if (int e = obj_error(p)) return e;
  return pvoc_dev_form(p, pvoc_check(pvoc_convert(p, spectra_out, frames, F, true), F), stream, [&](hipStream_t s) {
    const long held = p->scan.cap;   // the whole sub-batch workspace at the first need: its address never changes afterwards
    if (int e = ensure_workspaces({{&p->scan.ws, sizeof(unsigned) * pvoc_bins(p) * (size_t)held}}, s)) return e;
    PvocArgs a = pvoc_args(p, F);
    a.frames_in = (const float *)frames;
    a.spec_out = (cpx *)spectra_out;
    return pvoc_subbatches(F, held * kPvocChunk, [&](long f0, long nf) { return launch_pvoc_synth(a, f0, nf, p->di, s); });
  });
}

int clfa_pvoc_analyze(clfa_pvoc *p, const float *spectra, float *frames_out, long F) {
  return pvoc_convert_host(p, spectra, frames_out, F, false, [&](void *dspectra, void *dframes) {
    return clfa_pvoc_analyze_dev(p, dspectra, dframes, F, p->stream);
  });
}

int clfa_pvoc_synthesize(clfa_pvoc *p, const float *frames, float *spectra_out, long F) {
  return pvoc_convert_host(p, spectra_out, frames, F, true, [&](void *dspectra, void *dframes) {
    return clfa_pvoc_synthesize_dev(p, dframes, dspectra, F, p->stream);
  });
}

}  // extern "C"
