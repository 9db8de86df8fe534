// stft_host.cpp — C ABI of the short-time transforms (see include/clfft_amd.h): Stft.  Shared plumbing: host.hpp, where
// the staged blocking form lives; the rules of a call's arrays: overlap.hpp.
#include "fft_route.hpp"
#include "host.hpp"
#include "stft_launch.hpp"
#include "stft_plan.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// short-time analysis / overlap-add synthesis (stft_kernels.hip)
// ---------------------------------------------------------------------------------

struct clfa_stft {
  DeviceInfo di;
  int size = 0, hop = 0, logn = 0;
  int grid_max = 0;   // cap on a launch's workgroups (CLFA_STFT_GRID_MAX: tuning and test switch, read at creation)
  bool fwd = true;
  int err = 0;
  char log[512];
  hipStream_t stream = nullptr;
  DevBuf half, w2, win, cum;   // Clrfft tables of the direction, the window, its running sums of squares (synthesis, double)
  DevBuf sig, spec;            // staging of the blocking forms (stft_arrays)
  StreamOrder order;
};

static int stft_setup(clfa_stft *p, int device, int size, int hop, const float *window, bool fwd) {
  p->size = size;
  p->hop = hop;
  p->fwd = fwd;
  p->log[0] = 0;
  if (!is_pow2(size) || size < 64 || size > (2 << kLdsMaxLog)) {
    snprintf(p->log, sizeof(p->log), "size must be a power of two, 64..%d (got %d)", 2 << kLdsMaxLog, size);
    return CLFA_INVALID_VALUE;
  }
  if (hop < 1 || hop > size) {
    snprintf(p->log, sizeof(p->log), "hop must be 1..size (got %d)", hop);
    return CLFA_INVALID_VALUE;
  }
  const int m = size / 2;
  p->logn = ilog2(m);
  p->grid_max = (int)env_long("CLFA_STFT_GRID_MAX", 0, 0x7fffffffL);
  int e = device_info(device, p->di);
  if (e) return e;
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  if ((e = upload_half(p->half, m)) || (e = upload_w2(p->w2, m, fwd ? -1.f : 1.f))) return e;
  std::vector<float> w(window ? window : nullptr, window ? window + size : nullptr);
  if (!window) w.assign(size, 1.0f);
  if ((e = upload(p->win, w.data(), sizeof(float) * size))) return e;
  if (!fwd) {
    // the envelope's two running sums of w^2, kept in double: the kernel rounds once, after its lookup
    std::vector<double> c(2 * (size_t)size);
    stft_env_table(w.data(), size, hop, c.data());
    if ((e = upload(p->cum, c.data(), sizeof(double) * c.size()))) return e;
  }
  return CLFA_SUCCESS;
}

static long stft_frames_of(int size, int hop, long samples) { return samples < size ? 0 : 1 + (samples - size) / hop; }

// The two arrays of either direction (HostArrays, host.hpp): the signal, `channels` rows of `len` floats — with one
// channel the caller's stride is not used, the pitch is the row length — and the packed spectra of F frames per channel.
// The analysis writes the spectra, the synthesis the signal.
using StftArrays = HostArrays<clfa_stft, 2>;
static StftArrays stft_arrays(const clfa_stft *p, const void *signal, long stride, long len, const void *spectra, long F, long channels) {
  const size_t row = sizeof(float) * (size_t)len, pitch = channels > 1 ? sizeof(float) * (size_t)stride : row;
  return {{{signal, row, 4, !p->fwd, &clfa_stft::sig, true, (size_t)channels, pitch},
           {spectra, sizeof(cpx) * (size_t)F * channels * (p->size / 2), 8, p->fwd, &clfa_stft::spec}}};
}

// spectra of `frames` frames per channel; a grid of at most 2^31 - 1 frames (more would not fit a device)
static int stft_run(clfa_stft *p, StftArgs &a, long frames, long channels, hipStream_t s) {
  if (frames > 0x7fffffffL || channels > 0x7fffffffL || frames * channels > 0x7fffffffL) return CLFA_INVALID_VALUE;
  a.logn = p->logn;
  a.forward = p->fwd;
  a.hop = p->hop;
  a.F = (int)frames;
  a.channels = channels;
  a.nframes = frames * channels;
  a.window = (const float *)p->win.p;
  a.cum = (const double *)p->cum.p;
  a.grid_max = p->grid_max;
  a.half = (const cpx *)p->half.p;
  a.w2 = (const cpx *)p->w2.p;
  HIP_TRY(p->order.use(s));
  HIP_TRY(launch_stft(a, p->di, s));
  return CLFA_SUCCESS;
}

extern "C" {

int clfa_stft_create(clfa_stft **st, int device, int size, int hop, const float *window, int forward) {
  return create_object(st, [&](clfa_stft *p) { return stft_setup(p, device, size, hop, window, forward != 0); });
}

void clfa_stft_destroy(clfa_stft *p) { destroy_object(p); }

int clfa_stft_get_error(const clfa_stft *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_stft_get_log(const clfa_stft *p) { return p ? p->log : ""; }
// (valid size and hop: logn is set; the formulas need no device)
long clfa_stft_frames(const clfa_stft *p, long samples) { return p && p->logn && samples >= 0 ? stft_frames_of(p->size, p->hop, samples) : 0; }
long clfa_stft_samples(const clfa_stft *p, long frames) { return p && p->logn && frames > 0 ? (frames - 1) * p->hop + p->size : 0; }
size_t clfa_stft_workspace_bytes(const clfa_stft *p) {
  (void)p;
  return 0;   // the analysis reads the signal in place; the synthesis sums in LDS
}
const char *clfa_stft_kernel_name(const clfa_stft *p) { return !p ? "" : (p->fwd ? "k_stft_analyze" : "k_stft_synth"); }

int clfa_stft_analyze_dev(clfa_stft *p, const void *signal, long signal_stride, long samples, long channels, void *spectra,
                          void *stream) {
  if (int e = obj_error(p)) return e;
  if (!p->fwd || samples < 0 || channels < 0) return CLFA_INVALID_VALUE;
  const long F = stft_frames_of(p->size, p->hop, samples);
  if (F == 0 || channels == 0) return CLFA_SUCCESS;
  const StftArrays io = stft_arrays(p, signal, signal_stride, samples, spectra, F, channels);
  if ((channels > 1 && signal_stride < samples) || !arrays_ok(io.a, true)) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  StftArgs a;
  a.signal = (const float *)signal;
  a.stride = signal_stride;
  a.spec_out = (cpx *)spectra;
  a.aligned8 = ((uintptr_t)signal & 7) == 0 && (p->hop & 1) == 0 && (channels == 1 || (signal_stride & 1) == 0);
  return stft_run(p, a, F, channels, (hipStream_t)stream);
}

int clfa_stft_synthesize_dev(clfa_stft *p, const void *spectra, long frames, long channels, void *signal, long signal_stride,
                             int normalize, void *stream) {
  if (int e = obj_error(p)) return e;
  if (p->fwd || frames < 0 || channels < 0) return CLFA_INVALID_VALUE;
  if (frames == 0 || channels == 0) return CLFA_SUCCESS;
  const long L = (frames - 1) * p->hop + p->size;
  const StftArrays io = stft_arrays(p, signal, signal_stride, L, spectra, frames, channels);
  if ((channels > 1 && signal_stride < L) || !arrays_ok(io.a, true)) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  StftArgs a;
  a.spec_in = (const cpx *)spectra;
  a.out = (float *)signal;
  a.stride = signal_stride;
  a.normalize = normalize != 0;
  return stft_run(p, a, frames, channels, (hipStream_t)stream);
}

// the blocking forms: a NULL array is refused before the no-op; the staged rows are packed (device stride = row length)
int clfa_stft_analyze(clfa_stft *p, const float *signal, long signal_stride, long samples, long channels, float *spectra) {
  if (int e = obj_error(p)) return e;
  if (!p->fwd || !signal || !spectra || samples < 0 || channels < 0 || (channels > 1 && signal_stride < samples))
    return CLFA_INVALID_VALUE;
  const long F = stft_frames_of(p->size, p->hop, samples);
  if (F == 0 || channels == 0) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  return staged_call(p, stft_arrays(p, signal, signal_stride, samples, spectra, F, channels).a, [&](const void *const *d) {
    return clfa_stft_analyze_dev(p, d[0], samples, samples, channels, const_cast<void *>(d[1]), p->stream);
  });
}

int clfa_stft_synthesize(clfa_stft *p, const float *spectra, long frames, long channels, float *signal, long signal_stride,
                         int normalize) {
  if (int e = obj_error(p)) return e;
  if (p->fwd || !signal || !spectra || frames < 0 || channels < 0) return CLFA_INVALID_VALUE;
  if (frames == 0 || channels == 0) return CLFA_SUCCESS;
  const long L = (frames - 1) * p->hop + p->size;
  if (channels > 1 && signal_stride < L) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  return staged_call(p, stft_arrays(p, signal, signal_stride, L, spectra, frames, channels).a, [&](const void *const *d) {
    return clfa_stft_synthesize_dev(p, d[1], frames, channels, const_cast<void *>(d[0]), L, normalize, p->stream);
  });
}

}  // extern "C"
