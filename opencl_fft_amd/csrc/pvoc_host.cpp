// pvoc_host.cpp — C ABI of the phase vocoder on the Stft spectra (see include/clfft_amd.h): Pvoc.  Shared plumbing: host.hpp.
// The object and its states come first; then what every call shares — the description of its arrays (PvocArray: host.hpp's
// HostArray, checked by arrays_ok, staged by staged_call), the device form, and pvoc_call, which puts a call's results in
// the header's order — then one function per family of calls: scalar rules, array list, per-frame value rule, launch.
#include "bank_launch.hpp"
#include "bank_plan.hpp"
#include "fft_route.hpp"
#include "host.hpp"
#include "pitch_launch.hpp"
#include "pvoc_launch.hpp"
#include "tanal_launch.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// The object, its setup and its states
// ---------------------------------------------------------------------------------

struct clfa_pvoc {
  DeviceInfo di;
  int size = 0, hop = 0, M = 0, channels = 0;
  double sr = 0;
  float sh = 0.f, srs = 0.f, kf = 0.f;   // size / hop, sr / size, hop / sr: divided in double, rounded once
  int err = 0;
  char log[512];
  hipStream_t stream = nullptr;
  DevBuf etab;            // e[k], M + 1 complex
  DevBuf prev, theta;     // the two states: channels x (M + 1) complex / uint32
  DevBuf ws;              // the scan's chunk sums: allocated by the first synthesis that needs it
  long cap = 1;           // chunks per sub-batch (CLFA_PVOC_CHUNKS_MAX: tuning switch, read at creation)
  DevBuf sspec, sframes;  // staging of the host entry points
  // the frame operations (pvoc_ops.hip): size / sr, the Clrfft tables of size (forward sign) for the formant envelope,
  // the cap on a launch's workgroups (CLFA_PVOC_OPS_GRID_MAX, 0 = none), staging of their host forms
  float bpf = 0.f;
  DevBuf half, w2;
  int ops_grid_max = 0;
  DevBuf sop_out, sop_par;
  DevBuf spair_b, spair_q;   // the two-input operations (pvoc_pair.hip): staging of the second input and per-frame array
  DevBuf sshape_tab;         // the shaping operations (pvoc_shape.hip): staging of the table (their rows go to sop_par)
  // the oscillator bank (pvoc_adsyn.hip): 1 / sr, its state per channel and bin (P uint64, W int32, A float32), the ramp
  // w_j, its own workspace (the 64-bit chunk sums of one sub-batch, then the endpoints a sub-batch starts from), the
  // chunks per sub-batch, the cap on its workgroups (CLFA_PVOC_ADSYN_GRID_MAX, 0 = none), staging of the host form
  float ks = 0.f;
  DevBuf aphase, aw, aamp, ramp, aws;
  long acap = 1;
  int adsyn_grid_max = 0;
  DevBuf sfmod, ssig;
  // the operations along the frames (pvoc_time.hip): the smoothing's y and the freeze's held, channels x (M + 1) pairs
  // each; the blur's history of max_frames - 1 frames per channel and its spare (clfa_pvoc_blur_setup; blur_max 0 before)
  DevBuf tsmooth, theld, bhist, bspare;
  int blur_max = 0;
  // the per-bin delay (pvoc_delay.hip): the last delay_max input frames and the last delay_max output frames per channel,
  // the spare their commits share (clfa_pvoc_delay_setup; delay_max -1 before: 0 is a setup too), staging of the delays
  DevBuf dxhist, dyhist, dspare;
  int delay_max = -1;
  DevBuf sdelay_tab;
  // the descriptors (pvoc_desc.hip): the stream's previous frame, channels x (M + 1) pairs of which the amps are the
  // state `last`; staging of the host form's rows
  DevBuf dlast, sdesc;
  DevBuf strace_bins;   // the N loudest bins (pvoc_trace.hip): staging of the host form's bin list
  DevBuf sdemix_az;     // the stereo demix (pvoc_demix.hip): staging of the host form's azimuth profile
  DevBuf spitch_rows, spitch_peaks;   // the pitch (pitch_kernels.hip): staging of the host form's rows and peak list
  // the filter bank (bank_kernels.hip; clfa_pvoc_bank_setup, bank_B -1 before): the bands, the schedule that deals them to
  // the kernel's rows (bank_steps: its longest row), the weights and the DCT table, transposed; staging of the host
  // form's rows.  Configuration, not stream state: clfa_pvoc_reset leaves it alone
  DevBuf kbands, ksched, kweights, kdct, sbands;
  int bank_B = -1, bank_steps = 0;
  StreamOrder order;
};

static size_t pvoc_bins(const clfa_pvoc *p) { return (size_t)p->channels * (p->M + 1); }
static size_t pvoc_frame_bytes(const clfa_pvoc *p, long F) { return 2 * sizeof(float) * pvoc_bins(p) * (size_t)F; }
static size_t pvoc_spec_bytes(const clfa_pvoc *p, long F) { return sizeof(cpx) * (size_t)p->channels * (size_t)F * p->M; }
static bool pvoc_count_ok(long F) { return F >= 0 && F <= 0x7fffffffL; }   // a frame count

// chunks per sub-batch: sub-batches bound a scan's workspace (`word` bytes per channel, chunk and bin) to about 64 MiB;
// CLFA_PVOC_CHUNKS_MAX (tuning switch, read at creation) lowers it
static long pvoc_chunks_cap(const clfa_pvoc *p, size_t word) {
  long cap = (64L << 20) / ((long)word * (long)pvoc_bins(p));
  cap = cap < 1 ? 1 : (cap > 4096 ? 4096 : cap);
  if (const long v = env_long("CLFA_PVOC_CHUNKS_MAX", 0, cap)) cap = v;
  return cap;
}

// launch(f0, nf) over the call's F frames in sub-batches of at most `held` chunks: each advances the state by its frames,
// the next one starts from there
template <class Launch>
static int pvoc_subbatches(long F, long held, Launch launch) {
  for (long f0 = 0; f0 < F; f0 += held * kPvocChunk) {
    const long nf = F - f0 < held * kPvocChunk ? F - f0 : held * kPvocChunk;
    HIP_TRY(launch(f0, nf));
  }
  return CLFA_SUCCESS;
}

// the states as at creation: prev = (1, 0), theta = 0, the oscillator bank's P = W = A = 0, EMPTY bins in the smoothing's
// y, the freeze's held, the blur's history, the delay's two histories and the descriptors' previous frame (on p->stream,
// blocking)
static int pvoc_init_state(clfa_pvoc *p) {
  std::vector<cpx> one(pvoc_bins(p), mk(1.f, 0.f));
  HIP_TRY(hipMemcpyAsync(p->prev.p, one.data(), sizeof(cpx) * one.size(), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemsetAsync(p->theta.p, 0, sizeof(unsigned) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->aphase.p, 0, sizeof(unsigned long long) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->aw.p, 0, sizeof(int) * pvoc_bins(p), p->stream));
  HIP_TRY(hipMemsetAsync(p->aamp.p, 0, sizeof(float) * pvoc_bins(p), p->stream));
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->tsmooth.p, p->channels, p->M, p->srs, p->stream));
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->theld.p, p->channels, p->M, p->srs, p->stream));
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->dlast.p, p->channels, p->M, p->srs, p->stream));
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->bhist.p, (long)p->channels * (p->blur_max > 0 ? p->blur_max - 1 : 0), p->M, p->srs, p->stream));
  const long delay_rows = (long)p->channels * (p->delay_max > 0 ? p->delay_max : 0);
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->dxhist.p, delay_rows, p->M, p->srs, p->stream));
  HIP_TRY(launch_pvoc_time_fill((cpx *)p->dyhist.p, delay_rows, p->M, p->srs, p->stream));
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
  p->ks = (float)(1.0 / sr);
  p->cap = pvoc_chunks_cap(p, sizeof(unsigned));              // the synthesis' chunk sums are 4 bytes each,
  p->acap = pvoc_chunks_cap(p, sizeof(unsigned long long));   // the oscillator bank's 8
  p->ops_grid_max = (int)env_long("CLFA_PVOC_OPS_GRID_MAX", 0, 0x7fffffffL);
  p->adsyn_grid_max = (int)env_long("CLFA_PVOC_ADSYN_GRID_MAX", 0, 0x7fffffffL);
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
  if ((e = p->prev.ensure(sizeof(cpx) * pvoc_bins(p))) || (e = p->theta.ensure(sizeof(unsigned) * pvoc_bins(p)))) return e;
  std::vector<float> ramp(hop);
  for (int j = 1; j <= hop; j++) ramp[j - 1] = (float)((double)j / hop);
  if ((e = upload(p->ramp, ramp.data(), sizeof(float) * ramp.size()))) return e;
  if ((e = p->aphase.ensure(sizeof(unsigned long long) * pvoc_bins(p))) || (e = p->aw.ensure(sizeof(int) * pvoc_bins(p))) ||
      (e = p->aamp.ensure(sizeof(float) * pvoc_bins(p))))
    return e;
  if ((e = p->tsmooth.ensure(sizeof(cpx) * pvoc_bins(p))) || (e = p->theld.ensure(sizeof(cpx) * pvoc_bins(p)))) return e;
  if ((e = p->dlast.ensure(sizeof(cpx) * pvoc_bins(p)))) return e;
  return pvoc_init_state(p);
}

// the object's earlier work is complete (blocking); refused while its stream is being captured
static int pvoc_quiesce(clfa_pvoc *p) {
  if (!p->order.any) return CLFA_SUCCESS;
  if (StreamOrder::capturing(p->order.last)) return CLFA_INVALID_OPERATION;
  if (hipStreamSynchronize(p->order.last) != hipSuccess) {   // a stream the caller has destroyed: wait for the device
    (void)hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
  }
  return CLFA_SUCCESS;
}

// the blocking read of states: NULL arguments are invalid values, the object's earlier work is waited for
struct PvocState {
  void *host;
  DevBuf clfa_pvoc::*buf;
  size_t word;   // bytes per channel and bin
};
static int pvoc_read_state(clfa_pvoc *p, std::initializer_list<PvocState> states) {
  if (int e = obj_error(p)) return e;
  for (const PvocState &st : states)
    if (!st.host) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  for (const PvocState &st : states) HIP_TRY(hipMemcpy(st.host, (p->*st.buf).p, st.word * pvoc_bins(p), hipMemcpyDeviceToHost));
  return CLFA_SUCCESS;
}

// The results of the argument checks: 0 = go on, 1 = a successful no-op, < 0 = the error.  A call goes on after its
// device-free checks with the error, else the object's own error, else chk:
//   if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
static int pvoc_gate(const clfa_pvoc *p, int chk) { return chk < 0 ? chk : (p->err ? p->err : chk); }
static int pvoc_done(int e) { return e == 1 ? CLFA_SUCCESS : e; }

// what a launch answers, as a status
static int pvoc_code(int e) { return e; }
static int pvoc_code(hipError_t e) {
  HIP_TRY(e);
  return CLFA_SUCCESS;
}

// ---------------------------------------------------------------------------------
// One description of a call, checked, staged and handed to the launch from one place
// ---------------------------------------------------------------------------------

// One array of a call (HostArray, host.hpp; the rules: arrays_ok, overlap.hpp): the outputs are one, or two (trace's
// frames and bin list, demix's frames and profile, pitch's rows and peak list); what an op does not look at is not `used`: MIX's p and q, BLUR's q, most tables, a NULL fmod
using PvocArray = HostArray<clfa_pvoc>;

// The device forms after their checks (chk): the error, else the object's own, else a no-op's success, ahead of any device
// work; then launch(stream) on the object's device, ordered behind the object's earlier work
template <class Launch>
static int pvoc_dev_form(clfa_pvoc *p, int chk, void *stream, Launch launch) {
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  return pvoc_code(launch(s));
}

// The object can take a call's arguments at all: a NULL object is an invalid value, one whose creation arguments were bad
// (M == 0) answers with that error.  One that only found no device goes on: a bad argument is still an invalid value there,
// which is why a call's checks come before the object's own error.
static int pvoc_usable(const clfa_pvoc *p) {
  if (!p) return CLFA_INVALID_VALUE;
  return p->M ? CLFA_SUCCESS : (p->err ? p->err : CLFA_INVALID_VALUE);
}

// Either form of a call of F frames on a usable object, the results in the order of the header: the op code and the
// scalar ranges (scalars_ok: the family's), F == 0 as a successful no-op, the arrays, in a blocking form the per-frame
// values (values_ok(): the family's rule on the host arrays), `ready` (the blur's setup), the object's own error; then
// launch(d, stream) with the arrays the device reads and writes: the caller's in a device form, the staged ones in a
// blocking form.
template <size_t N, class Values, class Launch>
static int pvoc_call(clfa_pvoc *p, bool blocking, void *stream, bool scalars_ok, long F, const PvocArray (&arrays)[N], int ready,
                     Values values_ok, Launch launch) {
  static_assert(N <= kCallArrays, "kCallArrays");
  int chk = !scalars_ok || !pvoc_count_ok(F) || (F > 0 && !arrays_ok(arrays, !blocking)) ? CLFA_INVALID_VALUE : F == 0;
  if (chk == 0 && blocking && !values_ok()) chk = CLFA_INVALID_VALUE;
  if (chk == 0) chk = ready;
  if (!blocking) {
    const void *d[kCallArrays] = {};
    for (size_t i = 0; i < N; i++) d[i] = arrays[i].used ? arrays[i].ptr : nullptr;
    return pvoc_dev_form(p, chk, stream, [&](hipStream_t s) { return launch(d, s); });
  }
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  return staged_call(p, arrays, [&](const void *const *d) {
    return pvoc_dev_form(p, CLFA_SUCCESS, p->stream, [&](hipStream_t s) { return launch(d, s); });
  });
}
static bool pvoc_no_values() { return true; }

// the fields every launch of a frame operation takes
static void pvoc_frames_args(const clfa_pvoc *p, long F, PvocFramesArgs &a) {
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.logn = ilog2(p->M);
  a.half = (const cpx *)p->half.p;
  a.w2 = (const cpx *)p->w2.p;
  a.grid_max = p->ops_grid_max;
}

// ---------------------------------------------------------------------------------
// spectra <-> (amp, freq) frames (pvoc_kernels.hip).  Unlike the frame operations, both directions answer with the
// object's own error before they look at an argument.
// ---------------------------------------------------------------------------------

using PvocConvert = HostArrays<clfa_pvoc, 2>;   // the spectra, the frames
static PvocConvert pvoc_convert(const clfa_pvoc *p, const void *spectra, const void *frames, long F, bool synthesis) {
  return {{{spectra, pvoc_spec_bytes(p, F), 8, synthesis, &clfa_pvoc::sspec},
           {frames, pvoc_frame_bytes(p, F), 8, !synthesis, &clfa_pvoc::sframes}}};
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
  a.prev = (cpx *)p->prev.p;
  a.etab = (const cpx *)p->etab.p;
  a.theta = (unsigned *)p->theta.p;
  a.sums = (unsigned *)p->ws.p;
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
size_t clfa_pvoc_workspace_bytes(const clfa_pvoc *p) { return p ? p->ws.bytes : 0; }
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
  return pvoc_read_state(p, {{host, &clfa_pvoc::theta, sizeof(unsigned)}});
}

int clfa_pvoc_read_prev(clfa_pvoc *p, float *host) {
  return pvoc_read_state(p, {{host, &clfa_pvoc::prev, sizeof(cpx)}});
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
    const long held = p->cap;   // the whole sub-batch workspace at the first need: its address never changes afterwards
    if (int e = ensure_workspaces({{&p->ws, sizeof(unsigned) * pvoc_bins(p) * (size_t)held}}, s)) return e;
    PvocArgs a = pvoc_args(p, F);
    a.frames_in = (const float *)frames;
    a.spec_out = (cpx *)spectra_out;
    return pvoc_subbatches(F, held, [&](long f0, long nf) { return launch_pvoc_synth(a, f0, nf, p->di, s); });
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

// ---------------------------------------------------------------------------------
// frames -> frames: pitch scale, frequency shift, timed read (pvoc_ops.hip)
// ---------------------------------------------------------------------------------

// F: output frames, Fin: input frames (== F for scale and shift).  The blocking forms ask finite values of scale and
// shift, and scales in [1/4, 4]; the read's positions are clamped, whatever they are.
static int pvoc_ops_call(clfa_pvoc *p, bool blocking, int op, const void *in, long Fin, const void *par, void *out, long F,
                         int lowest, int keepform, float gain, int coefs, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = !(op == PVOC_READ && (Fin < 1 || Fin > (1L << 24))) &&
                          !(op == PVOC_SHIFT && (lowest < 1 || lowest > p->M - 1)) &&
                          !(op != PVOC_READ && keepform && (coefs < 1 || coefs >= p->M));
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, Fin), 8, false, &clfa_pvoc::sframes},
                              {out, pvoc_frame_bytes(p, F), 8, true, &clfa_pvoc::sop_out},
                              {par, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::sop_par}};
  const auto values_ok = [&] {
    const float *v = (const float *)par;
    for (long f = 0; f < F && op != PVOC_READ; f++)
      if (!std::isfinite(v[f]) || (op == PVOC_SCALE && !(v[f] >= 0.25f && v[f] <= 4.f))) return false;
    return true;
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, values_ok, [&](const void *const *d, hipStream_t s) {
    PvocOpsArgs a;
    pvoc_frames_args(p, F, a);
    a.op = op;
    a.Fin = Fin;
    a.in = (const cpx *)d[0];
    a.out = (cpx *)d[1];
    a.par = (const float *)d[2];
    a.lowest = lowest;
    a.keepform = keepform != 0;
    a.coefs = coefs;
    a.gain = gain;
    a.cf = p->srs;
    a.bpf = p->bpf;
    return launch_pvoc_ops(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_scale_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, long F, const void *scale, int keepform,
                        float gain, int coefs, void *stream) {
  return pvoc_ops_call(p, false, PVOC_SCALE, frames_in, F, scale, frames_out, F, 1, keepform, gain, coefs, stream);
}
int clfa_pvoc_shift_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, long F, const void *shift, int lowest_bin,
                        int keepform, float gain, int coefs, void *stream) {
  return pvoc_ops_call(p, false, PVOC_SHIFT, frames_in, F, shift, frames_out, F, lowest_bin, keepform, gain, coefs, stream);
}
int clfa_pvoc_read_dev(clfa_pvoc *p, const void *frames_in, long Fin, const void *pos, void *frames_out, long Fout,
                       void *stream) {
  return pvoc_ops_call(p, false, PVOC_READ, frames_in, Fin, pos, frames_out, Fout, 1, 0, 1.f, 1, stream);
}
int clfa_pvoc_scale(clfa_pvoc *p, const float *frames_in, float *frames_out, long F, const float *scale, int keepform,
                    float gain, int coefs) {
  return pvoc_ops_call(p, true, PVOC_SCALE, frames_in, F, scale, frames_out, F, 1, keepform, gain, coefs, nullptr);
}
int clfa_pvoc_shift(clfa_pvoc *p, const float *frames_in, float *frames_out, long F, const float *shift, int lowest_bin,
                    int keepform, float gain, int coefs) {
  return pvoc_ops_call(p, true, PVOC_SHIFT, frames_in, F, shift, frames_out, F, lowest_bin, keepform, gain, coefs, nullptr);
}
int clfa_pvoc_read(clfa_pvoc *p, const float *frames_in, long Fin, const float *pos, float *frames_out, long Fout) {
  return pvoc_ops_call(p, true, PVOC_READ, frames_in, Fin, pos, frames_out, Fout, 1, 0, 1.f, 1, nullptr);
}
const char *clfa_pvoc_ops_kernel_name(const clfa_pvoc *p, int op, int keepform) {
  if (!p || p->err || op < PVOC_SCALE || op > PVOC_READ) return "";
  return op == PVOC_READ ? "k_pvoc_read" : (keepform ? "k_pvoc_formant" : "k_pvoc_map");
}

}  // extern "C"

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
  const PvocArray arrays[] = {{signal, row, 4, false, &clfa_pvoc::ssig, true, (size_t)p->channels, pitch},
                              {out, pvoc_frame_bytes(p, Fout), 8, true, &clfa_pvoc::sop_out},
                              {window, sizeof(float) * (size_t)p->size, 4, false, &clfa_pvoc::sshape_tab},
                              {starts, sizeof(int) * (size_t)Fout, 4, false, &clfa_pvoc::sdelay_tab}};
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
// two streams of frames -> frames: cross, morph, filter, mix, vocode (pvoc_pair.hip)
// ---------------------------------------------------------------------------------

// MIX reads neither per-frame array.  The blocking form asks finite values, and the depths and weights in [0, 1].
static int pvoc_pair_call(clfa_pvoc *p, bool blocking, int op, const void *a, const void *b, void *out, long F,
                          const void *pp, const void *qq, int coefs, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = op >= PVOC_CROSS && op <= PVOC_VOCODE && !(op == PVOC_VOCODE && (coefs < 1 || coefs >= p->M));
  const bool mix = op == PVOC_MIX;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  const PvocArray arrays[] = {{a, fbytes, 8, false, &clfa_pvoc::sframes},    {b, fbytes, 8, false, &clfa_pvoc::spair_b},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},   {pp, pbytes, 4, false, &clfa_pvoc::sop_par, !mix},
                              {qq, pbytes, 4, false, &clfa_pvoc::spair_q, !mix}};
  const auto values_ok = [&] {
    const float *P = (const float *)pp, *Q = (const float *)qq;
    const bool unit_p = op == PVOC_MORPH || op == PVOC_FILTER || op == PVOC_VOCODE, unit_q = op == PVOC_MORPH;
    for (long f = 0; f < F && !mix; f++) {
      if (!std::isfinite(P[f]) || !std::isfinite(Q[f])) return false;
      if ((unit_p && !(P[f] >= 0.f && P[f] <= 1.f)) || (unit_q && !(Q[f] >= 0.f && Q[f] <= 1.f))) return false;
    }
    return true;
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, values_ok, [&](const void *const *d, hipStream_t s) {
    PvocPairArgs g;
    pvoc_frames_args(p, F, g);
    g.op = op;
    g.a = (const cpx *)d[0];
    g.b = (const cpx *)d[1];
    g.out = (cpx *)d[2];
    g.p = (const float *)d[3];
    g.q = (const float *)d[4];
    g.coefs = coefs;
    return launch_pvoc_pair(g, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_pair_dev(clfa_pvoc *p, int op, const void *frames_a, const void *frames_b, void *frames_out, long F,
                       const void *pp, const void *qq, int coefs, void *stream) {
  return pvoc_pair_call(p, false, op, frames_a, frames_b, frames_out, F, pp, qq, coefs, stream);
}
int clfa_pvoc_pair(clfa_pvoc *p, int op, const float *frames_a, const float *frames_b, float *frames_out, long F,
                   const float *pp, const float *qq, int coefs) {
  return pvoc_pair_call(p, true, op, frames_a, frames_b, frames_out, F, pp, qq, coefs, nullptr);
}
const char *clfa_pvoc_pair_kernel_name(const clfa_pvoc *p, int op) {
  if (!p || p->err || op < PVOC_CROSS || op > PVOC_VOCODE) return "";
  return op == PVOC_VOCODE ? "k_pvoc_vocode" : "k_pvoc_pair";
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// one stream of frames -> frames, along the bins: band, mask, stencil, arp, lock, warp (pvoc_shape.hip)
// ---------------------------------------------------------------------------------

// the values of one row the blocking form accepts: those the op names finite, and the op's ranges
static bool pvoc_shape_row_ok(int op, const float *r) {
  static const int cols[] = {4, 1, 2, 3, 2, 3};
  for (int i = 0; i < cols[op]; i++)
    if (!std::isfinite(r[i])) return false;
  const auto unit = [](float x) { return x >= 0.f && x <= 1.f; };
  switch (op) {
    case PVOC_BAND: return 0.f <= r[0] && r[0] <= r[1] && r[1] <= r[2] && r[2] <= r[3];
    case PVOC_MASK: return unit(r[0]);
    case PVOC_ARP: return unit(r[0]) && unit(r[1]);
    case PVOC_LOCK: return r[1] >= 0.f;
    case PVOC_WARP: return r[0] >= 0.25f && r[0] <= 4.f;
    default: return true;   // STENCIL: gain and level are free
  }
}

// The table is looked at for MASK and STENCIL only; flags: bit 0, for BAND alone; lowest and coefs: WARP's.
static int pvoc_shape_call(clfa_pvoc *p, bool blocking, int op, const void *in, void *out, long F, const void *par,
                           const void *table, int flags, int lowest, int coefs, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = op >= PVOC_BAND && op <= PVOC_WARP && !(flags & ~(op == PVOC_BAND ? 1 : 0)) &&
                          !(op == PVOC_WARP && (lowest < 1 || lowest > p->M - 1 || coefs < 1 || coefs >= p->M));
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::sframes},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},
                              {par, 4 * sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::sop_par},
                              {table, sizeof(float) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::sshape_tab,
                               op == PVOC_MASK || op == PVOC_STENCIL}};
  const auto values_ok = [&] {
    for (long f = 0; f < F; f++)
      if (!pvoc_shape_row_ok(op, (const float *)par + 4 * f)) return false;
    return true;
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, values_ok, [&](const void *const *d, hipStream_t s) {
    PvocShapeArgs a;
    pvoc_frames_args(p, F, a);
    a.op = op;
    a.in = (const cpx *)d[0];
    a.out = (cpx *)d[1];
    a.par = (const float *)d[2];
    a.table = (const float *)d[3];
    a.reject = flags & 1;
    a.lowest = lowest;
    a.coefs = coefs;
    a.bpf = p->bpf;
    return launch_pvoc_shape(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_shape_dev(clfa_pvoc *p, int op, const void *frames_in, void *frames_out, long F, const void *par,
                        const void *table, int flags, int lowest_bin, int coefs, void *stream) {
  return pvoc_shape_call(p, false, op, frames_in, frames_out, F, par, table, flags, lowest_bin, coefs, stream);
}
int clfa_pvoc_shape(clfa_pvoc *p, int op, const float *frames_in, float *frames_out, long F, const float *par,
                    const float *table, int flags, int lowest_bin, int coefs) {
  return pvoc_shape_call(p, true, op, frames_in, frames_out, F, par, table, flags, lowest_bin, coefs, nullptr);
}
const char *clfa_pvoc_shape_kernel_name(const clfa_pvoc *p, int op) {
  if (!p || p->err || op < PVOC_BAND || op > PVOC_WARP) return "";
  return op == PVOC_WARP ? "k_pvoc_warp" : (op == PVOC_LOCK ? "k_pvoc_lock" : "k_pvoc_shape");
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> frames along the stream, with carried state: blur, smooth, freeze (pvoc_time.hip)
// ---------------------------------------------------------------------------------

// whether the blur has been set up: asked after the arguments (and, in the blocking form, after the per-frame values)
static int pvoc_time_ready(const clfa_pvoc *p, int op) {
  return op == PVOC_BLUR && !p->blur_max ? CLFA_INVALID_OPERATION : CLFA_SUCCESS;
}

static DevBuf clfa_pvoc::*pvoc_time_state(int op) {
  return op == PVOC_BLUR ? &clfa_pvoc::bhist : (op == PVOC_SMOOTH ? &clfa_pvoc::tsmooth : &clfa_pvoc::theld);
}

// BLUR does not look at q.  The blocking form asks finite values, the blur's lengths in 1..max_frames (where it is set
// up) and the smoothing's weights in [0, 1].
static int pvoc_time_call(clfa_pvoc *p, bool blocking, int op, const void *in, void *out, long F, const void *pp,
                          const void *qq, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = op >= PVOC_BLUR && op <= PVOC_FREEZE;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::sframes},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},
                              {pp, pbytes, 4, false, &clfa_pvoc::sop_par},
                              {qq, pbytes, 4, false, &clfa_pvoc::spair_q, op != PVOC_BLUR}};
  const auto values_ok = [&] {
    const float *P = (const float *)pp, *Q = (const float *)qq;
    for (long f = 0; f < F; f++) {
      if (!std::isfinite(P[f]) || (op != PVOC_BLUR && !std::isfinite(Q[f]))) return false;
      if (op == PVOC_BLUR && (!(P[f] >= 1.f) || (p->blur_max && !(P[f] <= (float)p->blur_max)))) return false;
      if (op == PVOC_SMOOTH && !(P[f] >= 0.f && P[f] <= 1.f && Q[f] >= 0.f && Q[f] <= 1.f)) return false;
    }
    return true;
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, pvoc_time_ready(p, op), values_ok,
                   [&](const void *const *d, hipStream_t s) {
                     PvocTimeArgs a;
                     pvoc_frames_args(p, F, a);
                     a.op = op;
                     a.in = (const cpx *)d[0];
                     a.out = (cpx *)d[1];
                     a.p = (const float *)d[2];
                     a.q = (const float *)d[3];
                     a.state = (cpx *)(p->*pvoc_time_state(op)).p;
                     a.spare = (cpx *)p->bspare.p;
                     a.max_frames = p->blur_max;
                     return launch_pvoc_time(a, p->di, s);
                   });
}

extern "C" {

int clfa_pvoc_blur_setup(clfa_pvoc *p, int max_frames) {
  if (int e = pvoc_usable(p)) return e;
  if (max_frames < 1 || max_frames > 4096) return CLFA_INVALID_VALUE;
  if (p->err) return p->err;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  // both buffers first, so that a failed allocation leaves the object as it was
  const size_t bytes = pvoc_frame_bytes(p, max_frames - 1);
  DevBuf hist, spare;
  if (int e = hist.ensure(bytes)) return e;
  if (int e = spare.ensure(bytes)) return e;
  HIP_TRY(launch_pvoc_time_fill((cpx *)hist.p, (long)p->channels * (max_frames - 1), p->M, p->srs, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  std::swap(p->bhist.p, hist.p);
  std::swap(p->bhist.bytes, hist.bytes);
  std::swap(p->bspare.p, spare.p);
  std::swap(p->bspare.bytes, spare.bytes);
  p->blur_max = max_frames;
  return CLFA_SUCCESS;
}

int clfa_pvoc_time_dev(clfa_pvoc *p, int op, const void *frames_in, void *frames_out, long F, const void *pp,
                       const void *qq, void *stream) {
  return pvoc_time_call(p, false, op, frames_in, frames_out, F, pp, qq, stream);
}
int clfa_pvoc_time(clfa_pvoc *p, int op, const float *frames_in, float *frames_out, long F, const float *pp,
                   const float *qq) {
  return pvoc_time_call(p, true, op, frames_in, frames_out, F, pp, qq, nullptr);
}

int clfa_pvoc_time_read_state(clfa_pvoc *p, int op, float *host) {
  if (!p || op < PVOC_BLUR || op > PVOC_FREEZE || !host) return CLFA_INVALID_VALUE;
  if (int e = obj_error(p)) return e;
  if (int e = pvoc_time_ready(p, op)) return e;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  const size_t bytes = pvoc_frame_bytes(p, op == PVOC_BLUR ? p->blur_max - 1 : 1);
  if (bytes) HIP_TRY(hipMemcpy(host, (p->*pvoc_time_state(op)).p, bytes, hipMemcpyDeviceToHost));
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_time_state_bytes(const clfa_pvoc *p) {
  return p ? p->tsmooth.bytes + p->theld.bytes + p->bhist.bytes + p->bspare.bytes : 0;
}
int clfa_pvoc_blur_max_frames(const clfa_pvoc *p) { return p ? p->blur_max : 0; }
const char *clfa_pvoc_time_kernel_name(const clfa_pvoc *p, int op) {
  if (!p || p->err || op < PVOC_BLUR || op > PVOC_FREEZE) return "";
  return op == PVOC_BLUR ? "k_pvoc_blur" : (op == PVOC_SMOOTH ? "k_pvoc_smooth" : "k_pvoc_freeze");
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> frames along the stream: the per-bin delay with feedback, with carried state (pvoc_delay.hip)
// ---------------------------------------------------------------------------------

constexpr int kPvocDelayMax = 4096;   // the largest max_delay of clfa_pvoc_delay_setup

// whether the delay has been set up: asked after the arguments (and, in the blocking form, after the tables' values)
static int pvoc_delay_ready(const clfa_pvoc *p) { return p->delay_max < 0 ? CLFA_INVALID_OPERATION : CLFA_SUCCESS; }

// A NULL feedback is none.  The blocking form asks delays in 0..max_delay (before the setup: 0..4096, what a setup can make
// valid) and finite feedbacks in [-1, 1]; the device form clamps the delays and takes the feedbacks as they are.
static int pvoc_delay_call(clfa_pvoc *p, bool blocking, const void *in, void *out, long F, const void *delays,
                           const void *feedback, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::sframes},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},
                              {delays, sizeof(int) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::sdelay_tab},
                              {feedback, sizeof(float) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::sshape_tab, feedback != nullptr}};
  const auto values_ok = [&] {
    const int *d = (const int *)delays;
    const float *g = (const float *)feedback;
    for (int k = 0; k <= p->M; k++) {
      if (d[k] < 0 || d[k] > (p->delay_max >= 0 ? p->delay_max : kPvocDelayMax)) return false;
      if (g && !(std::isfinite(g[k]) && g[k] >= -1.f && g[k] <= 1.f)) return false;
    }
    return true;
  };
  return pvoc_call(p, blocking, stream, true, F, arrays, pvoc_delay_ready(p), values_ok, [&](const void *const *d, hipStream_t s) {
    PvocDelayArgs a;
    pvoc_frames_args(p, F, a);
    a.in = (const cpx *)d[0];
    a.out = (cpx *)d[1];
    a.delays = (const int *)d[2];
    a.feedback = (const float *)d[3];
    a.xhist = (cpx *)p->dxhist.p;
    a.yhist = (cpx *)p->dyhist.p;
    a.spare = (cpx *)p->dspare.p;
    a.L = p->delay_max;
    return launch_pvoc_delay(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_delay_setup(clfa_pvoc *p, int max_delay) {
  if (int e = pvoc_usable(p)) return e;
  if (max_delay < 0 || max_delay > kPvocDelayMax) return CLFA_INVALID_VALUE;
  if (p->err) return p->err;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  // the three buffers first, so that a failed allocation leaves the object as it was
  const size_t bytes = pvoc_frame_bytes(p, max_delay);
  DevBuf bufs[3];
  DevBuf clfa_pvoc::*const mine[3] = {&clfa_pvoc::dxhist, &clfa_pvoc::dyhist, &clfa_pvoc::dspare};
  for (DevBuf &b : bufs)
    if (int e = b.ensure(bytes)) return e;
  for (int i = 0; i < 2; i++) HIP_TRY(launch_pvoc_time_fill((cpx *)bufs[i].p, (long)p->channels * max_delay, p->M, p->srs, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (int i = 0; i < 3; i++) {
    std::swap((p->*mine[i]).p, bufs[i].p);
    std::swap((p->*mine[i]).bytes, bufs[i].bytes);
  }
  p->delay_max = max_delay;
  return CLFA_SUCCESS;
}

int clfa_pvoc_delay_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, long F, const void *delays,
                        const void *feedback, void *stream) {
  return pvoc_delay_call(p, false, frames_in, frames_out, F, delays, feedback, stream);
}
int clfa_pvoc_delay(clfa_pvoc *p, const float *frames_in, float *frames_out, long F, const int *delays, const float *feedback) {
  return pvoc_delay_call(p, true, frames_in, frames_out, F, delays, feedback, nullptr);
}

int clfa_pvoc_delay_read_state(clfa_pvoc *p, int which, float *host) {
  if (!p || which < 0 || which > 1 || !host) return CLFA_INVALID_VALUE;
  if (int e = obj_error(p)) return e;
  if (int e = pvoc_delay_ready(p)) return e;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  const size_t bytes = pvoc_frame_bytes(p, p->delay_max);
  if (bytes) HIP_TRY(hipMemcpy(host, (which ? p->dyhist : p->dxhist).p, bytes, hipMemcpyDeviceToHost));
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_delay_state_bytes(const clfa_pvoc *p) { return p ? p->dxhist.bytes + p->dyhist.bytes + p->dspare.bytes : 0; }
int clfa_pvoc_delay_max_frames(const clfa_pvoc *p) { return p ? p->delay_max : -1; }
const char *clfa_pvoc_delay_kernel_name(const clfa_pvoc *p, int feedback) {
  return !p || p->err ? "" : (feedback ? "k_pvoc_delay_fb" : "k_pvoc_delay");
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> eight descriptors per frame, with carried state (pvoc_desc.hip)
// ---------------------------------------------------------------------------------

static int pvoc_desc_call(clfa_pvoc *p, bool blocking, const void *in, void *desc, long F, int first_bin, int nbins,
                          int rectify, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M && (rectify == 0 || rectify == 1);
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::sframes},
                              {desc, 8 * sizeof(float) * (size_t)p->channels * (size_t)F, 4, true, &clfa_pvoc::sdesc}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    PvocDescArgs a;
    pvoc_frames_args(p, F, a);
    a.in = (const cpx *)d[0];
    a.desc = (float *)d[1];
    a.last = (cpx *)p->dlast.p;
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

// the amps of the previous frame: the first of every pair the device holds
int clfa_pvoc_desc_read_state(clfa_pvoc *p, float *host) {
  if (int e = obj_error(p)) return e;
  if (!host) return CLFA_INVALID_VALUE;
  std::vector<cpx> pairs(pvoc_bins(p));
  if (int e = pvoc_read_state(p, {{pairs.data(), &clfa_pvoc::dlast, sizeof(cpx)}})) return e;
  for (size_t i = 0; i < pairs.size(); i++) host[i] = pairs[i].x;
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_desc_state_bytes(const clfa_pvoc *p) { return p ? p->dlast.bytes : 0; }
const char *clfa_pvoc_desc_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_desc"; }

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> band energies, their log, a DCT of that (bank_kernels.hip)
// ---------------------------------------------------------------------------------

// whether the bank has been set up: asked after the arguments
static int pvoc_bank_ready(const clfa_pvoc *p) { return p->bank_B < 0 ? CLFA_INVALID_OPERATION : CLFA_SUCCESS; }

// floor is looked at with LOG only; ncoef is 1..B with DCT (before the setup: 1..256, what a setup can make valid), else 0.
// The output rows hold ncoef values with DCT, else B (before the setup the check takes rows of one value).
static int pvoc_bands_call(clfa_pvoc *p, bool blocking, const void *in, void *out, long F, int flags, int ncoef, float floor,
                           void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const int all = CLFA_PVOC_BANDS_POWER | CLFA_PVOC_BANDS_LOG | CLFA_PVOC_BANDS_DCT;
  const bool lg = flags & CLFA_PVOC_BANDS_LOG, dct = flags & CLFA_PVOC_BANDS_DCT;
  const int B = p->bank_B;
  const bool scalars_ok = !(flags & ~all) && (!lg || (std::isfinite(floor) && floor > 0.f)) &&
                          (dct ? ncoef >= 1 && ncoef <= (B >= 0 ? B : kBankMax) : ncoef == 0);
  const size_t N = dct ? (size_t)(ncoef > 0 ? ncoef : 0) : (size_t)(B > 0 ? B : 1);
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::sframes},
                              {out, sizeof(float) * (size_t)p->channels * (size_t)F * N, 4, true, &clfa_pvoc::sbands}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    BankArgs a;
    a.M = p->M;
    a.channels = p->channels;
    a.F = F;
    a.in = (const cpx *)d[0];
    a.out = (float *)d[1];
    a.B = B;
    a.steps = p->bank_steps;
    a.bands = (const int *)p->kbands.p;
    a.sched = (const int *)p->ksched.p;
    a.weights = (const float *)p->kweights.p;
    a.dct_t = (const float *)p->kdct.p;
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
  if (int e = pvoc_usable(p)) return e;
  if (!bank_ok(p->M, nbands, first, count, weights)) return CLFA_INVALID_VALUE;
  if (p->err) return p->err;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  const std::vector<BankBand> bands = bank_bands(nbands, first, count);
  const std::vector<int> sched = bank_schedule(nbands, count);
  const std::vector<float> D = bank_dct(nbands);
  std::vector<float> Dt(D.size());   // the kernel's lanes of neighbouring q read neighbouring words
  for (int q = 0; q < nbands; q++)
    for (int b = 0; b < nbands; b++) Dt[(size_t)b * nbands + q] = D[(size_t)q * nbands + b];
  const size_t nweights = (size_t)bands.back().woff + bands.back().count;
  int steps = 0;
  for (int r = 0; r < kBankRows; r++) steps = std::max(steps, sched[r + 1] - sched[r]);
  // every buffer first, so that a failed allocation leaves the object as it was
  DevBuf bufs[4];
  DevBuf clfa_pvoc::*const mine[4] = {&clfa_pvoc::kbands, &clfa_pvoc::ksched, &clfa_pvoc::kweights, &clfa_pvoc::kdct};
  const void *src[4] = {bands.data(), sched.data(), weights, Dt.data()};
  const size_t bytes[4] = {sizeof(BankBand) * bands.size(), sizeof(int) * sched.size(), sizeof(float) * nweights,
                           sizeof(float) * Dt.size()};
  for (int i = 0; i < 4; i++)
    if (int e = upload(bufs[i], src[i], bytes[i])) return e;
  for (int i = 0; i < 4; i++) {
    std::swap((p->*mine[i]).p, bufs[i].p);
    std::swap((p->*mine[i]).bytes, bufs[i].bytes);
  }
  p->bank_B = nbands;
  p->bank_steps = steps;
  return CLFA_SUCCESS;
}

int clfa_pvoc_bank_bands(const clfa_pvoc *p) { return p ? p->bank_B : -1; }

// the table the device uses, D[q][b]: the device keeps it transposed
int clfa_pvoc_bank_read_dct(clfa_pvoc *p, float *host) {
  if (!p || !host) return CLFA_INVALID_VALUE;
  if (int e = obj_error(p)) return e;
  if (int e = pvoc_bank_ready(p)) return e;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  const int B = p->bank_B;
  std::vector<float> Dt((size_t)B * B);
  HIP_TRY(hipMemcpy(Dt.data(), p->kdct.p, sizeof(float) * Dt.size(), hipMemcpyDeviceToHost));
  for (int q = 0; q < B; q++)
    for (int b = 0; b < B; b++) host[(size_t)q * B + b] = Dt[(size_t)b * B + q];
  return CLFA_SUCCESS;
}

size_t clfa_pvoc_bank_state_bytes(const clfa_pvoc *p) {
  return p ? p->kbands.bytes + p->ksched.bytes + p->kweights.bytes + p->kdct.bytes : 0;
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
// frames -> frames: the N loudest bins of every frame, or all but those, and the list of the bins (pvoc_trace.hip)
// ---------------------------------------------------------------------------------

// The one call with two outputs: the frames, and the bin list where `bins` is given (list_n is looked at only then).
// Every n has a meaning (a NaN or a negative keeps nothing), so the blocking form has no values to refuse.
static int pvoc_trace_call(clfa_pvoc *p, bool blocking, const void *in, void *out, const void *n, void *bins, int list_n,
                           long F, int first_bin, int nbins, int flags, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M &&
                          !(flags & ~CLFA_PVOC_TRACE_RESIDUAL) && !(bins && list_n < 1);
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const size_t lbytes = bins && list_n >= 1 ? sizeof(int) * (size_t)p->channels * (size_t)(F > 0 ? F : 0) * (size_t)list_n : 0;
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::sframes},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},
                              {n, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::sop_par},
                              {bins, lbytes, 4, true, &clfa_pvoc::strace_bins, bins != nullptr}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    PvocTraceArgs a;
    pvoc_frames_args(p, F, a);
    a.in = (const cpx *)d[0];
    a.out = (cpx *)d[1];
    a.n = (const float *)d[2];
    a.bins = (int *)d[3];
    a.list_n = list_n;
    a.lo = first_bin;
    a.hi = first_bin + nbins - 1;
    a.residual = flags & CLFA_PVOC_TRACE_RESIDUAL;
    return launch_pvoc_trace(a, p->di, s);
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, pvoc_no_values, launch);
}

extern "C" {

int clfa_pvoc_trace_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, const void *n, void *bins, int list_n, long F,
                        int first_bin, int nbins, int flags, void *stream) {
  return pvoc_trace_call(p, false, frames_in, frames_out, n, bins, list_n, F, first_bin, nbins, flags, stream);
}

int clfa_pvoc_trace(clfa_pvoc *p, const float *frames_in, float *frames_out, const float *n, int *bins, int list_n, long F,
                    int first_bin, int nbins, int flags) {
  return pvoc_trace_call(p, true, frames_in, frames_out, n, bins, list_n, F, first_bin, nbins, flags, nullptr);
}

const char *clfa_pvoc_trace_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_pvoc_trace"; }

}  // extern "C"

// ---------------------------------------------------------------------------------
// the left and the right frames of one recording -> frames, by azimuth, and the azimuth profile (pvoc_demix.hip)
// ---------------------------------------------------------------------------------

// The second call with two outputs: the frames, and the profile where `az` is given.  par: F rows of (pos, width).  The
// blocking form asks finite values, pos in [-1, 1] and width in [1, 2 points + 1]; the device form clamps.
static int pvoc_demix_call(clfa_pvoc *p, bool blocking, const void *l, const void *r, void *out, const void *par, void *az,
                           long F, int points, int first_bin, int nbins, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = points >= 1 && points <= 1024 && first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M;
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const size_t abytes = az && scalars_ok ? sizeof(float) * (size_t)p->channels * (size_t)(F > 0 ? F : 0) * (size_t)(2 * points + 1) : 0;
  const PvocArray arrays[] = {{l, fbytes, 8, false, &clfa_pvoc::sframes},
                              {r, fbytes, 8, false, &clfa_pvoc::spair_b},
                              {out, fbytes, 8, true, &clfa_pvoc::sop_out},
                              {par, 2 * sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::sop_par},
                              {az, abytes, 4, true, &clfa_pvoc::sdemix_az, az != nullptr}};
  const auto values_ok = [&] {
    const float *v = (const float *)par;
    for (long f = 0; f < F; f++) {
      const float pos = v[2 * f], width = v[2 * f + 1];
      if (!std::isfinite(pos) || !std::isfinite(width)) return false;
      if (!(pos >= -1.f && pos <= 1.f && width >= 1.f && width <= (float)(2 * points + 1))) return false;
    }
    return true;
  };
  return pvoc_call(p, blocking, stream, scalars_ok, F, arrays, CLFA_SUCCESS, values_ok, [&](const void *const *d, hipStream_t s) {
    PvocDemixArgs a;
    pvoc_frames_args(p, F, a);
    a.l = (const cpx *)d[0];
    a.r = (const cpx *)d[1];
    a.out = (cpx *)d[2];
    a.par = (const float *)d[3];
    a.az = (float *)d[4];
    a.points = points;
    a.lo = first_bin;
    a.hi = first_bin + nbins - 1;
    return launch_pvoc_demix(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_demix_dev(clfa_pvoc *p, const void *frames_l, const void *frames_r, void *frames_out, const void *par, void *az,
                        long F, int points, int first_bin, int nbins, void *stream) {
  return pvoc_demix_call(p, false, frames_l, frames_r, frames_out, par, az, F, points, first_bin, nbins, stream);
}

int clfa_pvoc_demix(clfa_pvoc *p, const float *frames_l, const float *frames_r, float *frames_out, const float *par, float *az,
                    long F, int points, int first_bin, int nbins) {
  return pvoc_demix_call(p, true, frames_l, frames_r, frames_out, par, az, F, points, first_bin, nbins, nullptr);
}

const char *clfa_pvoc_demix_kernel_name(const clfa_pvoc *p, int with_az) {
  return !p || p->err ? "" : (with_az ? "k_pvoc_demix_az" : "k_pvoc_demix");
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> four values per frame: the pitch from the frame's spectral peaks, and the peak list (pitch_kernels.hip)
// ---------------------------------------------------------------------------------

// The third call with two outputs: the rows, and the list where `peaks` is given.  All its parameters are scalars, so the
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
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::sframes},
                              {rows, 4 * sizeof(float) * frames, 4, true, &clfa_pvoc::spitch_rows},
                              {peaks, pbytes, 8, true, &clfa_pvoc::spitch_peaks, peaks != nullptr}};
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

// ---------------------------------------------------------------------------------
// frames -> samples: the oscillator bank (pvoc_adsyn.hip)
// ---------------------------------------------------------------------------------

static size_t pvoc_adsyn_ws_bytes(const clfa_pvoc *p) {
  return sizeof(unsigned long long) * pvoc_bins(p) * (size_t)p->acap + (sizeof(int) + sizeof(float)) * pvoc_bins(p);
}

// signal: channels rows of F hop floats, signal_stride floats apart at the caller's (the overlap rule takes the rows and
// the gaps between them as one span), packed where the blocking form stages them.  A NULL fmod is none.
static int pvoc_adsyn_call(clfa_pvoc *p, bool blocking, const void *frames, long F, const void *fmod, int first_bin, int nbins,
                           int step, float gain, void *signal, long signal_stride, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = step >= 1 && nbins >= 1 && first_bin >= 0 && (long)first_bin + ((long)nbins - 1) * step <= p->M &&
                          pvoc_count_ok(F) && signal_stride >= F * p->hop;
  const size_t row = sizeof(float) * (size_t)F * p->hop, pitch = sizeof(float) * (size_t)signal_stride;
  const PvocArray arrays[] = {{frames, pvoc_frame_bytes(p, F), 8, false, &clfa_pvoc::sframes},
                              {signal, row, 4, true, &clfa_pvoc::ssig, true, (size_t)p->channels, pitch},
                              {fmod, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::sfmod, fmod != nullptr}};
  const auto launch = [&](const void *const *d, hipStream_t s) {
    const long held = p->acap;   // the whole workspace at the first need: its address never changes afterwards
    if (int e = ensure_workspaces({{&p->aws, pvoc_adsyn_ws_bytes(p)}}, s)) return e;
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
    a.ks = p->ks;
    a.phase = (unsigned long long *)p->aphase.p;
    a.w = (int *)p->aw.p;
    a.amp = (float *)p->aamp.p;
    a.sums = (unsigned long long *)p->aws.p;
    a.w0 = (int *)(a.sums + pvoc_bins(p) * (size_t)held);
    a.a0 = (float *)(a.w0 + pvoc_bins(p));
    a.ramp = (const float *)p->ramp.p;
    a.signal = (float *)d[1];
    a.sstride = blocking ? F * p->hop : signal_stride;
    a.grid_max = p->adsyn_grid_max;
    return pvoc_subbatches(F, held, [&](long f0, long nf) { return launch_pvoc_adsyn(a, f0, nf, p->di, s); });
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
  return pvoc_read_state(p, {{phase, &clfa_pvoc::aphase, sizeof(unsigned long long)},
                             {w, &clfa_pvoc::aw, sizeof(int)},
                             {amp, &clfa_pvoc::aamp, sizeof(float)}});
}

size_t clfa_pvoc_adsyn_workspace_bytes(const clfa_pvoc *p) { return p ? p->aws.bytes : 0; }
int clfa_pvoc_adsyn_tile_bins(void) { return kAdsynTile; }
const char *clfa_pvoc_adsyn_kernel_name(const clfa_pvoc *p) { return !p || p->err ? "" : "k_adsyn_osc"; }

}  // extern "C"
