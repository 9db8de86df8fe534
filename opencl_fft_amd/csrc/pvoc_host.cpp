// pvoc_host.cpp — C ABI of the phase vocoder on the Stft spectra (see include/clfft_amd.h): Pvoc.  Shared plumbing: host.hpp.
#include "host.hpp"

using namespace clfa;

// ---------------------------------------------------------------------------------
// spectra <-> (amp, freq) frames (pvoc_kernels.hip)
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
  // the descriptors (pvoc_desc.hip): the stream's previous frame, channels x (M + 1) pairs of which the amps are the
  // state `last`; staging of the host form's rows
  DevBuf dlast, sdesc;
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
// y, the freeze's held, the blur's history and the descriptors' previous frame (on p->stream, blocking)
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

// The blocking host forms: every array has a staging buffer on the device, ensured in the order of the list; the inputs
// are copied in, dev() runs the device form on the staging buffers and the object's stream, the outputs are copied out,
// and the stream is waited for.  An array is `rows` rows of `bytes` each, packed in the staging buffer and `pitch` bytes
// apart on the host (0: packed there too, one plain copy); an input whose host pointer is NULL is left out.
struct PvocStaged {
  bool out;
  const void *host;
  DevBuf *buf;
  size_t bytes, rows = 1, pitch = 0;
};
template <class Dev>
static int pvoc_staged(clfa_pvoc *p, std::initializer_list<PvocStaged> arrays, Dev dev) {
  ENTER_DEVICE(p->di.device);
  for (const PvocStaged &a : arrays)
    if (int e = a.host ? a.buf->ensure(a.bytes * a.rows) : 0) return e;
  for (const PvocStaged &a : arrays)
    if (!a.out && a.host) HIP_TRY(hipMemcpyAsync(a.buf->p, a.host, a.bytes * a.rows, hipMemcpyHostToDevice, p->stream));
  if (int e = dev()) return e;
  for (const PvocStaged &a : arrays) {
    void *host = const_cast<void *>(a.host);
    if (a.out && a.pitch)
      HIP_TRY(hipMemcpy2DAsync(host, a.pitch, a.buf->p, a.bytes, a.bytes, a.rows, hipMemcpyDeviceToHost, p->stream));
    else if (a.out)
      HIP_TRY(hipMemcpyAsync(host, a.buf->p, a.bytes * a.rows, hipMemcpyDeviceToHost, p->stream));
  }
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

// The results of the argument checks: 0 = go on, 1 = a successful no-op, < 0 = the error.  An operation or the oscillator
// bank goes on after its device-free checks with the error, else the object's own error, else chk:
//   if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
static int pvoc_gate(const clfa_pvoc *p, int chk) { return chk < 0 ? chk : (p->err ? p->err : chk); }
static int pvoc_done(int e) { return e == 1 ? CLFA_SUCCESS : e; }

// the argument rules both directions share; 1 = a successful no-op
static int pvoc_check(const clfa_pvoc *p, const void *spectra, const void *frames, long F) {
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!spectra || !frames || ((uintptr_t)spectra & 7) || ((uintptr_t)frames & 7)) return CLFA_INVALID_VALUE;
  if (spans_overlap(spectra, pvoc_spec_bytes(p, F), frames, pvoc_frame_bytes(p, F))) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
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
  if (int e = pvoc_check(p, spectra, frames_out, F)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocArgs a = pvoc_args(p, F);
  a.spec_in = (const cpx *)spectra;
  a.frames_out = (float *)frames_out;
  HIP_TRY(launch_pvoc_analyze(a, p->di, s));
  return CLFA_SUCCESS;
}

int clfa_pvoc_synthesize_dev(clfa_pvoc *p, const void *frames, void *spectra_out, long F, void *stream) {
  if (int e = obj_error(p)) return e;
  if (int e = pvoc_check(p, spectra_out, frames, F)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  const long held = p->cap;   // the whole sub-batch workspace at the first need: its address never changes afterwards
  HIP_TRY(p->order.use(s));
  if (int e = ensure_workspaces({{&p->ws, sizeof(unsigned) * pvoc_bins(p) * (size_t)held}}, s)) return e;
  PvocArgs a = pvoc_args(p, F);
  a.frames_in = (const float *)frames;
  a.spec_out = (cpx *)spectra_out;
  return pvoc_subbatches(F, held, [&](long f0, long nf) { return launch_pvoc_synth(a, f0, nf, p->di, s); });
}

// ---------------------------------------------------------------------------------
// frames -> frames: pitch scale, frequency shift, timed read (pvoc_ops.hip)
// ---------------------------------------------------------------------------------

// The checks that need no device, in the order of the header: they come before the object's own error, so that on an
// object whose creation found no device a bad argument is still an invalid value (M != 0: the creation arguments were
// good).  0 = go on, 1 = a successful no-op, < 0 = the error.  F: output frames, Fin: input frames (== F for scale and shift).
static int pvoc_ops_check(const clfa_pvoc *p, int op, const void *in, long Fin, const void *par, const void *out, long F,
                          int lowest, int keepform, int coefs, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (op == PVOC_READ && (Fin < 1 || Fin > (1L << 24))) return CLFA_INVALID_VALUE;
  if (op == PVOC_SHIFT && (lowest < 1 || lowest > p->M - 1)) return CLFA_INVALID_VALUE;
  if (op != PVOC_READ && keepform && (coefs < 1 || coefs >= p->M)) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!in || !out || !par) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)in & 7) || ((uintptr_t)out & 7) || ((uintptr_t)par & 3))) return CLFA_INVALID_VALUE;
  const size_t ibytes = pvoc_frame_bytes(p, Fin), obytes = pvoc_frame_bytes(p, F);
  if (spans_overlap(in, ibytes, out, obytes) || spans_overlap(par, sizeof(float) * (size_t)F, out, obytes))
    return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

static int pvoc_ops_dev(clfa_pvoc *p, int op, const void *in, long Fin, const void *par, void *out, long F, int lowest,
                        int keepform, float gain, int coefs, void *stream) {
  if (int e = pvoc_gate(p, pvoc_ops_check(p, op, in, Fin, par, out, F, lowest, keepform, coefs, true))) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocOpsArgs a;
  a.op = op;
  a.logn = ilog2(p->M);
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.Fin = Fin;
  a.in = (const cpx *)in;
  a.out = (cpx *)out;
  a.par = (const float *)par;
  a.lowest = lowest;
  a.keepform = keepform != 0;
  a.coefs = coefs;
  a.gain = gain;
  a.cf = p->srs;
  a.bpf = p->bpf;
  a.half = (const cpx *)p->half.p;
  a.w2 = (const cpx *)p->w2.p;
  a.grid_max = p->ops_grid_max;
  HIP_TRY(launch_pvoc_ops(a, p->di, s));
  return CLFA_SUCCESS;
}

// the blocking forms: the same checks on the host arrays, then the per-frame values, then copies around the device form
static int pvoc_ops_host(clfa_pvoc *p, int op, const float *in, long Fin, const float *par, float *out, long F, int lowest,
                         int keepform, float gain, int coefs) {
  const int chk = pvoc_ops_check(p, op, in, Fin, par, out, F, lowest, keepform, coefs, false);
  if (chk < 0) return chk;
  for (long f = 0; f < F && op != PVOC_READ; f++) {
    if (!std::isfinite(par[f]) || (op == PVOC_SCALE && !(par[f] >= 0.25f && par[f] <= 4.f))) return CLFA_INVALID_VALUE;
  }
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  return pvoc_staged(p, {{false, in, &p->sframes, pvoc_frame_bytes(p, Fin)}, {true, out, &p->sop_out, pvoc_frame_bytes(p, F)},
                         {false, par, &p->sop_par, sizeof(float) * (size_t)F}}, [&] {
                       return pvoc_ops_dev(p, op, p->sframes.p, Fin, p->sop_par.p, p->sop_out.p, F, lowest, keepform, gain,
                                           coefs, p->stream);
                     });
}

int clfa_pvoc_scale_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, long F, const void *scale, int keepform,
                        float gain, int coefs, void *stream) {
  return pvoc_ops_dev(p, PVOC_SCALE, frames_in, F, scale, frames_out, F, 1, keepform, gain, coefs, stream);
}
int clfa_pvoc_shift_dev(clfa_pvoc *p, const void *frames_in, void *frames_out, long F, const void *shift, int lowest_bin,
                        int keepform, float gain, int coefs, void *stream) {
  return pvoc_ops_dev(p, PVOC_SHIFT, frames_in, F, shift, frames_out, F, lowest_bin, keepform, gain, coefs, stream);
}
int clfa_pvoc_read_dev(clfa_pvoc *p, const void *frames_in, long Fin, const void *pos, void *frames_out, long Fout,
                       void *stream) {
  return pvoc_ops_dev(p, PVOC_READ, frames_in, Fin, pos, frames_out, Fout, 1, 0, 1.f, 1, stream);
}
int clfa_pvoc_scale(clfa_pvoc *p, const float *frames_in, float *frames_out, long F, const float *scale, int keepform,
                    float gain, int coefs) {
  return pvoc_ops_host(p, PVOC_SCALE, frames_in, F, scale, frames_out, F, 1, keepform, gain, coefs);
}
int clfa_pvoc_shift(clfa_pvoc *p, const float *frames_in, float *frames_out, long F, const float *shift, int lowest_bin,
                    int keepform, float gain, int coefs) {
  return pvoc_ops_host(p, PVOC_SHIFT, frames_in, F, shift, frames_out, F, lowest_bin, keepform, gain, coefs);
}
int clfa_pvoc_read(clfa_pvoc *p, const float *frames_in, long Fin, const float *pos, float *frames_out, long Fout) {
  return pvoc_ops_host(p, PVOC_READ, frames_in, Fin, pos, frames_out, Fout, 1, 0, 1.f, 1);
}
const char *clfa_pvoc_ops_kernel_name(const clfa_pvoc *p, int op, int keepform) {
  if (!p || p->err || op < PVOC_SCALE || op > PVOC_READ) return "";
  return op == PVOC_READ ? "k_pvoc_read" : (keepform ? "k_pvoc_formant" : "k_pvoc_map");
}

int clfa_pvoc_analyze(clfa_pvoc *p, const float *spectra, float *frames_out, long F) {
  if (int e = obj_error(p)) return e;
  if (!pvoc_count_ok(F) || (F > 0 && (!spectra || !frames_out))) return CLFA_INVALID_VALUE;
  if (F == 0) return CLFA_SUCCESS;
  return pvoc_staged(p, {{false, spectra, &p->sspec, pvoc_spec_bytes(p, F)}, {true, frames_out, &p->sframes, pvoc_frame_bytes(p, F)}},
                     [&] { return clfa_pvoc_analyze_dev(p, p->sspec.p, p->sframes.p, F, p->stream); });
}

int clfa_pvoc_synthesize(clfa_pvoc *p, const float *frames, float *spectra_out, long F) {
  if (int e = obj_error(p)) return e;
  if (!pvoc_count_ok(F) || (F > 0 && (!frames || !spectra_out))) return CLFA_INVALID_VALUE;
  if (F == 0) return CLFA_SUCCESS;
  return pvoc_staged(p, {{true, spectra_out, &p->sspec, pvoc_spec_bytes(p, F)}, {false, frames, &p->sframes, pvoc_frame_bytes(p, F)}},
                     [&] { return clfa_pvoc_synthesize_dev(p, p->sframes.p, p->sspec.p, F, p->stream); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// two streams of frames -> frames: cross, morph, filter, mix, vocode (pvoc_pair.hip)
// ---------------------------------------------------------------------------------

// The checks that need no device, before the object's own error (as pvoc_ops_check).  0 = go on, 1 = a successful no-op,
// < 0 = the error.  MIX reads neither per-frame array: they are not looked at.
static int pvoc_pair_check(const clfa_pvoc *p, int op, const void *a, const void *b, const void *out, long F,
                           const void *pp, const void *qq, int coefs, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (op < PVOC_CROSS || op > PVOC_VOCODE) return CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (op == PVOC_VOCODE && (coefs < 1 || coefs >= p->M)) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!a || !b || !out) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)a & 7) || ((uintptr_t)b & 7) || ((uintptr_t)out & 7))) return CLFA_INVALID_VALUE;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  if (spans_overlap(a, fbytes, out, fbytes) || spans_overlap(b, fbytes, out, fbytes)) return CLFA_INVALID_VALUE;
  if (op == PVOC_MIX) return CLFA_SUCCESS;
  if (!pp || !qq) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)pp & 3) || ((uintptr_t)qq & 3))) return CLFA_INVALID_VALUE;
  if (spans_overlap(pp, pbytes, out, fbytes) || spans_overlap(qq, pbytes, out, fbytes)) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

static int pvoc_pair_dev(clfa_pvoc *p, int op, const void *a, const void *b, void *out, long F, const void *pp,
                         const void *qq, int coefs, void *stream) {
  if (int e = pvoc_gate(p, pvoc_pair_check(p, op, a, b, out, F, pp, qq, coefs, true))) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocPairArgs g;
  g.op = op;
  g.logn = ilog2(p->M);
  g.M = p->M;
  g.channels = p->channels;
  g.F = F;
  g.a = (const cpx *)a;
  g.b = (const cpx *)b;
  g.out = (cpx *)out;
  g.p = op == PVOC_MIX ? nullptr : (const float *)pp;
  g.q = op == PVOC_MIX ? nullptr : (const float *)qq;
  g.coefs = coefs;
  g.half = (const cpx *)p->half.p;
  g.w2 = (const cpx *)p->w2.p;
  g.grid_max = p->ops_grid_max;
  HIP_TRY(launch_pvoc_pair(g, p->di, s));
  return CLFA_SUCCESS;
}

// the blocking form: the same checks on the host arrays, then the per-frame values, then copies around the device form
static int pvoc_pair_host(clfa_pvoc *p, int op, const float *a, const float *b, float *out, long F, const float *pp,
                          const float *qq, int coefs) {
  const int chk = pvoc_pair_check(p, op, a, b, out, F, pp, qq, coefs, false);
  if (chk < 0) return chk;
  const bool unit_p = op == PVOC_MORPH || op == PVOC_FILTER || op == PVOC_VOCODE, unit_q = op == PVOC_MORPH;
  for (long f = 0; f < F && op != PVOC_MIX; f++) {
    if (!std::isfinite(pp[f]) || !std::isfinite(qq[f])) return CLFA_INVALID_VALUE;
    if ((unit_p && !(pp[f] >= 0.f && pp[f] <= 1.f)) || (unit_q && !(qq[f] >= 0.f && qq[f] <= 1.f))) return CLFA_INVALID_VALUE;
  }
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  const bool mix = op == PVOC_MIX;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  return pvoc_staged(p, {{false, a, &p->sframes, fbytes}, {false, b, &p->spair_b, fbytes}, {true, out, &p->sop_out, fbytes},
                         {false, mix ? nullptr : pp, &p->sop_par, pbytes}, {false, mix ? nullptr : qq, &p->spair_q, pbytes}}, [&] {
                       return pvoc_pair_dev(p, op, p->sframes.p, p->spair_b.p, p->sop_out.p, F, p->sop_par.p, p->spair_q.p,
                                            coefs, p->stream);
                     });
}

extern "C" {

int clfa_pvoc_pair_dev(clfa_pvoc *p, int op, const void *frames_a, const void *frames_b, void *frames_out, long F,
                       const void *pp, const void *qq, int coefs, void *stream) {
  return pvoc_pair_dev(p, op, frames_a, frames_b, frames_out, F, pp, qq, coefs, stream);
}
int clfa_pvoc_pair(clfa_pvoc *p, int op, const float *frames_a, const float *frames_b, float *frames_out, long F,
                   const float *pp, const float *qq, int coefs) {
  return pvoc_pair_host(p, op, frames_a, frames_b, frames_out, F, pp, qq, coefs);
}
const char *clfa_pvoc_pair_kernel_name(const clfa_pvoc *p, int op) {
  if (!p || p->err || op < PVOC_CROSS || op > PVOC_VOCODE) return "";
  return op == PVOC_VOCODE ? "k_pvoc_vocode" : "k_pvoc_pair";
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// one stream of frames -> frames, along the bins: band, mask, stencil, arp, lock, warp (pvoc_shape.hip)
// ---------------------------------------------------------------------------------

static bool pvoc_shape_table(int op) { return op == PVOC_MASK || op == PVOC_STENCIL; }

// The checks that need no device, before the object's own error (as pvoc_ops_check).  0 = go on, 1 = a successful no-op,
// < 0 = the error.  The table is looked at for MASK and STENCIL only.
static int pvoc_shape_check(const clfa_pvoc *p, int op, const void *in, const void *out, long F, const void *par,
                            const void *table, int flags, int lowest, int coefs, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (op < PVOC_BAND || op > PVOC_WARP) return CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (flags & ~(op == PVOC_BAND ? 1 : 0)) return CLFA_INVALID_VALUE;
  if (op == PVOC_WARP && (lowest < 1 || lowest > p->M - 1 || coefs < 1 || coefs >= p->M)) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!in || !out || !par) return CLFA_INVALID_VALUE;
  if (!pvoc_shape_table(op)) table = nullptr;
  else if (!table) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)in & 7) || ((uintptr_t)out & 7) || ((uintptr_t)par & 3) || ((uintptr_t)table & 3)))
    return CLFA_INVALID_VALUE;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = 4 * sizeof(float) * (size_t)F;
  if (spans_overlap(in, fbytes, out, fbytes) || spans_overlap(par, pbytes, out, fbytes)) return CLFA_INVALID_VALUE;
  if (table && spans_overlap(table, sizeof(float) * (size_t)(p->M + 1), out, fbytes)) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

static int pvoc_shape_dev(clfa_pvoc *p, int op, const void *in, void *out, long F, const void *par, const void *table,
                          int flags, int lowest, int coefs, void *stream) {
  if (int e = pvoc_gate(p, pvoc_shape_check(p, op, in, out, F, par, table, flags, lowest, coefs, true))) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocShapeArgs a;
  a.op = op;
  a.logn = ilog2(p->M);
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.in = (const cpx *)in;
  a.out = (cpx *)out;
  a.par = (const float *)par;
  a.table = pvoc_shape_table(op) ? (const float *)table : nullptr;
  a.reject = flags & 1;
  a.lowest = lowest;
  a.coefs = coefs;
  a.bpf = p->bpf;
  a.half = (const cpx *)p->half.p;
  a.w2 = (const cpx *)p->w2.p;
  a.grid_max = p->ops_grid_max;
  HIP_TRY(launch_pvoc_shape(a, p->di, s));
  return CLFA_SUCCESS;
}

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

// the blocking form: the same checks on the host arrays, then the per-frame values, then copies around the device form
static int pvoc_shape_host(clfa_pvoc *p, int op, const float *in, float *out, long F, const float *par, const float *table,
                           int flags, int lowest, int coefs) {
  const int chk = pvoc_shape_check(p, op, in, out, F, par, table, flags, lowest, coefs, false);
  if (chk < 0) return chk;
  for (long f = 0; f < F; f++)
    if (!pvoc_shape_row_ok(op, par + 4 * f)) return CLFA_INVALID_VALUE;
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  const bool tab = pvoc_shape_table(op);
  const size_t fbytes = pvoc_frame_bytes(p, F);
  return pvoc_staged(p, {{false, in, &p->sframes, fbytes}, {true, out, &p->sop_out, fbytes},
                         {false, par, &p->sop_par, 4 * sizeof(float) * (size_t)F},
                         {false, tab ? table : nullptr, &p->sshape_tab, sizeof(float) * (size_t)(p->M + 1)}}, [&] {
                       return pvoc_shape_dev(p, op, p->sframes.p, p->sop_out.p, F, p->sop_par.p, tab ? p->sshape_tab.p : nullptr,
                                             flags, lowest, coefs, p->stream);
                     });
}

extern "C" {

int clfa_pvoc_shape_dev(clfa_pvoc *p, int op, const void *frames_in, void *frames_out, long F, const void *par,
                        const void *table, int flags, int lowest_bin, int coefs, void *stream) {
  return pvoc_shape_dev(p, op, frames_in, frames_out, F, par, table, flags, lowest_bin, coefs, stream);
}
int clfa_pvoc_shape(clfa_pvoc *p, int op, const float *frames_in, float *frames_out, long F, const float *par,
                    const float *table, int flags, int lowest_bin, int coefs) {
  return pvoc_shape_host(p, op, frames_in, frames_out, F, par, table, flags, lowest_bin, coefs);
}
const char *clfa_pvoc_shape_kernel_name(const clfa_pvoc *p, int op) {
  if (!p || p->err || op < PVOC_BAND || op > PVOC_WARP) return "";
  return op == PVOC_WARP ? "k_pvoc_warp" : (op == PVOC_LOCK ? "k_pvoc_lock" : "k_pvoc_shape");
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// frames -> frames along the stream, with carried state: blur, smooth, freeze (pvoc_time.hip)
// ---------------------------------------------------------------------------------

// The checks that need no device, before the object's own error (as pvoc_ops_check).  0 = go on, 1 = a successful no-op,
// < 0 = the error.  BLUR does not look at q.  Whether the blur has been set up is pvoc_time_ready's, after these (and, in
// the blocking form, after the per-frame values).
static int pvoc_time_check(const clfa_pvoc *p, int op, const void *in, const void *out, long F, const void *pp,
                           const void *qq, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (op < PVOC_BLUR || op > PVOC_FREEZE) return CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!in || !out || !pp || (op != PVOC_BLUR && !qq)) return CLFA_INVALID_VALUE;
  if (op == PVOC_BLUR) qq = nullptr;
  if (device_ptrs && (((uintptr_t)in & 7) || ((uintptr_t)out & 7) || ((uintptr_t)pp & 3) || ((uintptr_t)qq & 3)))
    return CLFA_INVALID_VALUE;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  if (spans_overlap(in, fbytes, out, fbytes) || spans_overlap(pp, pbytes, out, fbytes)) return CLFA_INVALID_VALUE;
  if (qq && spans_overlap(qq, pbytes, out, fbytes)) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}
static int pvoc_time_ready(const clfa_pvoc *p, int op) {
  return op == PVOC_BLUR && !p->blur_max ? CLFA_INVALID_OPERATION : CLFA_SUCCESS;
}

static DevBuf clfa_pvoc::*pvoc_time_state(int op) {
  return op == PVOC_BLUR ? &clfa_pvoc::bhist : (op == PVOC_SMOOTH ? &clfa_pvoc::tsmooth : &clfa_pvoc::theld);
}

static int pvoc_time_dev(clfa_pvoc *p, int op, const void *in, void *out, long F, const void *pp, const void *qq,
                         void *stream) {
  int chk = pvoc_time_check(p, op, in, out, F, pp, qq, true);
  if (chk == 0) chk = pvoc_time_ready(p, op);
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocTimeArgs a;
  a.op = op;
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.in = (const cpx *)in;
  a.out = (cpx *)out;
  a.p = (const float *)pp;
  a.q = op == PVOC_BLUR ? nullptr : (const float *)qq;
  a.state = (cpx *)(p->*pvoc_time_state(op)).p;
  a.spare = (cpx *)p->bspare.p;
  a.max_frames = p->blur_max;
  a.grid_max = p->ops_grid_max;
  HIP_TRY(launch_pvoc_time(a, p->di, s));
  return CLFA_SUCCESS;
}

// the blocking form: the same checks on the host arrays, then the per-frame values, then copies around the device form
static int pvoc_time_host(clfa_pvoc *p, int op, const float *in, float *out, long F, const float *pp, const float *qq) {
  int chk = pvoc_time_check(p, op, in, out, F, pp, qq, false);
  if (chk < 0) return chk;
  for (long f = 0; f < F; f++) {
    if (!std::isfinite(pp[f]) || (op != PVOC_BLUR && !std::isfinite(qq[f]))) return CLFA_INVALID_VALUE;
    if (op == PVOC_BLUR && (!(pp[f] >= 1.f) || (p->blur_max && !(pp[f] <= (float)p->blur_max)))) return CLFA_INVALID_VALUE;
    if (op == PVOC_SMOOTH && !(pp[f] >= 0.f && pp[f] <= 1.f && qq[f] >= 0.f && qq[f] <= 1.f)) return CLFA_INVALID_VALUE;
  }
  if (chk == 0) chk = pvoc_time_ready(p, op);
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  const bool blur = op == PVOC_BLUR;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  return pvoc_staged(p, {{false, in, &p->sframes, fbytes}, {true, out, &p->sop_out, fbytes}, {false, pp, &p->sop_par, pbytes},
                         {false, blur ? nullptr : qq, &p->spair_q, pbytes}}, [&] {
                       return pvoc_time_dev(p, op, p->sframes.p, p->sop_out.p, F, p->sop_par.p, blur ? nullptr : p->spair_q.p,
                                            p->stream);
                     });
}

extern "C" {

int clfa_pvoc_blur_setup(clfa_pvoc *p, int max_frames) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
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
  return pvoc_time_dev(p, op, frames_in, frames_out, F, pp, qq, stream);
}
int clfa_pvoc_time(clfa_pvoc *p, int op, const float *frames_in, float *frames_out, long F, const float *pp,
                   const float *qq) {
  return pvoc_time_host(p, op, frames_in, frames_out, F, pp, qq);
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
// frames -> eight descriptors per frame, with carried state (pvoc_desc.hip)
// ---------------------------------------------------------------------------------

static size_t pvoc_desc_bytes(const clfa_pvoc *p, long F) { return 8 * sizeof(float) * (size_t)p->channels * (size_t)F; }

// The checks that need no device, before the object's own error (as pvoc_ops_check).  0 = go on, 1 = a successful no-op,
// < 0 = the error.
static int pvoc_desc_check(const clfa_pvoc *p, const void *in, const void *desc, long F, int first_bin, int nbins,
                           int rectify, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (first_bin < 0 || nbins < 1 || (long)first_bin + nbins - 1 > p->M) return CLFA_INVALID_VALUE;
  if (rectify != 0 && rectify != 1) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!in || !desc) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)in & 7) || ((uintptr_t)desc & 3))) return CLFA_INVALID_VALUE;
  if (spans_overlap(in, pvoc_frame_bytes(p, F), desc, pvoc_desc_bytes(p, F))) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

extern "C" {

int clfa_pvoc_desc_dev(clfa_pvoc *p, const void *frames_in, void *desc, long F, int first_bin, int nbins, int rectify,
                       void *stream) {
  if (int e = pvoc_gate(p, pvoc_desc_check(p, frames_in, desc, F, first_bin, nbins, rectify, true))) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  PvocDescArgs a;
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.in = (const cpx *)frames_in;
  a.desc = (float *)desc;
  a.last = (cpx *)p->dlast.p;
  a.lo = first_bin;
  a.hi = first_bin + nbins - 1;
  a.rectify = rectify;
  a.cf = p->srs;
  a.grid_max = p->ops_grid_max;
  HIP_TRY(launch_pvoc_desc(a, p->di, s));
  return CLFA_SUCCESS;
}

int clfa_pvoc_desc(clfa_pvoc *p, const float *frames_in, float *desc, long F, int first_bin, int nbins, int rectify) {
  if (int e = pvoc_gate(p, pvoc_desc_check(p, frames_in, desc, F, first_bin, nbins, rectify, false))) return pvoc_done(e);
  return pvoc_staged(p, {{false, frames_in, &p->sframes, pvoc_frame_bytes(p, F)}, {true, desc, &p->sdesc, pvoc_desc_bytes(p, F)}},
                     [&] { return clfa_pvoc_desc_dev(p, p->sframes.p, p->sdesc.p, F, first_bin, nbins, rectify, p->stream); });
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
// frames -> samples: the oscillator bank (pvoc_adsyn.hip)
// ---------------------------------------------------------------------------------

// The checks that need no device, before the object's own error (as pvoc_ops_check).  0 = go on, 1 = a successful no-op,
// < 0 = the error.
static int pvoc_adsyn_check(const clfa_pvoc *p, const void *frames, long F, const void *fmod, int first_bin, int nbins,
                            int step, const void *signal, long signal_stride, bool device_ptrs) {
  if (!p) return CLFA_INVALID_VALUE;
  if (!p->M) return p->err ? p->err : CLFA_INVALID_VALUE;
  if (!pvoc_count_ok(F)) return CLFA_INVALID_VALUE;
  if (step < 1 || nbins < 1 || first_bin < 0 || (long)first_bin + ((long)nbins - 1) * step > p->M) return CLFA_INVALID_VALUE;
  if (signal_stride < F * p->hop) return CLFA_INVALID_VALUE;
  if (F == 0) return 1;
  if (!frames || !signal) return CLFA_INVALID_VALUE;
  if (device_ptrs && (((uintptr_t)frames & 7) || ((uintptr_t)signal & 3) || ((uintptr_t)fmod & 3))) return CLFA_INVALID_VALUE;
  // the output's rows and the gaps between them, as one span
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const size_t obytes = sizeof(float) * ((size_t)(p->channels - 1) * (size_t)signal_stride + (size_t)F * p->hop);
  if (spans_overlap(frames, fbytes, signal, obytes)) return CLFA_INVALID_VALUE;
  if (fmod && spans_overlap(fmod, sizeof(float) * (size_t)F, signal, obytes)) return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

static size_t pvoc_adsyn_ws_bytes(const clfa_pvoc *p) {
  return sizeof(unsigned long long) * pvoc_bins(p) * (size_t)p->acap + (sizeof(int) + sizeof(float)) * pvoc_bins(p);
}

extern "C" {

int clfa_pvoc_adsyn_dev(clfa_pvoc *p, const void *frames, long F, const void *fmod, int first_bin, int nbins, int step,
                        float gain, void *signal, long signal_stride, void *stream) {
  if (int e = pvoc_gate(p, pvoc_adsyn_check(p, frames, F, fmod, first_bin, nbins, step, signal, signal_stride, true)))
    return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  const long held = p->acap;   // the whole workspace at the first need: its address never changes afterwards
  HIP_TRY(p->order.use(s));
  if (int e = ensure_workspaces({{&p->aws, pvoc_adsyn_ws_bytes(p)}}, s)) return e;
  PvocAdsynArgs a;
  a.M = p->M;
  a.channels = p->channels;
  a.hop = p->hop;
  a.F = F;
  a.frames = (const float *)frames;
  a.fmod = (const float *)fmod;
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
  a.signal = (float *)signal;
  a.sstride = signal_stride;
  a.grid_max = p->adsyn_grid_max;
  return pvoc_subbatches(F, held, [&](long f0, long nf) { return launch_pvoc_adsyn(a, f0, nf, p->di, s); });
}

int clfa_pvoc_adsyn(clfa_pvoc *p, const float *frames, long F, const float *fmod, int first_bin, int nbins, int step,
                    float gain, float *signal, long signal_stride) {
  if (int e = pvoc_gate(p, pvoc_adsyn_check(p, frames, F, fmod, first_bin, nbins, step, signal, signal_stride, false)))
    return pvoc_done(e);
  // the staged output's rows are packed, the caller's signal_stride floats apart
  return pvoc_staged(p, {{false, frames, &p->sframes, pvoc_frame_bytes(p, F)},
                         {true, signal, &p->ssig, sizeof(float) * (size_t)F * p->hop, (size_t)p->channels,
                          sizeof(float) * (size_t)signal_stride},
                         {false, fmod, &p->sfmod, sizeof(float) * (size_t)F}},
                     [&] {
                       return clfa_pvoc_adsyn_dev(p, p->sframes.p, F, fmod ? p->sfmod.p : nullptr, first_bin, nbins, step,
                                                  gain, p->ssig.p, F * p->hop, p->stream);
                     });
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
