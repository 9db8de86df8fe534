// pvoc_host.hpp — what the host sources of the phase vocoder share (pvoc_host.cpp: the object and spectra <-> frames,
// pvoc_frames_host.cpp, pvoc_stream_host.cpp, pvoc_rows_host.cpp, pvoc_signal_host.cpp: the families of calls), on top of
// host.hpp: the object, the byte helpers, the sub-batches of a scan, the blocking read of states, the one path of a
// family's set-up, and the one path of a call — the description of its arrays (PvocArray: host.hpp's HostArray, checked by
// arrays_ok, staged by staged_call), the device form, and pvoc_call, which puts a call's results in the header's order.
// No launch header is included here: each source adds the ones of its own families.
// Everything here is inline and hidden, as in host.hpp.
#pragma once
#include "host.hpp"

struct clfa_pvoc {
  clfa::DeviceInfo di;
  int size = 0, hop = 0, M = 0, channels = 0;
  double sr = 0;
  float sh = 0.f, srs = 0.f, kf = 0.f;   // size / hop, sr / size, hop / sr: divided in double, rounded once
  int err = 0;
  char log[512];
  hipStream_t stream = nullptr;
  clfa::DevBuf etab;   // e[k], M + 1 complex
  // spectra <-> frames (pvoc_kernels.hip): the two states, channels x (M + 1) complex / uint32; the scan's chunk sums,
  // allocated by the first synthesis that needs them; chunks per sub-batch (CLFA_PVOC_CHUNKS_MAX: tuning switch, read at
  // creation)
  struct Scan {
    clfa::DevBuf prev, theta, ws;
    long cap = 1;
  } scan;
  // the frame operations (pvoc_ops.hip and the families after it): size / sr, the Clrfft tables of size (forward sign) for
  // the formant envelope, the cap on a launch's workgroups (CLFA_PVOC_OPS_GRID_MAX, 0 = none)
  float bpf = 0.f;
  clfa::DevBuf half, w2;
  int ops_grid_max = 0;
  // the oscillator bank (pvoc_adsyn.hip): 1 / sr, its state per channel and bin (P uint64, W int32, A float32), the ramp
  // w_j, its own workspace (the 64-bit chunk sums of one sub-batch, then the endpoints a sub-batch starts from), the
  // chunks per sub-batch, the cap on its workgroups (CLFA_PVOC_ADSYN_GRID_MAX, 0 = none)
  struct Adsyn {
    float ks = 0.f;
    clfa::DevBuf phase, w, amp, ramp, ws;
    long cap = 1;
    int grid_max = 0;
  } adsyn;
  // the operations along the frames (pvoc_time.hip): the smoothing's y and the freeze's held, channels x (M + 1) pairs
  // each; the blur's history of max_frames - 1 frames per channel and its spare (clfa_pvoc_blur_setup; blur_max 0 before)
  struct Time {
    clfa::DevBuf smooth, held, hist, spare;
    int blur_max = 0;
  } time;
  // the per-bin delay (pvoc_delay.hip): the last `max` input frames and the last `max` output frames per channel, the
  // spare their commits share (clfa_pvoc_delay_setup; max -1 before: 0 is a setup too)
  struct Delay {
    clfa::DevBuf xhist, yhist, spare;
    int max = -1;
  } delay;
  // the descriptors (pvoc_desc.hip): the stream's previous frame, channels x (M + 1) pairs of which the amps are the
  // state `last`
  struct Desc {
    clfa::DevBuf last;
  } desc;
  // the filter bank (bank_kernels.hip; clfa_pvoc_bank_setup, B -1 before): the bands, the schedule that deals them to the
  // kernel's rows (steps: its longest row), the weights and the DCT table, transposed.  Configuration, not stream state:
  // clfa_pvoc_reset leaves it alone
  struct Bank {
    clfa::DevBuf bands, sched, weights, dct;
    int B = -1, steps = 0;
  } bank;
  // Staging of the blocking forms, one slot per role, whichever family the call belongs to; no call puts two of its arrays
  // in one slot (staged_call refuses that).  A blocking form waits for its stream before it returns, so nothing of one
  // call is in a slot when the next call fills it.  Members of the object itself: a HostArray names its slot as one.
  clfa::DevBuf stage_spectra, stage_in, stage_in2, stage_out;   // spectra; frames in, second frames in, frames out
  clfa::DevBuf stage_rows, stage_rows2;       // per-frame float rows (par, p, n, pos ...), the second of them (q)
  clfa::DevBuf stage_table, stage_itable;     // a float table over the bins or the window; an int table (delays, starts)
  clfa::DevBuf stage_signal, stage_fmod;      // signal rows, in or out; the oscillator bank's fmod
  clfa::DevBuf stage_out_rows, stage_out_list;   // rows per frame out (desc, bands, pitch); a list out (bins, profile, peaks)
  clfa::StreamOrder order;
};

namespace clfa {

inline size_t pvoc_bins(const clfa_pvoc *p) { return (size_t)p->channels * (p->M + 1); }
inline size_t pvoc_frame_bytes(const clfa_pvoc *p, long F) { return 2 * sizeof(float) * pvoc_bins(p) * (size_t)F; }
inline size_t pvoc_spec_bytes(const clfa_pvoc *p, long F) { return sizeof(cpx) * (size_t)p->channels * (size_t)F * p->M; }
inline bool pvoc_count_ok(long F) { return F >= 0 && F <= 0x7fffffffL; }   // a frame count

// chunks per sub-batch: sub-batches bound a scan's workspace (`word` bytes per channel, chunk and bin) to about 64 MiB;
// CLFA_PVOC_CHUNKS_MAX (tuning switch, read at creation) lowers it
inline long pvoc_chunks_cap(const clfa_pvoc *p, size_t word) {
  long cap = (64L << 20) / ((long)word * (long)pvoc_bins(p));
  cap = cap < 1 ? 1 : (cap > 4096 ? 4096 : cap);
  if (const long v = env_long("CLFA_PVOC_CHUNKS_MAX", 0, cap)) cap = v;
  return cap;
}

// launch(f0, nf) over the call's F frames in sub-batches of at most `frames` (the chunks held x the chunk): each advances
// the state by its frames, the next one starts from there
template <class Launch>
inline int pvoc_subbatches(long F, long frames, Launch launch) {
  for (long f0 = 0; f0 < F; f0 += frames) HIP_TRY(launch(f0, F - f0 < frames ? F - f0 : frames));
  return CLFA_SUCCESS;
}

// the object's earlier work is complete (blocking); refused while its stream is being captured
inline int pvoc_quiesce(clfa_pvoc *p) {
  if (!p->order.any) return CLFA_SUCCESS;
  if (StreamOrder::capturing(p->order.last)) return CLFA_INVALID_OPERATION;
  if (hipStreamSynchronize(p->order.last) != hipSuccess) {   // a stream the caller has destroyed: wait for the device
    (void)hipGetLastError();
    HIP_TRY(hipDeviceSynchronize());
  }
  return CLFA_SUCCESS;
}

// The blocking read of states of a non-NULL object: the object's error, NULL hosts as invalid values, `ready` (a family's
// set-up), then the object's earlier work is waited for and `bytes` of every state copied (none where that is 0).  What an
// entry point answers ahead of the object's error, it checks before it comes here.
struct PvocState {
  void *host;
  const DevBuf *buf;
  size_t bytes;
};
inline int pvoc_read_state(clfa_pvoc *p, int ready, std::initializer_list<PvocState> states) {
  if (p->err) return p->err;
  for (const PvocState &st : states)
    if (!st.host) return CLFA_INVALID_VALUE;
  if (ready) return ready;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  for (const PvocState &st : states)
    if (st.bytes) HIP_TRY(hipMemcpy(st.host, st.buf->p, st.bytes, hipMemcpyDeviceToHost));
  return CLFA_SUCCESS;
}

// The results of the argument checks: 0 = go on, 1 = a successful no-op, < 0 = the error.  A call goes on after its
// device-free checks with the error, else the object's own error, else chk:
//   if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
inline int pvoc_gate(const clfa_pvoc *p, int chk) { return chk < 0 ? chk : (p->err ? p->err : chk); }
inline int pvoc_done(int e) { return e == 1 ? CLFA_SUCCESS : e; }

// what a launch answers, as a status
inline int pvoc_code(int e) { return e; }
inline int pvoc_code(hipError_t e) {
  HIP_TRY(e);
  return CLFA_SUCCESS;
}

// One array of a call (HostArray, host.hpp; the rules: arrays_ok, overlap.hpp): the outputs are one, or two (trace's
// frames and bin list, demix's frames and profile, pitch's rows and peak list); what an op does not look at is not `used`:
// MIX's p and q, BLUR's q, most tables, a NULL fmod
using PvocArray = HostArray<clfa_pvoc>;

// The device forms after their checks (chk): the error, else the object's own, else a no-op's success, ahead of any device
// work; then launch(stream) on the object's device, ordered behind the object's earlier work
template <class Launch>
inline int pvoc_dev_form(clfa_pvoc *p, int chk, void *stream, Launch launch) {
  if (int e = pvoc_gate(p, chk)) return pvoc_done(e);
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  return pvoc_code(launch(s));
}

// The object can take a call's arguments at all: a NULL object is an invalid value, one whose creation arguments were bad
// (M == 0) answers with that error.  One that only found no device goes on: a bad argument is still an invalid value there,
// which is why a call's checks come before the object's own error.
inline int pvoc_usable(const clfa_pvoc *p) {
  if (!p) return CLFA_INVALID_VALUE;
  return p->M ? CLFA_SUCCESS : (p->err ? p->err : CLFA_INVALID_VALUE);
}

// A family's set-up (blur, delay, bank), blocking: the object usable, value_ok() (else an invalid value), the object's own
// error, its earlier work waited for; then build(fresh) allocates and fills every new buffer, and only when all of it
// succeeded commit(fresh) swaps them into the object and records the scalars.  A failure leaves the object as it was: what
// was allocated goes with `fresh`.
template <size_t N, class Ok, class Build, class Commit>
inline int pvoc_family_setup(clfa_pvoc *p, Ok value_ok, Build build, Commit commit) {
  if (int e = pvoc_usable(p)) return e;
  if (!value_ok()) return CLFA_INVALID_VALUE;
  if (p->err) return p->err;
  ENTER_DEVICE(p->di.device);
  if (int e = pvoc_quiesce(p)) return e;
  DevBuf fresh[N];
  if (int e = build(fresh)) return e;
  commit(fresh);
  return CLFA_SUCCESS;
}

// Either form of a call of F frames on a usable object, the results in the order of the header: the op code and the
// scalar ranges (scalars_ok: the family's), F == 0 as a successful no-op, the arrays, in a blocking form the per-frame
// values (values_ok(): the family's rule on the host arrays), `ready` (a family's set-up), the object's own error; then
// launch(d, stream) with the arrays the device reads and writes: the caller's in a device form, the staged ones in a
// blocking form.
template <size_t N, class Values, class Launch>
inline int pvoc_call(clfa_pvoc *p, bool blocking, void *stream, bool scalars_ok, long F, const PvocArray (&arrays)[N], int ready,
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
inline bool pvoc_no_values() { return true; }

// the fields every launch of a frame operation takes (A: a family's *Args over PvocFramesArgs, pvoc_launch.hpp)
template <class A>
inline void pvoc_frames_args(const clfa_pvoc *p, long F, A &a) {
  a.M = p->M;
  a.channels = p->channels;
  a.F = F;
  a.logn = ilog2(p->M);
  a.half = (const cpx *)p->half.p;
  a.w2 = (const cpx *)p->w2.p;
  a.grid_max = p->ops_grid_max;
}

}  // namespace clfa
