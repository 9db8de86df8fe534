// pvoc_stream_host.cpp — C ABI of the phase vocoder (include/clfft_amd.h), the calls from frames to frames along the stream,
// each with a carried history and a set-up: time (blur / smooth / freeze) and the per-bin delay.  Over pvoc_host.hpp's
// pvoc_call, pvoc_family_setup and pvoc_read_state.
#include "pvoc_host.hpp"
#include "pvoc_launch.hpp"

using namespace clfa;

// a history of `frames` frames per channel as at creation: EMPTY bins (on p->stream)
static hipError_t pvoc_fill_history(clfa_pvoc *p, DevBuf &b, int frames) {
  return launch_pvoc_time_fill((cpx *)b.p, (long)p->channels * frames, p->M, p->srs, p->stream);
}

// ---------------------------------------------------------------------------------
// frames -> frames along the stream, with carried state: blur, smooth, freeze (pvoc_time.hip)
// ---------------------------------------------------------------------------------

// whether the blur has been set up: asked after the arguments (and, in the blocking form, after the per-frame values)
static int pvoc_time_ready(const clfa_pvoc *p, int op) {
  return op == PVOC_BLUR && !p->time.blur_max ? CLFA_INVALID_OPERATION : CLFA_SUCCESS;
}

static DevBuf &pvoc_time_state(clfa_pvoc *p, int op) {
  return op == PVOC_BLUR ? p->time.hist : (op == PVOC_SMOOTH ? p->time.smooth : p->time.held);
}

// BLUR does not look at q.  The blocking form asks finite values, the blur's lengths in 1..max_frames (where it is set
// up) and the smoothing's weights in [0, 1].
static int pvoc_time_call(clfa_pvoc *p, bool blocking, int op, const void *in, void *out, long F, const void *pp,
                          const void *qq, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = op >= PVOC_BLUR && op <= PVOC_FREEZE;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  const int blur_max = p->time.blur_max;
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::stage_in},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},
                              {pp, pbytes, 4, false, &clfa_pvoc::stage_rows},
                              {qq, pbytes, 4, false, &clfa_pvoc::stage_rows2, op != PVOC_BLUR}};
  const auto values_ok = [&] {
    const float *P = (const float *)pp, *Q = (const float *)qq;
    for (long f = 0; f < F; f++) {
      if (!std::isfinite(P[f]) || (op != PVOC_BLUR && !std::isfinite(Q[f]))) return false;
      if (op == PVOC_BLUR && (!(P[f] >= 1.f) || (blur_max && !(P[f] <= (float)blur_max)))) return false;
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
                     a.state = (cpx *)pvoc_time_state(p, op).p;
                     a.spare = (cpx *)p->time.spare.p;
                     a.max_frames = blur_max;
                     return launch_pvoc_time(a, p->di, s);
                   });
}

extern "C" {

int clfa_pvoc_blur_setup(clfa_pvoc *p, int max_frames) {
  return pvoc_family_setup<2>(
      p, [&] { return max_frames >= 1 && max_frames <= 4096; },
      [&](DevBuf(&fresh)[2]) {   // the history, filled, and the spare
        for (DevBuf &b : fresh)
          if (int e = b.ensure(pvoc_frame_bytes(p, max_frames - 1))) return e;
        HIP_TRY(pvoc_fill_history(p, fresh[0], max_frames - 1));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return CLFA_SUCCESS;
      },
      [&](DevBuf(&fresh)[2]) {
        p->time.hist.swap(fresh[0]);
        p->time.spare.swap(fresh[1]);
        p->time.blur_max = max_frames;
      });
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
  const size_t bytes = pvoc_frame_bytes(p, op == PVOC_BLUR ? (p->time.blur_max > 0 ? p->time.blur_max - 1 : 0) : 1);
  return pvoc_read_state(p, pvoc_time_ready(p, op), {{host, &pvoc_time_state(p, op), bytes}});
}

size_t clfa_pvoc_time_state_bytes(const clfa_pvoc *p) {
  return p ? p->time.smooth.bytes + p->time.held.bytes + p->time.hist.bytes + p->time.spare.bytes : 0;
}
int clfa_pvoc_blur_max_frames(const clfa_pvoc *p) { return p ? p->time.blur_max : 0; }
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
static int pvoc_delay_ready(const clfa_pvoc *p) { return p->delay.max < 0 ? CLFA_INVALID_OPERATION : CLFA_SUCCESS; }

// A NULL feedback is none.  The blocking form asks delays in 0..max_delay (before the setup: 0..4096, what a setup can make
// valid) and finite feedbacks in [-1, 1]; the device form clamps the delays and takes the feedbacks as they are.
static int pvoc_delay_call(clfa_pvoc *p, bool blocking, const void *in, void *out, long F, const void *delays,
                           const void *feedback, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const int L = p->delay.max;
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::stage_in},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},
                              {delays, sizeof(int) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::stage_itable},
                              {feedback, sizeof(float) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::stage_table, feedback != nullptr}};
  const auto values_ok = [&] {
    const int *d = (const int *)delays;
    const float *g = (const float *)feedback;
    for (int k = 0; k <= p->M; k++) {
      if (d[k] < 0 || d[k] > (L >= 0 ? L : kPvocDelayMax)) return false;
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
    a.xhist = (cpx *)p->delay.xhist.p;
    a.yhist = (cpx *)p->delay.yhist.p;
    a.spare = (cpx *)p->delay.spare.p;
    a.L = L;
    return launch_pvoc_delay(a, p->di, s);
  });
}

extern "C" {

int clfa_pvoc_delay_setup(clfa_pvoc *p, int max_delay) {
  return pvoc_family_setup<3>(
      p, [&] { return max_delay >= 0 && max_delay <= kPvocDelayMax; },
      [&](DevBuf(&fresh)[3]) {   // the two histories, filled, and the spare
        for (DevBuf &b : fresh)
          if (int e = b.ensure(pvoc_frame_bytes(p, max_delay))) return e;
        for (int i = 0; i < 2; i++) HIP_TRY(pvoc_fill_history(p, fresh[i], max_delay));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return CLFA_SUCCESS;
      },
      [&](DevBuf(&fresh)[3]) {
        p->delay.xhist.swap(fresh[0]);
        p->delay.yhist.swap(fresh[1]);
        p->delay.spare.swap(fresh[2]);
        p->delay.max = max_delay;
      });
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
  const size_t bytes = pvoc_frame_bytes(p, p->delay.max > 0 ? p->delay.max : 0);
  return pvoc_read_state(p, pvoc_delay_ready(p), {{host, which ? &p->delay.yhist : &p->delay.xhist, bytes}});
}

size_t clfa_pvoc_delay_state_bytes(const clfa_pvoc *p) {
  return p ? p->delay.xhist.bytes + p->delay.yhist.bytes + p->delay.spare.bytes : 0;
}
int clfa_pvoc_delay_max_frames(const clfa_pvoc *p) { return p ? p->delay.max : -1; }
const char *clfa_pvoc_delay_kernel_name(const clfa_pvoc *p, int feedback) {
  return !p || p->err ? "" : (feedback ? "k_pvoc_delay_fb" : "k_pvoc_delay");
}

}  // extern "C"
