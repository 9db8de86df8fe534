// pvoc_frames_host.cpp — C ABI of the phase vocoder (include/clfft_amd.h), the stateless calls from frames to frames: ops
// (scale / shift / read), pair, shape, trace, demix.  One function per family over pvoc_host.hpp's pvoc_call: scalar rules,
// array list, per-frame value rule, launch.
#include "pvoc_host.hpp"
#include "pvoc_launch.hpp"

using namespace clfa;

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
  const PvocArray arrays[] = {{in, pvoc_frame_bytes(p, Fin), 8, false, &clfa_pvoc::stage_in},
                              {out, pvoc_frame_bytes(p, F), 8, true, &clfa_pvoc::stage_out},
                              {par, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::stage_rows}};
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
// two streams of frames -> frames: cross, morph, filter, mix, vocode (pvoc_pair.hip)
// ---------------------------------------------------------------------------------

// MIX reads neither per-frame array.  The blocking form asks finite values, and the depths and weights in [0, 1].
static int pvoc_pair_call(clfa_pvoc *p, bool blocking, int op, const void *a, const void *b, void *out, long F,
                          const void *pp, const void *qq, int coefs, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = op >= PVOC_CROSS && op <= PVOC_VOCODE && !(op == PVOC_VOCODE && (coefs < 1 || coefs >= p->M));
  const bool mix = op == PVOC_MIX;
  const size_t fbytes = pvoc_frame_bytes(p, F), pbytes = sizeof(float) * (size_t)F;
  const PvocArray arrays[] = {{a, fbytes, 8, false, &clfa_pvoc::stage_in},     {b, fbytes, 8, false, &clfa_pvoc::stage_in2},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},   {pp, pbytes, 4, false, &clfa_pvoc::stage_rows, !mix},
                              {qq, pbytes, 4, false, &clfa_pvoc::stage_rows2, !mix}};
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
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::stage_in},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},
                              {par, 4 * sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::stage_rows},
                              {table, sizeof(float) * (size_t)(p->M + 1), 4, false, &clfa_pvoc::stage_table,
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
// frames -> frames: the N loudest bins of every frame, or all but those, and the list of the bins (pvoc_trace.hip)
// ---------------------------------------------------------------------------------

// A call with two outputs: the frames, and the bin list where `bins` is given (list_n is looked at only then).  Every n
// has a meaning (a NaN or a negative keeps nothing), so the blocking form has no values to refuse.
static int pvoc_trace_call(clfa_pvoc *p, bool blocking, const void *in, void *out, const void *n, void *bins, int list_n,
                           long F, int first_bin, int nbins, int flags, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M &&
                          !(flags & ~CLFA_PVOC_TRACE_RESIDUAL) && !(bins && list_n < 1);
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const size_t lbytes = bins && list_n >= 1 ? sizeof(int) * (size_t)p->channels * (size_t)(F > 0 ? F : 0) * (size_t)list_n : 0;
  const PvocArray arrays[] = {{in, fbytes, 8, false, &clfa_pvoc::stage_in},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},
                              {n, sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::stage_rows},
                              {bins, lbytes, 4, true, &clfa_pvoc::stage_out_list, bins != nullptr}};
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

// A call with two outputs: the frames, and the profile where `az` is given.  par: F rows of (pos, width).  The blocking
// form asks finite values, pos in [-1, 1] and width in [1, 2 points + 1]; the device form clamps.
static int pvoc_demix_call(clfa_pvoc *p, bool blocking, const void *l, const void *r, void *out, const void *par, void *az,
                           long F, int points, int first_bin, int nbins, void *stream) {
  if (int e = pvoc_usable(p)) return e;
  const bool scalars_ok = points >= 1 && points <= 1024 && first_bin >= 0 && nbins >= 1 && (long)first_bin + nbins - 1 <= p->M;
  const size_t fbytes = pvoc_frame_bytes(p, F);
  const size_t abytes = az && scalars_ok ? sizeof(float) * (size_t)p->channels * (size_t)(F > 0 ? F : 0) * (size_t)(2 * points + 1) : 0;
  const PvocArray arrays[] = {{l, fbytes, 8, false, &clfa_pvoc::stage_in},
                              {r, fbytes, 8, false, &clfa_pvoc::stage_in2},
                              {out, fbytes, 8, true, &clfa_pvoc::stage_out},
                              {par, 2 * sizeof(float) * (size_t)F, 4, false, &clfa_pvoc::stage_rows},
                              {az, abytes, 4, true, &clfa_pvoc::stage_out_list, az != nullptr}};
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
