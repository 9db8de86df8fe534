// pconv_matrix_host.cpp — C ABI of the convolution matrix (see include/clfft_amd.h; kernels: pconv_matrix.hip): many
// inputs mixed into many outputs, and its timed crossfade.  Shared plumbing: conv_host.hpp and, below it, host.hpp.
#include "pconv_args.hpp"

using namespace clfa;

struct clfa_pconv_matrix {
  DeviceInfo di;
  int cvs = 0, pts = 0, nparts = 0, inputs = 0, outputs = 0, logb = 0;
  int wp = 0;                    // ring A position, shared by every input
  int err = 0;
  char log[256];
  hipStream_t stream = nullptr;
  DevBuf half, w2f, w2i;         // tables of the pts-bin transforms (as Clpconv)
  DevBuf H, ringA, tail;         // responses, input spectra rings, overlap-add tails
  DevBuf X, Y, P, tail_ws;       // sub-batch workspaces: allocated by the first call that needs them
  DevBuf in1, in2, out;          // staging of the blocking forms (conv_arrays; one input: in2 stays empty)
  DevBuf ir;                     // ... and of the pushes
  PconvMatrixPlan plan;
  int cap = 1;                   // blocks per sub-batch (CLFA_PCONV_MATRIX_BLOCKS_MAX: tuning switch, read at creation)
  StreamOrder order;
  // timed crossfade (push_ir_fade): allocated by the first fade push and kept, so that no address ever changes
  DevBuf H2, tail2;              // the responses faded to and their path's tails; copied over H / tail when the fade ends
  DevBuf Y2, P2, tail_ws2, mix;  // the second path's sub-batch workspaces and its samples (outputs x cap x pts floats)
  long fade_len = 0, fade_done = 0;   // blocks of the pending fade (0: none) and how many of them have been processed
  bool fade_two_mac = false;     // CLFA_PCONV_MATRIX_FADE_MAC=two: two launches of the plain MAC (tuning switch)
};

static BlockShape block_shape(const clfa_pconv_matrix *p) { return {p->pts, p->inputs, p->outputs}; }
// the launcher's view of the object (everything but the call's rows, K and w)
static PconvMatrixArgs mconv_args(const clfa_pconv_matrix *p) {
  PconvMatrixArgs a = pconv_matrix_args(p->logb, p->nparts, p->inputs, p->outputs, p->plan, p->cap, p->half, p->w2f, p->w2i, p->H,
                                        p->ringA, p->tail, p->X, p->Y, p->P, p->tail_ws);
  a.H2 = (const cpx *)p->H2.p;
  a.tail2 = (float *)p->tail2.p;
  a.Y2 = (cpx *)p->Y2.p;
  a.P2 = (cpx *)p->P2.p;
  a.tail_ws2 = (float *)p->tail_ws2.p;
  a.mix = (float *)p->mix.p;
  a.fade_len = p->fade_len;
  a.two_mac = p->fade_two_mac;
  return a;
}

// the sub-batch workspaces of a process call
static int mconv_workspaces(clfa_pconv_matrix *p, hipStream_t s) {
  const size_t frames = sizeof(cpx) * (size_t)p->cap * p->pts;
  return ensure_workspaces({{&p->X, frames * p->inputs},
                            {&p->Y, frames * p->outputs},
                            {&p->P, frames * p->outputs * (size_t)(p->plan.segs - 1)},
                            {&p->tail_ws, sizeof(float) * (size_t)p->outputs * p->pts}},
                           s);
}

static int mconv_setup(clfa_pconv_matrix *p, int device, int cvs, int pts, int inputs, int outputs) {
  p->log[0] = 0;
  p->cvs = cvs;
  p->pts = pts;
  p->inputs = inputs;
  p->outputs = outputs;
  if (!is_pow2(pts) || pts < (1 << kPconvBlocksMinLog) || pts > (1 << kPconvBlocksMaxLog)) {
    snprintf(p->log, sizeof(p->log), "pts must be a power of two, %d..%d (got %d)", 1 << kPconvBlocksMinLog,
             1 << kPconvBlocksMaxLog, pts);
    return CLFA_INVALID_VALUE;
  }
  if (cvs < pts || inputs < 1 || outputs < 1) {
    snprintf(p->log, sizeof(p->log), "need cvs >= pts, inputs >= 1, outputs >= 1 (got %d, %d, %d)", cvs, inputs, outputs);
    return CLFA_INVALID_VALUE;
  }
  p->logb = ilog2(pts);
  p->nparts = cvs / pts;   // floor, as Clpconv
  int e = device_info(device, p->di);
  if (e) return e;
  p->plan = pconv_matrix_plan(pts, p->nparts, inputs, outputs, p->di);
  // tuning switches, read per object (tools/time_mconv.py sweeps them): outputs per MAC tile, reduction segments
  if (const char *env = getenv("CLFA_PCONV_MATRIX_TILE")) {
    if (atoi(env) == 4 || atoi(env) == 16) p->plan.kt = atoi(env);
  }
  if (const char *env = getenv("CLFA_PCONV_MATRIX_SEGS")) {
    if (atoi(env) >= 1 && atoi(env) <= 4096) p->plan.segs = atoi(env);
  }
  if (const char *env = getenv("CLFA_PCONV_MATRIX_FADE_MAC")) p->fade_two_mac = !strcmp(env, "two");
  // sub-batch workspaces X, Y and the segments' partials (CLFA_PCONV_MATRIX_BLOCKS_MAX: read per object, like
  // CLFA_PCONV_BLOCKS_MAX)
  p->cap = subbatch_cap(((long)inputs + (long)outputs * p->plan.segs) * pts * (long)sizeof(cpx), "CLFA_PCONV_MATRIX_BLOCKS_MAX");
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  if ((e = upload_conv_tables(pts, p->half, p->w2f, p->w2i))) return e;
  const size_t frame = sizeof(cpx) * (size_t)pts;
  const size_t hbytes = frame * (size_t)outputs * inputs * p->nparts, abytes = frame * (size_t)inputs * p->nparts;
  const size_t tbytes = sizeof(float) * (size_t)outputs * pts;
  if ((e = p->H.ensure(hbytes)) || (e = p->ringA.ensure(abytes)) || (e = p->tail.ensure(tbytes))) return e;
  // zero responses, history and tails
  HIP_TRY(hipMemsetAsync(p->H.p, 0, hbytes, p->stream));
  HIP_TRY(hipMemsetAsync(p->ringA.p, 0, abytes, p->stream));
  HIP_TRY(hipMemsetAsync(p->tail.p, 0, tbytes, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

// the blocking host pushes after their refusals: the outputs x inputs packed rows staged, then the device form `push`
template <class Push>
static int mconv_push_host(clfa_pconv_matrix *p, const float *ir, Push push) {
  ENTER_DEVICE(p->di.device);
  const long len = (long)p->nparts * p->pts;
  return push_host(p, ir, sizeof(float) * (size_t)len * p->outputs * p->inputs, [&](const void *rows) { return push(rows, len); });
}

extern "C" {

int clfa_pconv_matrix_create(clfa_pconv_matrix **m, int device, int cvs, int pts, int inputs, int outputs) {
  return create_object(m, [&](clfa_pconv_matrix *p) { return mconv_setup(p, device, cvs, pts, inputs, outputs); });
}

void clfa_pconv_matrix_destroy(clfa_pconv_matrix *p) { destroy_object(p); }

int clfa_pconv_matrix_get_error(const clfa_pconv_matrix *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_pconv_matrix_get_log(const clfa_pconv_matrix *p) { return p ? p->log : ""; }
int clfa_pconv_matrix_nparts(const clfa_pconv_matrix *p) { return p && !p->err ? p->nparts : 0; }
size_t clfa_pconv_matrix_state_bytes(const clfa_pconv_matrix *p) {
  return p ? p->H.bytes + p->ringA.bytes + p->tail.bytes + p->H2.bytes + p->tail2.bytes : 0;
}
size_t clfa_pconv_matrix_workspace_bytes(const clfa_pconv_matrix *p) {
  return p ? p->X.bytes + p->Y.bytes + p->P.bytes + p->tail_ws.bytes + p->Y2.bytes + p->P2.bytes + p->tail_ws2.bytes + p->mix.bytes
           : 0;
}
long clfa_pconv_matrix_fade_remaining(const clfa_pconv_matrix *p) { return p ? p->fade_len - p->fade_done : 0; }
const char *clfa_pconv_matrix_kernel_name(const clfa_pconv_matrix *p) { return !p || p->err ? "" : "k_pconvm_mac"; }

int clfa_pconv_matrix_push_ir_dev(clfa_pconv_matrix *p, const void *ir, long row_stride, void *stream) {
  if (int e = obj_error(p)) return e;
  const long len = (long)p->nparts * p->pts;
  if (!device_rows_ok(ir) || row_stride < len) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: H is one end of it
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  // every partition of every row in one forward launch: row (o, i) partition q -> H frame ((o * inputs + i) * nparts + q)
  const int aligned = rows_aligned8(ir, row_stride);
  HIP_TRY(launch_pconvb_forward(p->logb, (const float *)ir, row_stride, (cpx *)p->H.p, p->nparts, p->nparts,
                                p->outputs * p->inputs, aligned, (const cpx *)p->half.p, (const cpx *)p->w2f.p, s));
  return CLFA_SUCCESS;
}

int clfa_pconv_matrix_push_ir(clfa_pconv_matrix *p, const float *ir) {
  if (int e = obj_error(p)) return e;
  if (!ir) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  return mconv_push_host(p, ir, [&](const void *d, long len) { return clfa_pconv_matrix_push_ir_dev(p, d, len, p->stream); });
}

int clfa_pconv_matrix_push_ir_fade_dev(clfa_pconv_matrix *p, const void *ir, long row_stride, long fade_blocks, void *stream) {
  if (int e = obj_error(p)) return e;
  const long len = (long)p->nparts * p->pts;
  if (!device_rows_ok(ir) || row_stride < len || !fade_blocks_ok(fade_blocks, p->pts)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // one fade at a time
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // everything the fade needs is allocated here, so that no process call allocates because of it: refused under capture
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  int e = mconv_workspaces(p, s);
  if (e) return e;
  if ((e = p->H2.ensure(p->H.bytes)) || (e = p->tail2.ensure(p->tail.bytes)) || (e = p->Y2.ensure(p->Y.bytes)) ||
      (e = p->P2.ensure(p->P.bytes)) || (e = p->tail_ws2.ensure(p->tail_ws.bytes)) ||
      (e = p->mix.ensure(sizeof(float) * (size_t)p->outputs * p->cap * p->pts)))
    return e;
  HIP_TRY(p->order.use(s));
  // the rows' spectra into the second set (as push_ir_dev into H), then that set's tails from the ring
  const int aligned = rows_aligned8(ir, row_stride);
  HIP_TRY(launch_pconvb_forward(p->logb, (const float *)ir, row_stride, (cpx *)p->H2.p, p->nparts, p->nparts,
                                p->outputs * p->inputs, aligned, (const cpx *)p->half.p, (const cpx *)p->w2f.p, s));
  PconvMatrixArgs a = mconv_args(p);
  a.w = p->wp;
  HIP_TRY(launch_pconv_matrix_prime(a, s));
  p->fade_len = fade_blocks;
  p->fade_done = 0;
  return CLFA_SUCCESS;
}

int clfa_pconv_matrix_push_ir_fade(clfa_pconv_matrix *p, const float *ir, long fade_blocks) {
  if (int e = obj_error(p)) return e;
  if (!ir || !fade_blocks_ok(fade_blocks, p->pts)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  return mconv_push_host(p, ir, [&](const void *d, long len) {
    return clfa_pconv_matrix_push_ir_fade_dev(p, d, len, fade_blocks, p->stream);
  });
}

int clfa_pconv_matrix_process_dev(clfa_pconv_matrix *p, void *out, long out_stride, const void *in, long in_stride,
                                  long nblocks, void *stream) {
  if (int e = obj_error(p)) return e;
  const long pts = p->pts, nparts = p->nparts;
  long len;
  if (int e = check_blocks_dev(nblocks, pts, out, out_stride, p->outputs, in, nullptr, in_stride, p->inputs, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // the progress of a fade is host state, which a replay would not advance
  if (p->fade_len && StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  if (int e = mconv_workspaces(p, s)) return e;
  HIP_TRY(p->order.use(s));
  PconvMatrixArgs a = mconv_args(p);
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = rows_aligned8(in, in_stride);
  a.aligned_out = rows_aligned8(out, out_stride);
  const float *src = (const float *)in;
  float *dst = (float *)out;
  for (long j0 = 0; j0 < nblocks; j0 += a.K) {
    // a sub-batch lies wholly inside or wholly outside a fade: cut at the fade's end
    const long fade = p->fade_len - p->fade_done;
    long k = nblocks - j0 < p->cap ? nblocks - j0 : p->cap;
    if (fade && fade < k) k = fade;
    a.K = (int)k;
    a.w = p->wp;
    a.in = src + j0 * pts;
    a.out = dst + j0 * pts;
    if (fade) {
      a.fade_pos = p->fade_done;
      HIP_TRY(launch_pconv_matrix_fade(a, s));
      p->fade_done += k;
    } else {
      HIP_TRY(launch_pconv_matrix(a, s));
    }
    p->wp = (int)((p->wp + a.K) % nparts);
    if (fade == k) {
      // the fade's last block: the second set becomes the first, in place (no address of the object changes)
      p->fade_len = p->fade_done = 0;
      HIP_TRY(hipMemcpyAsync(p->H.p, p->H2.p, p->H.bytes, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(p->tail.p, p->tail2.p, p->tail.bytes, hipMemcpyDeviceToDevice, s));
    }
  }
  return CLFA_SUCCESS;
}

int clfa_pconv_matrix_convolution(clfa_pconv_matrix *p, float *out, const float *in, long nblocks) {
  return blocks_host(p, out, in, nullptr, nblocks, [&](void *o, long len, const void *i1, const void *) {
    return clfa_pconv_matrix_process_dev(p, o, len, i1, len, nblocks, p->stream);
  });
}

}  // extern "C"
