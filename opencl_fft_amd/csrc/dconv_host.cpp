// dconv_host.cpp — C ABI of the direct convolution (see include/clfft_amd.h): Cldconv, one block per call, several
// channels and whole signals per call.  Shared plumbing: conv_host.hpp and, below it, host.hpp.
#include "conv_host.hpp"
#include "dconv_launch.hpp"

using namespace clfa;

struct clfa_dconv {
  DeviceInfo di;
  int irsize = 0, vsize = 0, wp = 0, channels = 1;
  int err = 0;
  hipStream_t stream = nullptr;
  DevBuf del, coefs;   // channels rings of irsize + vsize floats each; one wp for all of them
  DevBuf in1, in2, out;   // staging of the blocking forms (conv_arrays), allocated at creation for one block
  ZeroCopy zc;         // ... zero-copy staging for small blocks (mapped pinned host memory)
  DevBuf part, cnt;    // partial sums per tap chunk and their arrival counter (plan.G > 1)
  DconvPlan plan{64, 1, 1};
  StreamOrder order;
  // many blocks per call (clfa_dconv_process_blocks_dev)
  DconvBlocksPlan bplan;   // tap segments, fixed at creation
  int bcap = 1;            // blocks per sub-batch (CLFA_DCONV_BLOCKS_MAX: tuning switch, read at creation)
  DevBuf bpart;            // the segments' partial sums (bplan.segs > 1): allocated by the first call that needs them
  DevBuf ir;               // staging of push_ir (channels > 1)
};

static BlockShape block_shape(const clfa_dconv *d) { return {d->vsize, d->channels, d->channels}; }
static int dconv_setup(clfa_dconv *d, int device, int irsize, int vsize, int channels) {
  d->irsize = irsize;
  d->vsize = vsize;
  d->channels = channels;
  if (irsize < 1 || vsize < 1 || (long)irsize * vsize > 0x7fffffffL || channels < 1 || channels > 65535) return CLFA_INVALID_VALUE;
  int e = device_info(device, d->di);
  if (e) return e;
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
  const size_t ring = sizeof(float) * ((size_t)irsize + vsize) * (size_t)channels, blk = sizeof(float) * (size_t)vsize;
  d->plan = dconv_plan(irsize, vsize);
  d->bplan = dconv_blocks_plan(irsize);
  // (CLFA_DCONV_BLOCKS_MAX is read per object, like CLFA_PCONV_MATRIX_BLOCKS_MAX)
  // sub-batches bound the segments' workspace; an unsegmented response has none, and its calls are cut only by the switch
  d->bcap = subbatch_cap((long)d->bplan.segs * channels * vsize * (long)sizeof(float), "CLFA_DCONV_BLOCKS_MAX");
  const char *cap_env = getenv("CLFA_DCONV_BLOCKS_MAX");
  if (d->bplan.segs == 1 && !(cap_env && atol(cap_env) > 0)) d->bcap = 0x7fffffff;
  if (const char *env = getenv("CLFA_DCONV_BLOCKS_R")) {   // tuning switch, read per object: outputs per lane, 2 or 8
    if (atoi(env) == 2 || atoi(env) == 8) d->bplan.force_r = atoi(env);
  }
  if ((e = d->del.ensure(ring)) || (e = d->coefs.ensure(ring)) || (e = d->out.ensure(blk)) || (e = d->in1.ensure(blk)) ||
      (e = d->in2.ensure(blk)) || (e = d->part.ensure(blk * d->plan.G)) ||
      (e = d->cnt.ensure(sizeof(unsigned) * d->plan.VB)))
    return e;
  // the reference leaves these uninitialised (cl_dconv.cpp:87-91); zero is the intent
  HIP_TRY(hipMemsetAsync(d->del.p, 0, ring, d->stream));
  HIP_TRY(hipMemsetAsync(d->coefs.p, 0, ring, d->stream));
  HIP_TRY(hipMemsetAsync(d->cnt.p, 0, sizeof(unsigned) * d->plan.VB, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return CLFA_SUCCESS;
}

// one block on stream s, everything device-resident: ring write at wp with wrap-around (intent of cl_dconv.cpp:112-122;
// the two-input form writes in2 into the coefficient ring at the same point, :134-147), wp advanced (:124), vsize
// outputs — all in ONE launch (dconv_block.hip, k_dconv_block)
static int dconv_block(clfa_dconv *d, float *out, const float *in1, const float *in2, hipStream_t s) {
  const int wp = d->wp;
  HIP_TRY(launch_dconv_block(d->plan, out, in1, in2, (float *)d->del.p, (float *)d->coefs.p, (float *)d->part.p,
                             (unsigned *)d->cnt.p, d->irsize, d->vsize, wp, d->di.num_cus, s));
  d->wp = (wp + d->vsize) % (d->irsize + d->vsize);   // committed only once the launch has been accepted
  return CLFA_SUCCESS;
}

static int dconv_host(clfa_dconv *d, float *out, const float *in1, const float *in2) {
  if (int e = obj_error(d)) return e;
  if (!out || !in1) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(d->di.device);
  HIP_TRY(d->order.use(d->stream));
  // an audio block goes zero-copy as the partitioned convolution's host path does (kZeroCopyMaxDconv)
  return block_call(d, kZeroCopyMaxDconv, out, in1, in2, sizeof(float) * (size_t)d->vsize,
                    [&](void *o, const void *i1, const void *i2) {
                      return dconv_block(d, (float *)o, (const float *)i1, (const float *)i2, d->stream);
                    });
}

extern "C" {

int clfa_dconv_create_channels(clfa_dconv **dc, int device, int irsize, int vsize, int channels) {
  return create_object(dc, [&](clfa_dconv *d) { return dconv_setup(d, device, irsize, vsize, channels); });
}

int clfa_dconv_create(clfa_dconv **dc, int device, int irsize, int vsize) {
  return clfa_dconv_create_channels(dc, device, irsize, vsize, 1);
}

void clfa_dconv_destroy(clfa_dconv *d) { destroy_object(d); }

int clfa_dconv_get_error(const clfa_dconv *d) { return d ? d->err : CLFA_INVALID_VALUE; }
int clfa_dconv_channels(const clfa_dconv *d) { return d ? d->channels : 0; }
int clfa_dconv_wp(const clfa_dconv *d) { return d ? d->wp : -1; }
size_t clfa_dconv_state_bytes(const clfa_dconv *d) { return d ? d->del.bytes + d->coefs.bytes : 0; }
size_t clfa_dconv_blocks_workspace_bytes(const clfa_dconv *d) { return d ? d->bpart.bytes : 0; }
const char *clfa_dconv_blocks_kernel_name(const clfa_dconv *d, int time_varying) {
  if (!d || d->err) return "";
  return time_varying ? "loop" : "k_dconvb_fir";
}

int clfa_dconv_push_ir_dev(clfa_dconv *d, const void *ir, long channel_stride, void *stream) {
  if (int e = obj_error(d)) return e;
  if (!device_rows_ok(ir) || channel_stride < d->irsize) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(d->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(d->order.use(s));
  // row c -> the first irsize floats of channel c's coefficient ring
  HIP_TRY(hipMemcpy2DAsync(d->coefs.p, sizeof(float) * ((size_t)d->irsize + d->vsize), ir, sizeof(float) * (size_t)channel_stride,
                           sizeof(float) * (size_t)d->irsize, (size_t)d->channels, hipMemcpyDeviceToDevice, s));
  return CLFA_SUCCESS;
}

int clfa_dconv_push_ir(clfa_dconv *d, const float *ir) {
  if (int e = obj_error(d)) return e;
  if (!ir) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(d->di.device);
  HIP_TRY(d->order.use(d->stream));
  if (d->channels > 1)
    return push_host(d, ir, sizeof(float) * (size_t)d->channels * d->irsize,
                     [&](const void *rows) { return clfa_dconv_push_ir_dev(d, rows, d->irsize, d->stream); });
  // one channel: straight into the coefficient ring
  HIP_TRY(hipMemcpyAsync(d->coefs.p, ir, sizeof(float) * d->irsize, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return CLFA_SUCCESS;
}

int clfa_dconv_process_blocks_dev(clfa_dconv *d, void *out, long out_stride, const void *in1, const void *in2, long in_stride,
                                  long nblocks, void *stream) {
  if (int e = obj_error(d)) return e;
  const long vs = d->vsize, ch = d->channels, end = (long)d->irsize + d->vsize;
  long len;
  if (int e = check_blocks_dev(nblocks, vs, out, out_stride, ch, in1, in2, in_stride, ch, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  ENTER_DEVICE(d->di.device);
  hipStream_t s = (hipStream_t)stream;
  const float *a1 = (const float *)in1, *a2 = (const float *)in2;
  float *o = (float *)out;
  if (a2) {
    // "loop": per block and channel one launch of k_dconv_block on that channel's rings.  The launches are serial on s, so
    // the one part / cnt pair serves every channel.  Correct, not fast.
    HIP_TRY(d->order.use(s));
    for (long j = 0; j < nblocks; j++) {
      for (long c = 0; c < ch; c++)
        HIP_TRY(launch_dconv_block(d->plan, o + c * out_stride + j * vs, a1 + c * in_stride + j * vs, a2 + c * in_stride + j * vs,
                                   (float *)d->del.p + c * end, (float *)d->coefs.p + c * end, (float *)d->part.p,
                                   (unsigned *)d->cnt.p, d->irsize, d->vsize, d->wp, d->di.num_cus, s));
      d->wp = (int)((d->wp + vs) % end);
    }
    return CLFA_SUCCESS;
  }
  const long kmax = nblocks < d->bcap ? nblocks : d->bcap;
  const long part_stride = kmax * vs;
  if (int e = ensure_workspaces({{&d->bpart, d->bplan.segs > 1 ? sizeof(float) * (size_t)d->bplan.segs * ch * part_stride : 0}}, s))
    return e;
  HIP_TRY(d->order.use(s));
  DconvBlocksArgs a;
  a.plan = d->bplan;
  a.irsize = d->irsize;
  a.end = (int)end;
  a.channels = (int)ch;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.del = (float *)d->del.p;
  a.coefs = (const float *)d->coefs.p;
  a.part = (float *)d->bpart.p;
  a.part_stride = part_stride;
  for (long j0 = 0; j0 < nblocks; j0 += kmax) {
    const long k = nblocks - j0 < kmax ? nblocks - j0 : kmax;
    a.L = k * vs;
    a.wp = d->wp;
    a.in1 = a1 + j0 * vs;
    a.out = o + j0 * vs;
    HIP_TRY(launch_dconv_blocks(a, d->di, s));
    d->wp = (int)((d->wp + a.L) % end);
  }
  return CLFA_SUCCESS;
}

int clfa_dconv_convolution_blocks(clfa_dconv *d, float *out, const float *in1, const float *in2, long nblocks) {
  return blocks_host(d, out, in1, in2, nblocks, [&](void *o, long len, const void *i1, const void *i2) {
    return clfa_dconv_process_blocks_dev(d, o, len, i1, i2, len, nblocks, d->stream);
  });
}

// (several channels: one block of each, channels x vsize contiguous floats, is the block call with nblocks = 1)
int clfa_dconv_convolution(clfa_dconv *d, float *out, const float *in) {
  if (d && !d->err && d->channels > 1) return clfa_dconv_convolution_blocks(d, out, in, nullptr, 1);
  return dconv_host(d, out, in, nullptr);
}

int clfa_dconv_convolution_tv(clfa_dconv *d, float *out, const float *in1, const float *in2) {
  if (d && !d->err && !in2) return CLFA_INVALID_VALUE;
  if (d && !d->err && d->channels > 1) return clfa_dconv_convolution_blocks(d, out, in1, in2, 1);
  return dconv_host(d, out, in1, in2);
}

int clfa_dconv_process_dev(clfa_dconv *d, void *out, const void *in1, const void *in2, void *stream) {
  if (int e = obj_error(d)) return e;
  if (d->channels > 1) return clfa_dconv_process_blocks_dev(d, out, d->vsize, in1, in2, d->vsize, 1, stream);
  if (!out || !in1) return CLFA_INVALID_VALUE;
  // the last-arriving workgroup writes out while others may still stage their in1 / in2 windows: no overlap at all
  const size_t blk = sizeof(float) * (size_t)d->vsize;
  if (spans_overlap(out, blk, in1, blk) || (in2 && spans_overlap(out, blk, in2, blk))) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(d->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(d->order.use(s));
  return dconv_block(d, (float *)out, (const float *)in1, (const float *)in2, s);
}

}  // extern "C"
