// conv_host.cpp — C ABI of the convolutions (see include/clfft_amd.h): Clpconv and its multi-block route, Cldconv, the
// convolution matrix, the non-uniformly partitioned convolution and its matrix form.  Shared plumbing: host.hpp, where the staged blocking form lives (staged_call); the rules of a
// call's arrays: overlap.hpp.  Every object stages its blocking calls in members in1, in2, out and its responses in ir.
#include "dconv_launch.hpp"
#include "fft_launch.hpp"
#include "fft_route.hpp"
#include "fft_tables.hpp"
#include "host.hpp"
#include "pconv_launch.hpp"

using namespace clfa;

namespace {

// zero-copy staging of single blocks (mapped pinned host memory)
struct ZeroCopy {
  HostBuf in1, in2, out;
};

// bytes per block up to which the convolutions' blocking host calls go zero-copy: the kernels read the input from, and
// write the output to, mapped pinned host memory (one pass each way), instead of two hipMemcpyAsync calls of 10-15 us
// each around a kernel of a few microseconds
constexpr size_t kZeroCopyMaxConv = (size_t)256 << 10;   // the convolutions' blocks (measured at this size only)
// Cldconv only for blocks of up to 4096 samples: every workgroup whose ring window meets the new block reads it from there
constexpr size_t kZeroCopyMaxDconv = (size_t)16 << 10;

// The arrays of a blocking call of object T, packed, in the order their staging is ensured: in1, out, in2 (ibytes per
// input, a NULL in2 is not used; obytes of output) ...
template <class T>
HostArrays<T, 3> conv_arrays(void *out, size_t obytes, const void *in1, const void *in2, size_t ibytes) {
  return {{{in1, ibytes, 4, false, &T::in1}, {out, obytes, 4, true, &T::out}, {in2, ibytes, 4, false, &T::in2, in2 != nullptr}}};
}
// ... and the staged form around run(out, in1, in2), its one synchronisation the blocking read of cl_conv.cpp:455
template <class T, class Run>
int conv_staged(T *p, const HostArrays<T, 3> &io, Run run) {
  return staged_call(p, io.a, [&](const void *const *d) { return run(const_cast<void *>(d[1]), d[0], d[2]); });
}

// A blocking host call of one audio block (blk bytes per input and output): up to zc_max bytes the kernels read the
// inputs from, and write the output to, mapped pinned host memory — no copy calls, one synchronisation (cl_conv.cpp:399,
// 455); larger blocks take the staged form
template <class T, class Run>
int block_call(T *p, size_t zc_max, float *out, const float *in1, const float *in2, size_t blk, Run run) {
  if (blk > zc_max) return conv_staged(p, conv_arrays<T>(out, blk, in1, in2, blk), run);
  ZeroCopy &z = p->zc;
  int e;
  if ((e = z.in1.ensure(blk)) || (e = z.out.ensure(blk)) || (in2 && (e = z.in2.ensure(blk)))) return e;
  memcpy(z.in1.h, in1, blk);
  if (in2) memcpy(z.in2.h, in2, blk);
  if ((e = run(z.out.d, z.in1.d, in2 ? z.in2.d : nullptr))) return e;
  HIP_TRY(hipStreamSynchronize(p->stream));
  memcpy(out, z.out.h, blk);
  return CLFA_SUCCESS;
}

// tables of the pts-bin transforms of Clpconv and the matrix (cl_conv.cpp:263-287)
int upload_conv_tables(int pts, DevBuf &half, DevBuf &w2f, DevBuf &w2i) {
  int e;
  if ((e = upload_half(half, pts)) || (e = upload_w2(w2f, pts, -1.f)) || (e = upload_w2(w2i, pts, 1.f))) return e;
  return CLFA_SUCCESS;
}

// blocks per multi-block sub-batch: workspaces of per_block bytes per block within ~384 MiB, at most 1024 blocks; the
// tuning switch `env` (read per object) may lower it
int subbatch_cap(long per_block, const char *env_name) {
  long cap = (384L << 20) / per_block;
  const char *env = getenv(env_name);
  if (env && atol(env) > 0 && atol(env) < cap) cap = atol(env);
  return (int)(cap < 1 ? 1 : (cap > 1024 ? 1024 : cap));
}

// rows of floats in device memory, looked at alone: the shared check's NULL and alignment answers
bool device_rows_ok(const void *rows) {
  const CallArray<int> a[] = {{rows, sizeof(float), 4, false, 0}};
  return arrays_ok(a, true);
}

// the count check of a multi-block call: *len = nblocks * pts floats per row, 0 when there is nothing to do
int blocks_len(long nblocks, long pts, long *len) {
  *len = 0;
  if (nblocks < 0 || nblocks > 0x7fffffffL / pts) return CLFA_INVALID_VALUE;
  *len = nblocks * pts;
  return CLFA_SUCCESS;
}

// ... and the checks of a device-resident one: out_rows rows of out and in_rows rows of in1 (and in2, where given), there
// and 4-byte aligned, strides of at least *len floats, out overlapping no input row even partly
int check_blocks_dev(long nblocks, long pts, const void *out, long out_stride, long out_rows, const void *in1,
                     const void *in2, long in_stride, long in_rows, long *len) {
  if (int e = blocks_len(nblocks, pts, len)) return e;
  if (!*len) return CLFA_SUCCESS;
  if (!device_rows_ok(out) || !device_rows_ok(in1) || (in2 && !device_rows_ok(in2))) return CLFA_INVALID_VALUE;
  if (in_stride < *len || out_stride < *len) return CLFA_INVALID_VALUE;
  // Where the two overlap rules meet: the shared description's rule (arrays_ok) takes a strided array as one span, gaps
  // included; the multi-block device forms and the matrix promise more — an output row may lie in the gap between two
  // input rows — so they ask the row-precise rows_overlap instead, and only NULL and alignment of the shared check.
  const long lb = *len * (long)sizeof(float);
  const long osb = out_stride * (long)sizeof(float), isb = in_stride * (long)sizeof(float);
  if (rows_overlap(out, osb, out_rows, in1, isb, in_rows, lb) || (in2 && rows_overlap(out, osb, out_rows, in2, isb, in_rows, lb)))
    return CLFA_INVALID_VALUE;
  return CLFA_SUCCESS;
}

// what a multi-block call of an object moves: nblocks * pts floats in each row (block_shape(p): behind every object)
struct BlockShape {
  long pts, in_rows, out_rows;
};

// The blocking multi-block forms: the object's error, the count, the arrays (there, and the packed output sharing no byte
// with a packed input), then the staged form around dev(out, len, in1, in2), the object's device form on packed rows
template <class T, class Dev>
int blocks_host(T *p, float *out, const float *in1, const float *in2, long nblocks, Dev dev) {
  if (int e = obj_error(p)) return e;
  const BlockShape shape = block_shape(p);
  long len;
  if (int e = blocks_len(nblocks, shape.pts, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  const HostArrays<T, 3> io = conv_arrays<T>(out, sizeof(float) * len * shape.out_rows, in1, in2, sizeof(float) * len * shape.in_rows);
  if (!arrays_ok(io.a, false)) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  return conv_staged(p, io, [&](void *o, const void *i1, const void *i2) { return dev(o, len, i1, i2); });
}

// The blocking pushes of a response: `bytes` of packed rows staged in the object's ir, then push(rows), the device form on
// the object's stream, one synchronisation.  The caller has run its refusals and entered the device.
template <class T, class Push>
int push_host(T *p, const float *ir, size_t bytes, Push push) {
  const HostArray<T> rows[] = {{ir, bytes, 4, false, &T::ir}};
  return staged_call(p, rows, [&](const void *const *d) { return push(d[0]); });
}

}  // namespace

// ---------------------------------------------------------------------------------
// partitioned convolution
// ---------------------------------------------------------------------------------

struct clfa_pconv {
  DeviceInfo di;
  PconvGeom g{};
  int cvs = 0, pts = 0;
  int wp = 0, wp2 = 0;   // cl_conv.cpp:144
  int err = 0;
  hipStream_t stream = nullptr;
  DevBuf half, w2f, w2i;             // tables (cl_conv.cpp:263-287)
  DevBuf ringA, ringB, acc, tail;    // spec1, spec2, in1-as-accumulator, olap tail
  DevBuf in1, in2, out;              // staging of the blocking forms (conv_arrays)
  ZeroCopy zc;                       // ... zero-copy staging for small blocks
  DevBuf ir;                         // ... and for push_ir
  DevBuf four, scratch, work;        // partitions above the LDS sizes: large-N tables, scratch, work frames
  StreamOrder order;
  bool fused = false;                // one launch per block (resolved at creation)
  PconvCoop coop{-1, 1};             // few channels: one cooperative launch per block (logs >= 0)
  DevBuf cnt;                        // ... its arrival counters (one per channel)
  FftTables big;
  // multi-block calls (clfa_pconv_process_blocks_dev): workspaces allocated by the first call that needs them
  int bcap = 1;                      // blocks per sub-batch (CLFA_PCONV_BLOCKS_MAX: tuning switch, read at creation)
  int bkt = 4;                       // outputs per MAC tile
  DevBuf bX, bXB, bY, btail, bstage; // spectra of the new blocks / second inputs, output spectra, new tail; loop staging
};

static BlockShape block_shape(const clfa_pconv *p) { return {p->pts, p->g.channels, p->g.channels}; }
static int pconv_setup(clfa_pconv *p, int device, int cvs, int pts, int channels) {
  p->cvs = cvs;
  p->pts = pts;
  if (!is_pow2(pts) || pts < 2 || pts > (1 << kPconvMaxLogBins) || cvs < pts || channels < 1)
    return CLFA_INVALID_VALUE;
  p->g.bins = pts;                 // cl_conv.cpp:143
  p->g.logb = ilog2(pts);
  p->g.nparts = cvs / pts;         // floor: remainder samples are dropped
  p->g.channels = channels;
  p->wp = 0;
  p->wp2 = p->g.nparts - 1;        // cl_conv.cpp:144
  int e = device_info(device, p->di);
  if (e) return e;
  p->fused = pconv_fused_ok(p->g, p->di) && !getenv("CLFA_PCONV_NO_FUSE");   // tuning switch, read once
  if (!p->fused) p->coop = pconv_coop_plan(p->g, p->di);
  // multi-block sub-batches: the three channels x cap x bins complex workspaces
  // (CLFA_PCONV_BLOCKS_MAX is read per object, like CLFA_PCONV_COOP_MAX_KB)
  p->bcap = subbatch_cap(3L * channels * pts * (long)sizeof(cpx), "CLFA_PCONV_BLOCKS_MAX");
  p->bkt = pconv_blocks_tile(p->g, p->di);
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  if ((e = upload_conv_tables(pts, p->half, p->w2f, p->w2i))) return e;
  if (p->g.logb > kLdsMaxLog) {
    const int n = pts;
    std::vector<cpx> all;
    fill_fourstep_tables(all, p->g.logb);
    if ((e = upload(p->four, all.data(), sizeof(cpx) * all.size()))) return e;
    p->big.four = (const cpx *)p->four.p;
    if ((e = p->scratch.ensure((size_t)fourstep_grid(p->di) * n * sizeof(cpx)))) return e;
    if ((e = p->work.ensure(sizeof(cpx) * (size_t)channels * n))) return e;
  }
  const size_t ring = sizeof(cpx) * (size_t)channels * p->g.nparts * pts;
  const size_t blk = sizeof(float) * (size_t)channels * pts;
  if ((e = p->ringA.ensure(ring))) return e;
  if ((e = p->ringB.ensure(ring))) return e;
  const int acc_copies = p->coop.logs >= 0 ? p->coop.sparts : pconv_mac_split(p->g);
  if ((e = p->acc.ensure(sizeof(cpx) * (size_t)channels * pts * acc_copies))) return e;
  if ((e = p->tail.ensure(blk))) return e;
  if (p->coop.logs >= 0) {
    if ((e = p->cnt.ensure(sizeof(unsigned) * (size_t)channels))) return e;
    HIP_TRY(hipMemsetAsync(p->cnt.p, 0, sizeof(unsigned) * (size_t)channels, p->stream));
  }
  // zero-initialised state (cl_conv.cpp:303-313)
  HIP_TRY(hipMemsetAsync(p->ringA.p, 0, ring, p->stream));
  HIP_TRY(hipMemsetAsync(p->ringB.p, 0, ring, p->stream));
  HIP_TRY(hipMemsetAsync(p->tail.p, 0, blk, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

// forward chain of one block for all channels: in -> spectrum frame `frame` of `ring`
static int pconv_forward(clfa_pconv *p, const float *in, long in_stride, cpx *ring, int frame, hipStream_t s) {
  if (p->g.logb <= kLdsMaxLog) {
    HIP_TRY(launch_pconv_forward(p->g, in, in_stride, ring, frame, (const cpx *)p->half.p, (const cpx *)p->w2f.p, s));
    return CLFA_SUCCESS;
  }
  // composed: zero-pad -> large-N forward FFT (unscaled) -> reference r2c -> place the frames in the ring
  const int bins = p->g.bins, ch = p->g.channels;
  cpx *work = (cpx *)p->work.p;
  HIP_TRY(launch_pconv_pad(in, in_stride, work, bins, ch, s));
  HIP_TRY(launch_fft_4step(p->g.logb, true, false, work, (cpx *)p->scratch.p, p->big, ch, p->di, s));
  HIP_TRY(launch_r2c_pack(work, (const cpx *)p->w2f.p, bins, ch, s));
  HIP_TRY(hipMemcpy2DAsync(ring + (size_t)frame * bins, sizeof(cpx) * (size_t)p->g.nparts * bins, work,
                           sizeof(cpx) * (size_t)bins, sizeof(cpx) * (size_t)bins, ch, hipMemcpyDeviceToDevice, s));
  return CLFA_SUCCESS;
}

// inverse chain: accumulator -> c2r -> inverse FFT -> overlap-add
static int pconv_inverse(clfa_pconv *p, float *out, hipStream_t s) {
  if (p->g.logb <= kLdsMaxLog) {
    HIP_TRY(launch_pconv_inverse(p->g, (const cpx *)p->acc.p, (float *)p->tail.p, out, (const cpx *)p->half.p,
                                 (const cpx *)p->w2i.p, s));
    return CLFA_SUCCESS;
  }
  const int bins = p->g.bins, ch = p->g.channels;
  cpx *acc = (cpx *)p->acc.p;
  HIP_TRY(launch_c2r_unpack(acc, (const cpx *)p->w2i.p, bins, ch, s));
  HIP_TRY(launch_fft_4step(p->g.logb, false, false, acc, (cpx *)p->scratch.p, p->big, ch, p->di, s));
  HIP_TRY(launch_pconv_olap((const float *)acc, (float *)p->tail.p, out, bins, ch, s));
  return CLFA_SUCCESS;
}

static bool pconv_blocks_looped(const clfa_pconv *p) {
  return p->g.logb < kPconvBlocksMinLog || p->g.logb > kPconvBlocksMaxLog;
}

extern "C" {

int clfa_pconv_create(clfa_pconv **pc, int device, int cvs, int pts, int channels) {
  return create_object(pc, [&](clfa_pconv *p) { return pconv_setup(p, device, cvs, pts, channels); });
}

void clfa_pconv_destroy(clfa_pconv *p) { destroy_object(p); }

int clfa_pconv_get_error(const clfa_pconv *p) { return p ? p->err : CLFA_INVALID_VALUE; }
int clfa_pconv_nparts(const clfa_pconv *p) { return p ? p->g.nparts : 0; }
int clfa_pconv_wp(const clfa_pconv *p) { return p ? p->wp : -1; }
int clfa_pconv_wp2(const clfa_pconv *p) { return p ? p->wp2 : -1; }
const char *clfa_pconv_kernel_name(const clfa_pconv *p) {
  if (!p || p->err) return "";
  return p->fused ? "k_pconv_fused" : (p->coop.logs >= 0 ? "k_pconv_coop" : "chain");
}
size_t clfa_pconv_state_bytes(const clfa_pconv *p) {
  return p ? p->ringA.bytes + p->ringB.bytes + p->acc.bytes + p->tail.bytes : 0;
}

int clfa_pconv_push_ir_dev(clfa_pconv *p, const void *ir, long channel_stride, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!ir || channel_stride < (long)p->g.nparts * p->pts) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  const long stride = channel_stride;
  // cl_conv.cpp:358-386: partition i -> frame wp2, wp2 counts down from nparts-1
  for (int i = 0; i < p->g.nparts; i++) {
    int e = pconv_forward(p, (const float *)ir + (long)i * p->pts, stride, (cpx *)p->ringB.p, p->wp2, s);
    if (e) return e;
    p->wp2 = p->wp2 == 0 ? p->g.nparts - 1 : p->wp2 - 1;
  }
  return CLFA_SUCCESS;
}

int clfa_pconv_push_ir(clfa_pconv *p, const float *ir) {
  if (int e = obj_error(p)) return e;
  if (!ir) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  const long len = (long)p->g.nparts * p->pts;
  return push_host(p, ir, sizeof(float) * (size_t)p->g.channels * len,
                   [&](const void *rows) { return clfa_pconv_push_ir_dev(p, rows, len, p->stream); });
}

int clfa_pconv_process_dev(clfa_pconv *p, void *out, const void *in1, const void *in2, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!out || !in1) return CLFA_INVALID_VALUE;
  if (p->fused || p->coop.logs >= 0) {
    // the one-launch routes read the inputs of ALL channels while workgroups of other channels may already write their
    // output (the buffers are __restrict__): any overlap of out with an input — not only equal pointers — is refused.
    // (The launch chain below has read every input when its forward launch ends, before the inverse launch writes `out`:
    // in place is fine there, as it was for the reference's host arrays.)
    const size_t blk = sizeof(float) * (size_t)p->pts * (size_t)p->g.channels;
    if (spans_overlap(out, blk, in1, blk) || (in2 && spans_overlap(out, blk, in2, blk))) return CLFA_INVALID_VALUE;
  }
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  int e;
  if (p->fused || p->coop.logs >= 0) {
    // whole block in one launch; ring indices advance exactly as below — committed only once the launch has been accepted
    // (a rejected launch must not skew the host's ring position against the device's rings)
    const int frame1 = p->wp, frame2 = p->wp2;
    const int wp_next = p->wp != p->g.nparts - 1 ? p->wp + 1 : 0;
    const int wp2_next = in2 ? (p->wp2 == 0 ? p->g.nparts - 1 : p->wp2 - 1) : p->wp2;
    if (!p->fused) {
      HIP_TRY(launch_pconv_coop(p->g, p->coop, (const float *)in1, (const float *)in2, (cpx *)p->ringA.p,
                                (cpx *)p->ringB.p, (float *)p->tail.p, (float *)out, frame1, frame2, wp_next,
                                (const cpx *)p->half.p, (const cpx *)p->w2f.p, (const cpx *)p->w2i.p, (cpx *)p->acc.p,
                                (unsigned *)p->cnt.p, p->di.num_cus, s));
    } else {
      HIP_TRY(launch_pconv_fused(p->g, (const float *)in1, (const float *)in2, (cpx *)p->ringA.p, (cpx *)p->ringB.p,
                                 (float *)p->tail.p, (float *)out, frame1, frame2, wp_next, (const cpx *)p->half.p,
                                 (const cpx *)p->w2f.p, (const cpx *)p->w2i.p, s, p->g.channels < p->di.num_cus));
    }
    p->wp = wp_next;
    p->wp2 = wp2_next;
    return CLFA_SUCCESS;
  }
  const bool lds = p->g.logb <= kLdsMaxLog;
  // forward chain(s): cl_conv.cpp:399-419 / 465-513 (both inputs of a time-varying block in one launch)
  if (lds && in2) {
    HIP_TRY(launch_pconv_forward(p->g, (const float *)in1, p->pts, (cpx *)p->ringA.p, p->wp, (const cpx *)p->half.p,
                                 (const cpx *)p->w2f.p, s, (const float *)in2, (cpx *)p->ringB.p, p->wp2));
  } else {
    if ((e = pconv_forward(p, (const float *)in1, p->pts, (cpx *)p->ringA.p, p->wp, s))) return e;
    if (in2 && (e = pconv_forward(p, (const float *)in2, p->pts, (cpx *)p->ringB.p, p->wp2, s))) return e;
  }
  p->wp = p->wp != p->g.nparts - 1 ? p->wp + 1 : 0;            // cl_conv.cpp:424 / 516
  if (in2) p->wp2 = p->wp2 == 0 ? p->g.nparts - 1 : p->wp2 - 1;  // cl_conv.cpp:519
  // cl_conv.cpp:428-449.  (Adding the partial sums of a split MAC inside the single-workgroup inverse kernel
  // instead of the wide k_pconv_reduce launch was measured: 22 -> 130 us per block for one channel.)
  HIP_TRY(launch_pconv_mac(p->g, (const cpx *)p->ringA.p, (const cpx *)p->ringB.p, p->wp, (cpx *)p->acc.p, s));
  if ((e = pconv_inverse(p, (float *)out, s))) return e;
  return CLFA_SUCCESS;
}

static int pconv_host(clfa_pconv *p, float *out, const float *in1, const float *in2) {
  if (int e = obj_error(p)) return e;
  if (!out || !in1) return CLFA_INVALID_VALUE;
  ENTER_DEVICE(p->di.device);
  // one audio block of a few channels goes zero-copy
  return block_call(p, kZeroCopyMaxConv, out, in1, in2, sizeof(float) * (size_t)p->g.channels * p->pts,
                    [&](void *o, const void *i1, const void *i2) { return clfa_pconv_process_dev(p, o, i1, i2, p->stream); });
}

int clfa_pconv_convolution(clfa_pconv *p, float *out, const float *in) { return pconv_host(p, out, in, nullptr); }
int clfa_pconv_convolution_tv(clfa_pconv *p, float *out, const float *in1, const float *in2) {
  if (!in2) return CLFA_INVALID_VALUE;
  return pconv_host(p, out, in1, in2);
}

// ---- many blocks per call -------------------------------------------------------

const char *clfa_pconv_blocks_kernel_name(const clfa_pconv *p) {
  if (!p || p->err) return "";
  return pconv_blocks_looped(p) ? "loop" : "k_pconvb_mac";
}

size_t clfa_pconv_blocks_workspace_bytes(const clfa_pconv *p) {
  return p ? p->bX.bytes + p->bXB.bytes + p->bY.bytes + p->btail.bytes + p->bstage.bytes : 0;
}

int clfa_pconv_process_blocks_dev(clfa_pconv *p, void *out, long out_stride, const void *in1, const void *in2,
                                  long in_stride, long nblocks, void *stream) {
  if (int e = obj_error(p)) return e;
  const long pts = p->pts, ch = p->g.channels, nparts = p->g.nparts;
  long len;
  if (int e = check_blocks_dev(nblocks, pts, out, out_stride, ch, in1, in2, in_stride, ch, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  const size_t frames = sizeof(cpx) * (size_t)ch * (size_t)p->bcap * (size_t)pts;
  int e = pconv_blocks_looped(p)
              ? ensure_workspaces({{&p->bstage, sizeof(float) * (size_t)ch * (size_t)pts * 3}}, s)
              : ensure_workspaces({{&p->bX, frames}, {&p->bY, frames}, {&p->btail, sizeof(float) * (size_t)ch * (size_t)pts},
                                   {&p->bXB, in2 ? frames : 0}}, s);
  if (e) return e;
  HIP_TRY(p->order.use(s));
  const float *a1 = (const float *)in1, *a2 = (const float *)in2;
  float *o = (float *)out;
  if (pconv_blocks_looped(p)) {
    // partitions outside the LDS transform sizes: block by block through clfa_pconv_process_dev, each block gathered into
    // contiguous channels x pts staging (any alignment and stride) and scattered back
    float *st1 = (float *)p->bstage.p, *st2 = st1 + ch * pts, *sto = st2 + ch * pts;
    const size_t row = sizeof(float) * (size_t)pts;
    const size_t isb = sizeof(float) * (size_t)in_stride, osb = sizeof(float) * (size_t)out_stride;
    for (long j = 0; j < nblocks; j++) {
      HIP_TRY(hipMemcpy2DAsync(st1, row, a1 + j * pts, isb, row, (size_t)ch, hipMemcpyDeviceToDevice, s));
      if (a2) HIP_TRY(hipMemcpy2DAsync(st2, row, a2 + j * pts, isb, row, (size_t)ch, hipMemcpyDeviceToDevice, s));
      if ((e = clfa_pconv_process_dev(p, sto, st1, a2 ? st2 : nullptr, stream))) return e;
      HIP_TRY(hipMemcpy2DAsync(o + j * pts, osb, sto, row, row, (size_t)ch, hipMemcpyDeviceToDevice, s));
    }
    return CLFA_SUCCESS;
  }
  PconvBlocks a;
  a.g = p->g;
  a.cap = p->bcap;
  a.kt = p->bkt;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = ((uintptr_t)in1 & 7) == 0 && (!in2 || ((uintptr_t)in2 & 7) == 0) && (in_stride & 1) == 0;
  a.aligned_out = ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0;
  a.ringA = (cpx *)p->ringA.p;
  a.ringB = (cpx *)p->ringB.p;
  a.tail = (float *)p->tail.p;
  a.X = (cpx *)p->bX.p;
  a.XB = (cpx *)p->bXB.p;
  a.Y = (cpx *)p->bY.p;
  a.tail_ws = (float *)p->btail.p;
  a.half = (const cpx *)p->half.p;
  a.w2f = (const cpx *)p->w2f.p;
  a.w2i = (const cpx *)p->w2i.p;
  // time-varying sub-batches stay within nparts blocks: each second-input ring frame then changes at most once
  const long kmax = in2 && nparts < p->bcap ? nparts : p->bcap;
  for (long j0 = 0; j0 < nblocks; j0 += kmax) {
    a.K = (int)(nblocks - j0 < kmax ? nblocks - j0 : kmax);
    a.w = p->wp;
    a.w2 = p->wp2;
    a.in1 = a1 + j0 * pts;
    a.in2 = a2 ? a2 + j0 * pts : nullptr;
    a.out = o + j0 * pts;
    HIP_TRY(launch_pconv_blocks(a, s));
    p->wp = (int)((p->wp + a.K) % nparts);
    if (a2) p->wp2 = (int)(((p->wp2 - a.K) % nparts + nparts) % nparts);
  }
  return CLFA_SUCCESS;
}

int clfa_pconv_convolution_blocks(clfa_pconv *p, float *out, const float *in1, const float *in2, long nblocks) {
  return blocks_host(p, out, in1, in2, nblocks, [&](void *o, long len, const void *i1, const void *i2) {
    return clfa_pconv_process_blocks_dev(p, o, len, i1, i2, len, nblocks, p->stream);
  });
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// direct convolution
// ---------------------------------------------------------------------------------

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

// ---------------------------------------------------------------------------------
// convolution matrix (pconv_matrix.hip)
// ---------------------------------------------------------------------------------

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
  PconvMatrixArgs a;
  a.logb = p->logb;
  a.bins = p->pts;
  a.nparts = p->nparts;
  a.inputs = p->inputs;
  a.outputs = p->outputs;
  a.plan = p->plan;
  a.cap = p->cap;
  a.H = (const cpx *)p->H.p;
  a.ringA = (cpx *)p->ringA.p;
  a.tail = (float *)p->tail.p;
  a.X = (cpx *)p->X.p;
  a.Y = (cpx *)p->Y.p;
  a.P = (cpx *)p->P.p;
  a.tail_ws = (float *)p->tail_ws.p;
  a.half = (const cpx *)p->half.p;
  a.w2f = (const cpx *)p->w2f.p;
  a.w2i = (const cpx *)p->w2i.p;
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
  const int aligned = ((uintptr_t)ir & 7) == 0 && (row_stride & 1) == 0;
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
  if (!device_rows_ok(ir) || row_stride < len || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts)
    return CLFA_INVALID_VALUE;
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
  const int aligned = ((uintptr_t)ir & 7) == 0 && (row_stride & 1) == 0;
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
  if (!ir || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts) return CLFA_INVALID_VALUE;
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
  a.aligned_in = ((uintptr_t)in & 7) == 0 && (in_stride & 1) == 0;
  a.aligned_out = ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0;
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

// ---------------------------------------------------------------------------------
// non-uniformly partitioned convolution (pconv_nup.hip; the head is the blocks route of pconv_blocks.hip)
// ---------------------------------------------------------------------------------

// one level: its geometry, tables, input-spectra ring (`ring` frames: the tail keeps two more than its sum walks, the
// history from which a fade push recomputes the second path), ring position
struct NupLevel {
  PconvGeom g{};
  int ring = 0;
  DevBuf half, w2f, w2i;
  DevBuf ringA;
  int w = 0;
};

// what depends on the responses: both levels' spectra of them, the levels' overlap-add tails (a single block's inverse
// reads one and writes the other; hcur / tcur: the one in force), the finished tail block's samples, being mixed in, and
// the tail block's accumulators, filled slice by slice.  A fade runs two of these over the shared rings
struct NupSet {
  DevBuf ringB[2];
  DevBuf tail0[2], tail1[2];
  int hcur = 0, tcur = 0;
  DevBuf pend, Y1;
  size_t state_bytes() const {
    return ringB[0].bytes + ringB[1].bytes + tail0[0].bytes + tail0[1].bytes + tail1[0].bytes + tail1[1].bytes + pend.bytes;
  }
  hipError_t clear_history(hipStream_t s) {   // (the responses stay)
    for (DevBuf *b : {&tail0[0], &tail0[1], &tail1[0], &tail1[1], &pend})
      if (hipError_t e = hipMemsetAsync(b->p, 0, b->bytes, s)) return e;
    hcur = tcur = 0;
    return hipSuccess;
  }
};

struct clfa_nupconv {
  DeviceInfo di;
  int cvs = 0, pts0 = 0, pts1 = 0, m = 0, channels = 0;
  int err = 0;
  char log[256];
  hipStream_t stream = nullptr;
  NupLevel lv[2];                // the head (2m partitions of pts0) and the tail (n1 partitions of pts1)
  NupSet sets[2];                // sets[cur]: the responses in force and their path.  sets[cur ^ 1]: the second path of a
  int cur = 0;                   // timed crossfade (push_ir_fade), allocated by the first fade push and kept; it becomes
                                 // the first, on the host, when the fade's last block is issued
  NupSet &first() { return sets[cur]; }
  NupSet &second() { return sets[cur ^ 1]; }
  DevBuf stage;                  // the tail block being collected
  DevBuf stage2;                 // ... and the second input's (allocated by the first time-varying call)
  int tv_count = 0;              // time-varying blocks among the head blocks of the tail block being collected
  DevBuf Y0;                    // a single head block's accumulators (a single block's X is its ring frame w)
  DevBuf Y0b, headb;             // a fade: the second path's head accumulators and head samples (channels x pts0)
  long fade_len = 0, fade_done = 0;   // head blocks of the pending fade (0: none) and how many of them have been processed
  DevBuf bX, bY, btail;          // the head's sub-batch workspaces, for hcap blocks (grown by the call that needs more)
  DevBuf bXB;                    // ... and the second input's spectra, for hcap2 blocks (time-varying calls of several blocks)
  int hcap = 0, hcap2 = 0, bcap = 1, bkt = 4;
  DevBuf in1, in2, out;          // staging of the blocking forms (conv_arrays; in2: the time-varying second input)
  DevBuf ir;                     // ... and of push_ir
  StreamOrder order;
  long c = 0;                    // head blocks since creation / reset
};

static BlockShape block_shape(const clfa_nupconv *p) { return {p->pts0, p->channels, p->channels}; }
static long nup_ir_len(const clfa_nupconv *p) { return 2L * p->pts1 + (long)p->lv[1].g.nparts * p->pts1; }

// a set's buffers (kept once they exist)
static int nup_alloc_set(const clfa_nupconv *p, NupSet &b) {
  const size_t ch = (size_t)p->channels;
  int e;
  for (int i = 0; i < 2; i++)
    if ((e = b.ringB[i].ensure(sizeof(cpx) * ch * p->lv[i].g.nparts * p->lv[i].g.bins)) ||
        (e = b.tail0[i].ensure(sizeof(float) * ch * p->pts0)) || (e = b.tail1[i].ensure(sizeof(float) * ch * p->pts1)))
      return e;
  if ((e = b.pend.ensure(sizeof(float) * ch * p->pts1)) || (e = b.Y1.ensure(sizeof(cpx) * ch * p->pts1))) return e;
  return CLFA_SUCCESS;
}

static int nup_setup(clfa_nupconv *p, int device, int cvs, int pts0, int pts1, int channels) {
  p->log[0] = 0;
  p->cvs = cvs;
  p->pts0 = pts0;
  p->pts1 = pts1;
  p->channels = channels;
  const int lo = 1 << kPconvBlocksMinLog, hi = 1 << kPconvBlocksMaxLog;
  if (!is_pow2(pts0) || pts0 < lo) {
    snprintf(p->log, sizeof(p->log), "pts0 must be a power of two, %d..%d (got %d)", lo, hi / 2, pts0);
    return CLFA_INVALID_VALUE;
  }
  if (!is_pow2(pts1) || pts1 > hi || pts1 <= pts0) {
    snprintf(p->log, sizeof(p->log), "pts1 must be a power of two above pts0, at most %d (got pts0 %d, pts1 %d)", hi, pts0, pts1);
    return CLFA_INVALID_VALUE;
  }
  if (cvs / 3 < pts1) {
    snprintf(p->log, sizeof(p->log), "cvs must be at least 3 * pts1 = %d (got %d)", 3 * pts1, cvs);
    return CLFA_INVALID_VALUE;
  }
  if (channels < 1) {
    snprintf(p->log, sizeof(p->log), "channels must be at least 1 (got %d)", channels);
    return CLFA_INVALID_VALUE;
  }
  p->m = pts1 / pts0;
  p->lv[0].g = {ilog2(pts0), pts0, 2 * p->m, channels};
  p->lv[1].g = {ilog2(pts1), pts1, (cvs - 2 * pts1) / pts1, channels};   // floor: remainder samples are dropped
  p->lv[0].ring = p->lv[0].g.nparts;
  p->lv[1].ring = p->lv[1].g.nparts + 2;
  int e = device_info(device, p->di);
  if (e) return e;
  p->bcap = subbatch_cap(3L * channels * pts0 * (long)sizeof(cpx), "CLFA_PCONV_BLOCKS_MAX");   // as Clpconv's blocks route
  p->bkt = pconv_blocks_tile(p->lv[0].g, p->di);
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  for (NupLevel &l : p->lv) {
    if ((e = upload_conv_tables(l.g.bins, l.half, l.w2f, l.w2i))) return e;
    if ((e = l.ringA.ensure(sizeof(cpx) * (size_t)channels * l.ring * l.g.bins))) return e;
    HIP_TRY(hipMemsetAsync(l.ringA.p, 0, l.ringA.bytes, p->stream));
  }
  NupSet &a = p->first();
  if ((e = nup_alloc_set(p, a)) || (e = p->stage.ensure(sizeof(float) * (size_t)channels * pts1)) ||
      (e = p->Y0.ensure(sizeof(cpx) * (size_t)channels * pts0)))
    return e;
  for (DevBuf *b : {&a.ringB[0], &a.ringB[1], &p->stage}) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes, p->stream));
  HIP_TRY(a.clear_history(p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

// partition i of every row -> response frame nparts - 1 - i of the level (the frame the MAC pairs with the i-th newest
// input block), with the blocks route's forward transform: the bits Clpconv's push gives
static int nup_push_level(const NupLevel &l, const DevBuf &ringB, const float *ir, long stride, hipStream_t s) {
  const int aligned = ((uintptr_t)ir & 7) == 0 && (stride & 1) == 0;
  for (int i = 0; i < l.g.nparts; i++)
    HIP_TRY(launch_pconvb_forward(l.g.logb, ir + (long)i * l.g.bins, stride, (cpx *)ringB.p + (long)(l.g.nparts - 1 - i) * l.g.bins,
                                  1, l.g.nparts, l.g.channels, aligned, (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  return CLFA_SUCCESS;
}

// the head's K blocks through the blocks route, sub-batch by sub-batch, as clfa_pconv_process_blocks_dev.  in2: the blocks
// are time-varying ones at positions pos, pos + 1, ... < n0 of their response period, the time-varying blocks route: block
// j's second input becomes response frame n0 - 1 - (pos + j) for itself and the blocks after it
static int nup_head(clfa_nupconv *p, float *out, long out_stride, const float *in, long in_stride, long nblocks, hipStream_t s,
                    const float *in2 = nullptr, long in2_stride = 0, long pos = 0) {
  NupLevel &l = p->lv[0];
  NupSet &set = p->first();
  PconvBlocks a;
  a.g = l.g;
  a.cap = p->hcap;
  a.kt = p->bkt;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = ((uintptr_t)in & 7) == 0 && (in_stride & 1) == 0;
  a.aligned_out = ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0;
  a.ringA = (cpx *)l.ringA.p;
  a.ringB = (cpx *)set.ringB[0].p;
  a.tail = (float *)set.tail0[set.hcur].p;
  a.X = (cpx *)p->bX.p;
  a.Y = (cpx *)p->bY.p;
  a.tail_ws = (float *)p->btail.p;
  a.half = (const cpx *)l.half.p;
  a.w2f = (const cpx *)l.w2f.p;
  a.w2i = (const cpx *)l.w2i.p;
  a.XB = (cpx *)p->bXB.p;
  a.in2_stride = in2_stride;
  a.aligned_in2 = ((uintptr_t)in2 & 7) == 0 && (in2_stride & 1) == 0;
  for (long j0 = 0; j0 < nblocks; j0 += a.K) {
    a.K = (int)(nblocks - j0 < p->hcap ? nblocks - j0 : p->hcap);
    a.w = l.w;
    a.in1 = in + j0 * p->pts0;
    a.in2 = in2 ? in2 + j0 * p->pts0 : nullptr;
    a.w2 = (int)(l.g.nparts - 1 - (pos + j0));
    a.out = out + j0 * p->pts0;
    HIP_TRY(launch_pconv_blocks(a, s));
    l.w = (int)((l.w + a.K) % l.g.nparts);
  }
  return CLFA_SUCCESS;
}

// h[0 : 2*pts1) in the head's partitions, h[2*pts1 : 2*pts1 + n1*pts1) in the tail's, in stream order
static int nup_push_levels(const clfa_nupconv *p, const DevBuf &ringB0, const DevBuf &ringB1, const float *ir, long stride,
                           hipStream_t s) {
  if (int e = nup_push_level(p->lv[0], ringB0, ir, stride, s)) return e;
  return nup_push_level(p->lv[1], ringB1, ir + 2L * p->pts1, stride, s);
}

// one block of a level, single-block route.  forward: its samples -> ring frame w (committing it is the caller's w + 1)
static int nup_forward(const NupLevel &l, const float *in, long in_stride, hipStream_t s) {
  HIP_TRY(launch_pconvb_forward(l.g.logb, in, in_stride, (cpx *)l.ringA.p + (long)l.w * l.g.bins, 1, l.ring, l.g.channels,
                                ((uintptr_t)in & 7) == 0 && (in_stride & 1) == 0, (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  return CLFA_SUCCESS;
}
// ... the multiply-accumulate of items [item0, item0 + nitems) of the block in frame w under the responses ringB, into Y
static NupcMacJob nup_job(const NupLevel &l, const DevBuf &ringB, const DevBuf &Y, int w, int item0, int nitems) {
  return {(const cpx *)l.ringA.p, (const cpx *)ringB.p, (cpx *)Y.p, w, l.g.bins, l.g.nparts, l.ring, item0, nitems};
}
// ... inverse transform and overlap-add: Y and the tail in force -> out, the other tail, which comes into force
static int nup_inverse(const NupLevel &l, const DevBuf &Y, DevBuf (&tails)[2], int &cur, float *out, long out_stride, hipStream_t s) {
  HIP_TRY(launch_pconvb_inverse(l.g.logb, (const cpx *)Y.p, (const float *)tails[cur].p, (float *)tails[cur ^ 1].p, out, out_stride, 1, 1,
                                1, l.g.channels, ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0, (const cpx *)l.half.p,
                                (const cpx *)l.w2i.p, s));
  cur ^= 1;
  return CLFA_SUCCESS;
}

// The time-varying second input (clfft_amd.h), step 1, asked at phase 0 of period P >= 1: the response frame of the tail
// level that the second input's finished tail block U = P - 1 rewrites, or -1 where it rewrites none — one of its m head
// blocks was a plain block, or it lies in the two head-covered tail blocks of its response period
static int nup_tv_frame(const clfa_nupconv *p) {
  const int n1 = p->lv[1].g.nparts;
  const long r = (p->c / p->m - 1) % (n1 + 2);
  return p->tv_count == p->m && r >= 2 ? n1 - 1 - (int)(r - 2) : -1;
}
// ... carried out by a plain block: the second stage row -> that frame of the set in force, push_ir's transform
static int nup_tv_commit(clfa_nupconv *p, hipStream_t s) {
  const NupLevel &t = p->lv[1];
  const int fr = nup_tv_frame(p);
  if (fr >= 0)
    HIP_TRY(launch_pconvb_forward(t.g.logb, (const float *)p->stage2.p, p->pts1, (cpx *)p->first().ringB[1].p + (long)fr * t.g.bins, 1,
                                  t.g.nparts, t.g.channels, 1, (const cpx *)t.half.p, (const cpx *)t.w2f.p, s));
  return CLFA_SUCCESS;
}

// nblocks >= 1 blocks outside a fade.  One block: the head's forward transform straight into its ring frame, its
// multiply-accumulate beside the tail's slice in one launch of k_nupc_mac, its inverse.  Several blocks: the head through
// the blocks route over the whole call.  The arithmetic of a bin is the same on both ways, and both leave the same rings,
// tails and positions.  x2 (or NULL): the blocks are time-varying ones, a stretch that lies on one side of a = n0 in its
// response period — their second input is staged beside x, and before a = n0 the head takes the time-varying blocks route.
static int nup_blocks(clfa_nupconv *p, float *o, long out_stride, const float *x, long in_stride, long nblocks, hipStream_t s,
                      const float *x2 = nullptr, long in2_stride = 0) {
  const long pts0 = p->pts0, m = p->m;
  const int ch = p->channels;
  const bool single = nblocks == 1;
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &a = p->first();
  if (!single) {
    const long pos = p->c % ((long)(t.g.nparts + 2) * m);
    const bool tv = x2 && pos < h.g.nparts;
    if (int e = nup_head(p, o, out_stride, x, in_stride, nblocks, s, tv ? x2 : nullptr, in2_stride, pos)) return e;
  }
  // the tail, period by period: head blocks [j0, j0 + k) of the call are phases [sa, sb) of period P, in which tail block
  // P - 1 is multiplied and tail block P - 2 is heard
  const int hb0 = (int)(pts0 / 2);
  for (long j0 = 0; j0 < nblocks;) {
    const long P = p->c / m;
    const int sa = (int)(p->c % m);
    const long k = nblocks - j0 < m - sa ? nblocks - j0 : m - sa;
    const int sb = sa + (int)k, off = sa * (int)pts0, n = (int)(k * pts0);
    if (single)
      if (int e = nup_forward(h, x, in_stride, s)) return e;
    // phase 0: the spectrum of the finished block, before this period's samples overwrite the row
    if (P >= 1 && sa == 0) {
      if (int e = nup_forward(t, (const float *)p->stage.p, p->pts1, s)) return e;
      if (int e = nup_tv_commit(p, s)) return e;
    }
    if (sa == 0) p->tv_count = 0;
    if (x2) {
      HIP_TRY(launch_nupc_stage2(x + j0 * pts0, in_stride, (float *)p->stage.p, x2 + j0 * pts0, in2_stride, (float *)p->stage2.p,
                                 p->pts1, off, n, ch, s));
      p->tv_count += (int)k;
    } else {
      HIP_TRY(launch_nupc_stage(x + j0 * pts0, in_stride, (float *)p->stage.p, p->pts1, off, n, ch, s));
    }
    NupcMacJob jobs[2];
    int njobs = 0;
    if (single) jobs[njobs++] = nup_job(h, a.ringB[0], p->Y0, h.w, 0, hb0);
    if (P >= 1) jobs[njobs++] = nup_job(t, a.ringB[1], a.Y1, t.w, sa * hb0, (sb - sa) * hb0);
    if (njobs) HIP_TRY(launch_nupc_mac(jobs, njobs, ch, s));
    if (single) {
      if (int e = nup_inverse(h, p->Y0, a.tail0, a.hcur, o, out_stride, s)) return e;
      h.w = (h.w + 1) % h.ring;
    }
    HIP_TRY(launch_nupc_mix(o + j0 * pts0, out_stride, (const float *)a.pend.p, p->pts1, off, n, ch, s));
    // after slice m - 1: the block's samples replace the ones just heard, its spectrum stays in the ring
    if (P >= 1 && sb == m) {
      if (int e = nup_inverse(t, a.Y1, a.tail1, a.tcur, (float *)a.pend.p, p->pts1, s)) return e;
      t.w = (t.w + 1) % t.ring;
    }
    p->c += k;
    j0 += k;
  }
  return CLFA_SUCCESS;
}

// One time-varying block (clfft_amd.h: the four steps), in one launch fewer than a plain block: k_nupc_fwd transforms both
// inputs of a level in one launch and files the samples it loads in the stage rows.  At phase 0 the tail level's launch
// goes first — it reads the stage rows that the head level's launch then overwrites: the finished block of x into the
// input ring and, where step 1 applies, the second input's into its response frame.  The head level's launch: x into
// ring frame w, the second input's block into response frame n0 - 1 - a where a = c mod R0 < n0 (otherwise that job only
// copies).  The rest is the plain block's.
static int nup_tv_block(clfa_nupconv *p, float *o, long out_stride, const float *x, long in_stride, const float *x2, long in2_stride,
                        hipStream_t s) {
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &a = p->first();
  const int ch = p->channels, pts0 = p->pts0, m = p->m, hb0 = pts0 / 2, n0 = h.g.nparts;
  const long P = p->c / m, R0 = (long)(t.g.nparts + 2) * m, pos = p->c % R0;
  const int sa = (int)(p->c % m), off = sa * pts0;
  const auto rows8 = [](const void *q, long stride) { return ((uintptr_t)q & 7) == 0 && (stride & 1) == 0; };
  if (P >= 1 && sa == 0) {
    NupcFwdJob jobs[2];
    int njobs = 0;
    jobs[njobs++] = {(const float *)p->stage.p, p->pts1, 1, (cpx *)t.ringA.p + (long)t.w * t.g.bins, t.ring, nullptr, 0};
    const int fr = nup_tv_frame(p);
    if (fr >= 0) jobs[njobs++] = {(const float *)p->stage2.p, p->pts1, 1, (cpx *)a.ringB[1].p + (long)fr * t.g.bins, t.g.nparts, nullptr, 0};
    HIP_TRY(launch_nupc_fwd(t.g.logb, jobs, njobs, ch, (const cpx *)t.half.p, (const cpx *)t.w2f.p, s));
  }
  if (sa == 0) p->tv_count = 0;
  const NupcFwdJob jobs0[2] = {
      {x, in_stride, rows8(x, in_stride), (cpx *)h.ringA.p + (long)h.w * pts0, h.ring, (float *)p->stage.p + off, p->pts1},
      {x2, in2_stride, rows8(x2, in2_stride), pos < n0 ? (cpx *)a.ringB[0].p + (long)(n0 - 1 - pos) * pts0 : nullptr, n0,
       (float *)p->stage2.p + off, p->pts1}};
  HIP_TRY(launch_nupc_fwd(h.g.logb, jobs0, 2, ch, (const cpx *)h.half.p, (const cpx *)h.w2f.p, s));
  p->tv_count++;
  NupcMacJob jobs[2];
  int njobs = 0;
  jobs[njobs++] = nup_job(h, a.ringB[0], p->Y0, h.w, 0, hb0);
  if (P >= 1) jobs[njobs++] = nup_job(t, a.ringB[1], a.Y1, t.w, sa * hb0, hb0);
  HIP_TRY(launch_nupc_mac(jobs, njobs, ch, s));
  if (int e = nup_inverse(h, p->Y0, a.tail0, a.hcur, o, out_stride, s)) return e;
  h.w = (h.w + 1) % h.ring;
  HIP_TRY(launch_nupc_mix(o, out_stride, (const float *)a.pend.p, p->pts1, off, pts0, ch, s));
  if (P >= 1 && sa == m - 1) {
    if (int e = nup_inverse(t, a.Y1, a.tail1, a.tcur, (float *)a.pend.p, p->pts1, s)) return e;
    t.w = (t.w + 1) % t.ring;
  }
  p->c++;
  return CLFA_SUCCESS;
}

// nblocks >= 1 time-varying blocks outside a fade, cut at a = c mod R0 = n0 and at the response period's end: the blocks
// with a in [0, n0) rewrite a head partition each, the head's time-varying blocks route; the others, a in [n0, R0), are a
// static stretch for the head.  A stretch of one block is the single time-varying block.
static int nup_tv_blocks(clfa_nupconv *p, float *o, long out_stride, const float *x, long in_stride, const float *x2, long in2_stride,
                         long nblocks, hipStream_t s) {
  const long pts0 = p->pts0, n0 = p->lv[0].g.nparts, R0 = (long)(p->lv[1].g.nparts + 2) * p->m;
  for (long j = 0; j < nblocks;) {
    const long pos = p->c % R0;
    const long end = pos < n0 ? n0 : R0, k = nblocks - j < end - pos ? nblocks - j : end - pos;
    if (int e = k == 1 ? nup_tv_block(p, o + j * pts0, out_stride, x + j * pts0, in_stride, x2 + j * pts0, in2_stride, s)
                       : nup_blocks(p, o + j * pts0, out_stride, x + j * pts0, in_stride, k, s, x2 + j * pts0, in2_stride))
      return e;
    j += k;
  }
  return CLFA_SUCCESS;
}

// the head's sub-batch workspaces for a call of `rest` blocks through the blocks route; tv: the second input's as well
static int nup_ensure_head(clfa_nupconv *p, long rest, hipStream_t s, bool tv = false) {
  const size_t ch = (size_t)p->channels, pts0 = (size_t)p->pts0;
  if (rest > 1 && rest > p->hcap) {
    const int cap = (int)(rest < p->bcap ? rest : p->bcap);
    if (cap > p->hcap) {
      const size_t frames = sizeof(cpx) * ch * (size_t)cap * pts0;
      if (int e = ensure_workspaces({{&p->bX, frames}, {&p->bY, frames}, {&p->btail, sizeof(float) * ch * pts0}}, s)) return e;
      p->hcap = cap;
    }
  }
  // (the frames of a channel lie hcap frames apart in every workspace of the sub-batch)
  if (tv && p->hcap2 < p->hcap) {
    if (int e = ensure_workspaces({{&p->bXB, sizeof(cpx) * ch * (size_t)p->hcap * pts0}}, s)) return e;
    p->hcap2 = p->hcap;
  }
  return CLFA_SUCCESS;
}

// One head block of a fade, on the single-block route with every response-dependent step run for both sets over the
// shared rings: the four multiply-accumulates are one launch, the first path's head goes to the output rows and the
// second's to headb, and k_nupc_fade_mix forms both paths' head + pending sums and a + g * (b - a).  After the fade's last
// block the second set becomes the first (nothing is copied; the object is not capturable, so no address has to stay
// fixed).
static int nup_fade_block(clfa_nupconv *p, float *o, long out_stride, const float *x, long in_stride, hipStream_t s) {
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &a = p->first(), &b = p->second();
  const int ch = p->channels, pts0 = p->pts0, m = p->m, hb0 = pts0 / 2;
  const long P = p->c / m;
  const int sa = (int)(p->c % m), off = sa * pts0;
  if (int e = nup_forward(h, x, in_stride, s)) return e;
  if (P >= 1 && sa == 0) {
    if (int e = nup_forward(t, (const float *)p->stage.p, p->pts1, s)) return e;
    if (int e = nup_tv_commit(p, s)) return e;   // (time-varying blocks before the fade push: into the set in force)
  }
  if (sa == 0) p->tv_count = 0;
  HIP_TRY(launch_nupc_stage(x, in_stride, (float *)p->stage.p, p->pts1, off, pts0, ch, s));
  NupcMacJob jobs[kNupcMacJobs];
  int njobs = 0;
  jobs[njobs++] = nup_job(h, a.ringB[0], p->Y0, h.w, 0, hb0);
  jobs[njobs++] = nup_job(h, b.ringB[0], p->Y0b, h.w, 0, hb0);
  if (P >= 1) {
    jobs[njobs++] = nup_job(t, a.ringB[1], a.Y1, t.w, sa * hb0, hb0);
    jobs[njobs++] = nup_job(t, b.ringB[1], b.Y1, t.w, sa * hb0, hb0);
  }
  HIP_TRY(launch_nupc_mac(jobs, njobs, ch, s));
  int e;
  if ((e = nup_inverse(h, p->Y0, a.tail0, a.hcur, o, out_stride, s)) ||
      (e = nup_inverse(h, p->Y0b, b.tail0, b.hcur, (float *)p->headb.p, pts0, s)))
    return e;
  h.w = (h.w + 1) % h.ring;
  HIP_TRY(launch_nupc_fade_mix(o, out_stride, (const float *)p->headb.p, (const float *)a.pend.p, (const float *)b.pend.p, p->pts1,
                               off, pts0, ch, p->fade_done * pts0, (float)(p->fade_len * pts0), s));
  if (P >= 1 && sa == m - 1) {
    if ((e = nup_inverse(t, a.Y1, a.tail1, a.tcur, (float *)a.pend.p, p->pts1, s)) ||
        (e = nup_inverse(t, b.Y1, b.tail1, b.tcur, (float *)b.pend.p, p->pts1, s)))
      return e;
    t.w = (t.w + 1) % t.ring;
  }
  p->c++;
  if (++p->fade_done == p->fade_len) {
    p->cur ^= 1;
    p->fade_len = p->fade_done = 0;
  }
  return CLFA_SUCCESS;
}

// The second set's history at position c = P * m + sa, recomputed under its responses from the rings alone with the plain
// path's kernels, hence with its bits: the head's tail from head block c - 1; the tail level's tail, pending row and tail
// again from tail blocks P - 3 and P - 2 (whole blocks in one multiply-accumulate: a bin's sum does not depend on how the
// bins are cut into slices); slices [0, sa) of tail block P - 1, in progress.  A block of negative index is not computed:
// what it would have left is the +0 the rows are cleared to.  Tail block P - 3 reads back to input block P - 2 - n1, which
// is why the tail's ring keeps n1 + 2 frames.
static int nup_prime(clfa_nupconv *p, hipStream_t s) {
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &b = p->second();
  const int ch = p->channels, hb0 = p->pts0 / 2;
  const long P = p->c / p->m;
  const int sa = (int)(p->c % p->m);
  HIP_TRY(b.clear_history(s));
  const auto back = [](const NupLevel &l, int k) { return (l.w - k + l.ring) % l.ring; };   // the frame k blocks before frame w
  // a whole block of level l in frame w: multiply-accumulate, inverse (the samples: to `out`)
  const auto block = [&](const NupLevel &l, const DevBuf &ringB, const DevBuf &Y, int w, DevBuf (&tails)[2], int &cur, float *out) {
    const NupcMacJob job = nup_job(l, ringB, Y, w, 0, l.g.bins / 2);
    HIP_TRY(launch_nupc_mac(&job, 1, ch, s));
    return nup_inverse(l, Y, tails, cur, out, l.g.bins, s);
  };
  int e;
  if (p->c >= 1 && (e = block(h, b.ringB[0], p->Y0b, back(h, 1), b.tail0, b.hcur, (float *)p->headb.p))) return e;
  if (P >= 3 && (e = block(t, b.ringB[1], b.Y1, back(t, 2), b.tail1, b.tcur, (float *)b.pend.p))) return e;
  if (P >= 2 && (e = block(t, b.ringB[1], b.Y1, back(t, 1), b.tail1, b.tcur, (float *)b.pend.p))) return e;
  if (P >= 1 && sa > 0) {
    const NupcMacJob job = nup_job(t, b.ringB[1], b.Y1, t.w, 0, sa * hb0);
    HIP_TRY(launch_nupc_mac(&job, 1, ch, s));
  }
  return CLFA_SUCCESS;
}

extern "C" {

int clfa_nupconv_create(clfa_nupconv **pc, int device, int cvs, int pts0, int pts1, int channels) {
  return create_object(pc, [&](clfa_nupconv *p) { return nup_setup(p, device, cvs, pts0, pts1, channels); });
}

void clfa_nupconv_destroy(clfa_nupconv *p) { destroy_object(p); }

int clfa_nupconv_get_error(const clfa_nupconv *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_nupconv_get_log(const clfa_nupconv *p) { return p ? p->log : ""; }
int clfa_nupconv_nparts(const clfa_nupconv *p, int level) {
  return p && !p->err && (level == 0 || level == 1) ? p->lv[level].g.nparts : 0;
}
long clfa_nupconv_position(const clfa_nupconv *p) { return p ? p->c : 0; }
size_t clfa_nupconv_state_bytes(const clfa_nupconv *p) {
  if (!p) return 0;
  return p->lv[0].ringA.bytes + p->lv[1].ringA.bytes + p->stage.bytes + p->stage2.bytes + p->sets[0].state_bytes() +
         p->sets[1].state_bytes();
}
size_t clfa_nupconv_workspace_bytes(const clfa_nupconv *p) {
  return p ? p->Y0.bytes + p->sets[0].Y1.bytes + p->sets[1].Y1.bytes + p->Y0b.bytes + p->headb.bytes + p->bX.bytes + p->bY.bytes +
                 p->btail.bytes + p->bXB.bytes
           : 0;
}
long clfa_nupconv_fade_remaining(const clfa_nupconv *p) { return p ? p->fade_len - p->fade_done : 0; }
const char *clfa_nupconv_kernel_name(const clfa_nupconv *p) { return !p || p->err ? "" : "k_nupc_mac"; }

int clfa_nupconv_push_ir_dev(clfa_nupconv *p, const void *ir, long channel_stride, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || channel_stride < nup_ir_len(p)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: the responses are one end of it
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  return nup_push_levels(p, p->first().ringB[0], p->first().ringB[1], (const float *)ir, channel_stride, s);
}

int clfa_nupconv_push_ir(clfa_nupconv *p, const float *ir) {
  if (int e = obj_error(p)) return e;
  if (!ir) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const long len = nup_ir_len(p);
  return push_host(p, ir, sizeof(float) * (size_t)p->channels * len,
                   [&](const void *rows) { return clfa_nupconv_push_ir_dev(p, rows, len, p->stream); });
}

int clfa_nupconv_push_ir_fade_dev(clfa_nupconv *p, const void *ir, long channel_stride, long fade_blocks, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || channel_stride < nup_ir_len(p) || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts0)
    return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // one fade at a time
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // everything the fade needs is allocated here, so that no process call allocates because of it: refused under capture
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  NupSet &b = p->second();
  int e;
  if ((e = nup_alloc_set(p, b)) || (e = p->Y0b.ensure(p->Y0.bytes)) || (e = p->headb.ensure(sizeof(float) * (size_t)p->channels * p->pts0)))
    return e;
  HIP_TRY(p->order.use(s));
  // the rows' spectra into the second set (as push_ir_dev into the first), then that set's history from the rings
  if ((e = nup_push_levels(p, b.ringB[0], b.ringB[1], (const float *)ir, channel_stride, s)) || (e = nup_prime(p, s))) return e;
  p->fade_len = fade_blocks;
  p->fade_done = 0;
  return CLFA_SUCCESS;
}

int clfa_nupconv_push_ir_fade(clfa_nupconv *p, const float *ir, long fade_blocks) {
  if (int e = obj_error(p)) return e;
  if (!ir || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts0) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const long len = nup_ir_len(p);
  return push_host(p, ir, sizeof(float) * (size_t)p->channels * len,
                   [&](const void *rows) { return clfa_nupconv_push_ir_fade_dev(p, rows, len, fade_blocks, p->stream); });
}

int clfa_nupconv_process_dev(clfa_nupconv *p, void *out, long out_stride, const void *in, long in_stride, long nblocks,
                             void *stream) {
  if (int e = obj_error(p)) return e;
  const long pts0 = p->pts0, ch = p->channels;
  long len;
  if (int e = check_blocks_dev(nblocks, pts0, out, out_stride, ch, in, nullptr, in_stride, ch, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // the phase of the schedule (and the progress of a fade) is host state, which a replay would not advance
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  // a fade's blocks run one at a time; what follows the fade in the same call takes the usual route
  const long fade = p->fade_len - p->fade_done, nf = nblocks < fade ? nblocks : fade, rest = nblocks - nf;
  if (int e = nup_ensure_head(p, rest, s)) return e;
  HIP_TRY(p->order.use(s));
  const float *x = (const float *)in;
  float *o = (float *)out;
  for (long j = 0; j < nf; j++)
    if (int e = nup_fade_block(p, o + j * pts0, out_stride, x + j * pts0, in_stride, s)) return e;
  return rest ? nup_blocks(p, o + nf * pts0, out_stride, x + nf * pts0, in_stride, rest, s) : CLFA_SUCCESS;
}

int clfa_nupconv_convolution(clfa_nupconv *p, float *out, const float *in, long nblocks) {
  return blocks_host(p, out, in, nullptr, nblocks, [&](void *o, long len, const void *i1, const void *) {
    return clfa_nupconv_process_dev(p, o, len, i1, len, nblocks, p->stream);
  });
}

long clfa_nupconv_tv_period(const clfa_nupconv *p) { return p && !p->err ? (long)(p->lv[1].g.nparts + 2) * p->m : 0; }

int clfa_nupconv_process_tv_dev(clfa_nupconv *p, void *out, long out_stride, const void *in, long in_stride, const void *in2,
                                long in2_stride, long nblocks, void *stream) {
  if (!in2) return clfa_nupconv_process_dev(p, out, out_stride, in, in_stride, nblocks, stream);
  if (int e = obj_error(p)) return e;
  const long pts0 = p->pts0, ch = p->channels;
  long len;
  if (int e = check_blocks_dev(nblocks, pts0, out, out_stride, ch, in, nullptr, in_stride, ch, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  // the second input's rows: their own stride, and no byte shared with an output row (the inputs may share theirs)
  if (!device_rows_ok(in2) || in2_stride < len) return CLFA_INVALID_VALUE;
  const long sf = (long)sizeof(float);
  if (rows_overlap(out, out_stride * sf, ch, in2, in2_stride * sf, ch, len * sf)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: which set would the blocks rewrite
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;   // (as process_dev)
  const bool first = !p->stage2.p;
  if (int e = p->stage2.ensure(p->stage.bytes)) return e;
  // the longest stretch that takes the blocks route: the n0 head-rewriting blocks of a response period, or the others
  const long n0 = p->lv[0].g.nparts, stat = clfa_nupconv_tv_period(p) - n0, longest = stat > n0 ? stat : n0;
  if (int e = nup_ensure_head(p, nblocks < longest ? nblocks : longest, s, true)) return e;
  HIP_TRY(p->order.use(s));
  if (first) HIP_TRY(hipMemsetAsync(p->stage2.p, 0, p->stage2.bytes, s));
  return nup_tv_blocks(p, (float *)out, out_stride, (const float *)in, in_stride, (const float *)in2, in2_stride, nblocks, s);
}

int clfa_nupconv_convolution_tv(clfa_nupconv *p, float *out, const float *in, const float *in2, long nblocks) {
  return blocks_host(p, out, in, in2, nblocks, [&](void *o, long len, const void *i1, const void *i2) {
    return clfa_nupconv_process_tv_dev(p, o, len, i1, len, i2, len, nblocks, p->stream);
  });
}

int clfa_nupconv_reset(clfa_nupconv *p, void *stream) {
  if (int e = obj_error(p)) return e;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: finish it first
  HIP_TRY(p->order.use(s));
  // the input history, the tails and the blocks in progress; the responses stay
  for (NupLevel &l : p->lv) {
    HIP_TRY(hipMemsetAsync(l.ringA.p, 0, l.ringA.bytes, s));
    l.w = 0;
  }
  HIP_TRY(hipMemsetAsync(p->stage.p, 0, p->stage.bytes, s));
  // the second input's block in progress and how much of it is there
  if (p->stage2.p) HIP_TRY(hipMemsetAsync(p->stage2.p, 0, p->stage2.bytes, s));
  p->tv_count = 0;
  HIP_TRY(p->first().clear_history(s));
  p->c = 0;
  return CLFA_SUCCESS;
}

}  // extern "C"

// ---------------------------------------------------------------------------------
// non-uniformly partitioned convolution matrix (pconv_nupm.hip; a head of many blocks is launch_pconv_matrix)
// ---------------------------------------------------------------------------------

// one level: its geometry, tables, segments, the inputs' spectra ring (`ring` frames per input, the matrix's layout: the
// head's nparts, which launch_pconv_matrix runs over; the tail keeps two more than its sum walks, the history from which
// a fade push recomputes the second path), ring position
struct NupmLevel {
  int logb = 0, bins = 0, nparts = 0, ring = 0, segs = 1;
  DevBuf half, w2f, w2i;
  DevBuf ringA;
  int w = 0;
};

// what depends on the responses, per level [0] / [1]: the outputs x inputs response spectra, the outputs' overlap-add
// tails (a single block's inverse reads one and writes the other; hcur / tcur: the one in force), a single block's
// accumulators and partial sums; and the finished tail block's samples, being mixed in (outputs x pts1).  A fade runs two
// of these over the shared rings
struct NupmSet {
  DevBuf H[2];
  DevBuf tail0[2], tail1[2];
  int hcur = 0, tcur = 0;
  DevBuf pend;
  DevBuf Y[2], P[2];
  size_t state_bytes() const {
    return H[0].bytes + H[1].bytes + tail0[0].bytes + tail0[1].bytes + tail1[0].bytes + tail1[1].bytes + pend.bytes;
  }
  size_t workspace_bytes() const { return Y[0].bytes + Y[1].bytes + P[0].bytes + P[1].bytes; }
  hipError_t clear_history(hipStream_t s) {   // (the responses stay)
    for (DevBuf *b : {&tail0[0], &tail0[1], &tail1[0], &tail1[1], &pend})
      if (hipError_t e = hipMemsetAsync(b->p, 0, b->bytes, s)) return e;
    hcur = tcur = 0;
    return hipSuccess;
  }
};

struct clfa_nupconv_matrix {
  DeviceInfo di;
  int cvs = 0, pts0 = 0, pts1 = 0, m = 0, inputs = 0, outputs = 0;
  int err = 0;
  char log[256];
  hipStream_t stream = nullptr;
  NupmLevel lv[2];               // the head (2m partitions of pts0) and the tail (n1 partitions of pts1)
  NupmSet sets[2];               // sets[cur]: the responses in force and their path.  sets[cur ^ 1]: the second path of a
  int cur = 0;                   // timed crossfade (push_ir_fade), allocated by the first fade push and kept; it becomes
                                 // the first, on the host, when the fade's last block is issued
  NupmSet &first() { return sets[cur]; }
  NupmSet &second() { return sets[cur ^ 1]; }
  DevBuf stage;                  // the tail block being collected (inputs x pts1)
  DevBuf headb;                  // a fade: the second path's head samples (outputs x pts0)
  long fade_len = 0, fade_done = 0;   // head blocks of the pending fade (0: none) and how many of them have been processed
  DevBuf bX, bY, bP, btail;      // the head's sub-batch workspaces, for hcap blocks (grown by the call that needs more)
  int hcap = 0, bcap = 1, bkt = 4;
  DevBuf in1, in2, out;          // staging of the blocking form (conv_arrays; in2 stays empty)
  DevBuf ir;                     // ... and of push_ir
  StreamOrder order;
  long c = 0;                    // head blocks since creation / reset
};

static BlockShape block_shape(const clfa_nupconv_matrix *p) { return {p->pts0, p->inputs, p->outputs}; }
static long nupm_ir_len(const clfa_nupconv_matrix *p) { return 2L * p->pts1 + (long)p->lv[1].nparts * p->pts1; }

// a set's buffers (kept once they exist)
static int nupm_alloc_set(const clfa_nupconv_matrix *p, NupmSet &b) {
  const size_t outs = (size_t)p->outputs;
  int e;
  for (int k = 0; k < 2; k++) {
    const NupmLevel &l = p->lv[k];
    const size_t frame = sizeof(cpx) * (size_t)l.bins;
    if ((e = b.H[k].ensure(frame * outs * p->inputs * l.nparts)) || (e = b.Y[k].ensure(frame * outs)) ||
        (l.segs > 1 && (e = b.P[k].ensure(frame * outs * (size_t)(l.segs - 1)))) ||
        (e = b.tail0[k].ensure(sizeof(float) * outs * p->pts0)) || (e = b.tail1[k].ensure(sizeof(float) * outs * p->pts1)))
      return e;
  }
  return b.pend.ensure(sizeof(float) * outs * p->pts1);
}

static int nupm_setup(clfa_nupconv_matrix *p, int device, int cvs, int pts0, int pts1, int inputs, int outputs) {
  p->log[0] = 0;
  p->cvs = cvs;
  p->pts0 = pts0;
  p->pts1 = pts1;
  p->inputs = inputs;
  p->outputs = outputs;
  const int lo = 1 << kPconvBlocksMinLog, hi = 1 << kPconvBlocksMaxLog;
  if (!is_pow2(pts0) || pts0 < lo) {
    snprintf(p->log, sizeof(p->log), "pts0 must be a power of two, %d..%d (got %d)", lo, hi / 2, pts0);
    return CLFA_INVALID_VALUE;
  }
  if (!is_pow2(pts1) || pts1 > hi || pts1 <= pts0) {
    snprintf(p->log, sizeof(p->log), "pts1 must be a power of two above pts0, at most %d (got pts0 %d, pts1 %d)", hi, pts0, pts1);
    return CLFA_INVALID_VALUE;
  }
  if (cvs / 3 < pts1) {
    snprintf(p->log, sizeof(p->log), "cvs must be at least 3 * pts1 = %d (got %d)", 3 * pts1, cvs);
    return CLFA_INVALID_VALUE;
  }
  if (inputs < 1) {
    snprintf(p->log, sizeof(p->log), "inputs must be at least 1 (got %d)", inputs);
    return CLFA_INVALID_VALUE;
  }
  if (outputs < 1) {
    snprintf(p->log, sizeof(p->log), "outputs must be at least 1 (got %d)", outputs);
    return CLFA_INVALID_VALUE;
  }
  p->m = pts1 / pts0;
  NupmLevel &h = p->lv[0], &t = p->lv[1];
  h.logb = ilog2(pts0), h.bins = pts0, h.nparts = 2 * p->m;
  t.logb = ilog2(pts1), t.bins = pts1, t.nparts = (cvs - 2 * pts1) / pts1;   // floor: remainder samples are dropped
  h.ring = h.nparts;
  t.ring = t.nparts + 2;
  int e = device_info(device, p->di);
  if (e) return e;
  // each level's segments: the matrix's plan and its tuning switch, as mconv_setup — for the head at its geometry, for the
  // tail at the geometry of a SLICE (pts0 bins of n1 partitions): a single-block call offers the multiply-accumulate
  // pts0 / 2 items per output, not pts1 / 2, and with the whole block's count 64 x 64 at 64 / 4096 ran one segment of 3968
  // terms on 32 waves (896 us per block against 160 for Nupconv on expanded inputs; profiles/HISTORY.md)
  for (NupmLevel &l : p->lv) {
    const PconvMatrixPlan pl = pconv_matrix_plan(pts0, l.nparts, inputs, outputs, p->di);
    l.segs = pl.segs;
    if (&l == &h) p->bkt = pl.kt;
    if (const char *env = getenv("CLFA_PCONV_MATRIX_SEGS")) {
      if (atoi(env) >= 1 && atoi(env) <= 4096) l.segs = atoi(env);
    }
  }
  p->bcap = subbatch_cap(((long)inputs + (long)outputs * h.segs) * pts0 * (long)sizeof(cpx), "CLFA_PCONV_MATRIX_BLOCKS_MAX");
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  for (NupmLevel &l : p->lv) {
    if ((e = upload_conv_tables(l.bins, l.half, l.w2f, l.w2i))) return e;
    if ((e = l.ringA.ensure(sizeof(cpx) * (size_t)l.bins * inputs * l.ring))) return e;
    HIP_TRY(hipMemsetAsync(l.ringA.p, 0, l.ringA.bytes, p->stream));
  }
  NupmSet &a = p->first();
  if ((e = nupm_alloc_set(p, a)) || (e = p->stage.ensure(sizeof(float) * (size_t)inputs * pts1))) return e;
  for (DevBuf *b : {&a.H[0], &a.H[1], &p->stage}) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes, p->stream));
  HIP_TRY(a.clear_history(p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

// every partition of every row into a set's response spectra, one forward launch per level, as
// clfa_pconv_matrix_push_ir_dev: row (o, i) partition q -> H frame ((o * inputs + i) * nparts + q); h[0 : 2*pts1) in the
// head's partitions, what follows in the tail's
static int nupm_push_levels(const clfa_nupconv_matrix *p, const NupmSet &set, const float *rows, long row_stride, hipStream_t s) {
  for (int k = 0; k < 2; k++) {
    const NupmLevel &l = p->lv[k];
    const float *src = rows + (k ? 2L * p->pts1 : 0);
    const int aligned = ((uintptr_t)src & 7) == 0 && (row_stride & 1) == 0;
    HIP_TRY(launch_pconvb_forward(l.logb, src, row_stride, (cpx *)set.H[k].p, l.nparts, l.nparts, p->outputs * p->inputs, aligned,
                                  (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  }
  return CLFA_SUCCESS;
}

// one block of a level, single-block route.  forward: the inputs' samples -> ring frame w (committing it is the caller's
// w + 1)
static int nupm_forward(const clfa_nupconv_matrix *p, const NupmLevel &l, const float *in, long in_stride, hipStream_t s) {
  HIP_TRY(launch_pconvb_forward(l.logb, in, in_stride, (cpx *)l.ringA.p + (long)l.w * l.bins, 1, l.ring, p->inputs,
                                ((uintptr_t)in & 7) == 0 && (in_stride & 1) == 0, (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  return CLFA_SUCCESS;
}
// ... the multiply-accumulate of items [item0, item0 + nitems) of level k's block in frame w under the set's responses,
// into the set's accumulators
static NupmMacJob nupm_job(const clfa_nupconv_matrix *p, int k, const NupmSet &set, int w, int item0, int nitems) {
  const NupmLevel &l = p->lv[k];
  return {(const cpx *)l.ringA.p, (const cpx *)set.H[k].p, (cpx *)set.Y[k].p, (cpx *)set.P[k].p, w, l.bins, l.nparts, l.ring, l.segs,
          item0, nitems};
}
// ... inverse transform and overlap-add: Y and the tail in force -> out, the other tail, which comes into force
static int nupm_inverse(const clfa_nupconv_matrix *p, int k, NupmSet &set, float *out, long out_stride, hipStream_t s) {
  const NupmLevel &l = p->lv[k];
  DevBuf(&tails)[2] = k ? set.tail1 : set.tail0;
  int &cur = k ? set.tcur : set.hcur;
  HIP_TRY(launch_pconvb_inverse(l.logb, (const cpx *)set.Y[k].p, (const float *)tails[cur].p, (float *)tails[cur ^ 1].p, out, out_stride,
                                1, 1, 1, p->outputs, ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0, (const cpx *)l.half.p,
                                (const cpx *)l.w2i.p, s));
  cur ^= 1;
  return CLFA_SUCCESS;
}

// the head's K blocks through the matrix's sub-batch launches, sub-batch by sub-batch, as clfa_pconv_matrix_process_dev
static int nupm_head(clfa_nupconv_matrix *p, float *out, long out_stride, const float *in, long in_stride, long nblocks, hipStream_t s) {
  NupmLevel &l = p->lv[0];
  NupmSet &set = p->first();
  PconvMatrixArgs a;
  a.logb = l.logb;
  a.bins = l.bins;
  a.nparts = l.nparts;
  a.inputs = p->inputs;
  a.outputs = p->outputs;
  a.plan.kt = p->bkt;
  a.plan.segs = l.segs;
  a.cap = p->hcap;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = ((uintptr_t)in & 7) == 0 && (in_stride & 1) == 0;
  a.aligned_out = ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0;
  a.H = (const cpx *)set.H[0].p;
  a.ringA = (cpx *)l.ringA.p;
  a.tail = (float *)set.tail0[set.hcur].p;
  a.X = (cpx *)p->bX.p;
  a.Y = (cpx *)p->bY.p;
  a.P = (cpx *)p->bP.p;
  a.tail_ws = (float *)p->btail.p;
  a.half = (const cpx *)l.half.p;
  a.w2f = (const cpx *)l.w2f.p;
  a.w2i = (const cpx *)l.w2i.p;
  for (long j0 = 0; j0 < nblocks; j0 += a.K) {
    a.K = (int)(nblocks - j0 < p->hcap ? nblocks - j0 : p->hcap);
    a.w = l.w;
    a.in = in + j0 * p->pts0;
    a.out = out + j0 * p->pts0;
    HIP_TRY(launch_pconv_matrix(a, s));
    l.w = (int)((l.w + a.K) % l.nparts);
  }
  return CLFA_SUCCESS;
}

// nblocks >= 1 blocks outside a fade.  One block: the head's forward transform straight into its ring frame, its
// multiply-accumulate beside the tail's slice in one launch of k_nupm_mac, the segments' sums, its inverse.  Several
// blocks: the head through the matrix's launches over the whole call, the tail's slices between two period boundaries in
// one launch.  The arithmetic of a bin is the same on both ways, and both leave the same rings, tails and positions.
static int nupm_blocks(clfa_nupconv_matrix *p, float *o, long out_stride, const float *x, long in_stride, long nblocks, hipStream_t s) {
  const long pts0 = p->pts0, m = p->m;
  const bool single = nblocks == 1;
  NupmLevel &h = p->lv[0], &t = p->lv[1];
  NupmSet &a = p->first();
  if (!single)
    if (int e = nupm_head(p, o, out_stride, x, in_stride, nblocks, s)) return e;
  // the tail, period by period: head blocks [j0, j0 + k) of the call are phases [sa, sb) of period P, in which tail block
  // P - 1 is multiplied and tail block P - 2 is heard
  const int hb0 = (int)(pts0 / 2);
  for (long j0 = 0; j0 < nblocks;) {
    const long P = p->c / m;
    const int sa = (int)(p->c % m);
    const long k = nblocks - j0 < m - sa ? nblocks - j0 : m - sa;
    const int sb = sa + (int)k, off = sa * (int)pts0, n = (int)(k * pts0);
    if (single)
      if (int e = nupm_forward(p, h, x, in_stride, s)) return e;
    // phase 0: the spectra of the finished block, before this period's samples overwrite the rows
    if (P >= 1 && sa == 0)
      if (int e = nupm_forward(p, t, (const float *)p->stage.p, p->pts1, s)) return e;
    HIP_TRY(launch_nupc_stage(x + j0 * pts0, in_stride, (float *)p->stage.p, p->pts1, off, n, p->inputs, s));
    NupmMacJob jobs[kNupmMacJobs];
    int njobs = 0;
    if (single) jobs[njobs++] = nupm_job(p, 0, a, h.w, 0, hb0);
    if (P >= 1) jobs[njobs++] = nupm_job(p, 1, a, t.w, sa * hb0, (sb - sa) * hb0);
    if (njobs) {
      HIP_TRY(launch_nupm_mac(jobs, njobs, p->inputs, p->outputs, s));
      HIP_TRY(launch_nupm_reduce(jobs, njobs, p->outputs, s));
    }
    if (single) {
      if (int e = nupm_inverse(p, 0, a, o, out_stride, s)) return e;
      h.w = (h.w + 1) % h.ring;
    }
    HIP_TRY(launch_nupc_mix(o + j0 * pts0, out_stride, (const float *)a.pend.p, p->pts1, off, n, p->outputs, s));
    // after slice m - 1: the block's samples replace the ones just heard, its spectra stay in the ring
    if (P >= 1 && sb == m) {
      if (int e = nupm_inverse(p, 1, a, (float *)a.pend.p, p->pts1, s)) return e;
      t.w = (t.w + 1) % t.ring;
    }
    p->c += k;
    j0 += k;
  }
  return CLFA_SUCCESS;
}

// One head block of a fade, on the single-block route with every response-dependent step run for both sets over the
// shared rings: the four multiply-accumulates are one launch and their segments' sums another, the first path's head goes
// to the output rows and the second's to headb, and k_nupc_fade_mix forms both paths' head + pending sums and
// a + g * (b - a) over the outputs rows.  After the fade's last block the second set becomes the first (nothing is copied;
// the object is not capturable, so no address has to stay fixed).
static int nupm_fade_block(clfa_nupconv_matrix *p, float *o, long out_stride, const float *x, long in_stride, hipStream_t s) {
  NupmLevel &h = p->lv[0], &t = p->lv[1];
  NupmSet &a = p->first(), &b = p->second();
  const int pts0 = p->pts0, m = p->m, hb0 = pts0 / 2;
  const long P = p->c / m;
  const int sa = (int)(p->c % m), off = sa * pts0;
  if (int e = nupm_forward(p, h, x, in_stride, s)) return e;
  if (P >= 1 && sa == 0)
    if (int e = nupm_forward(p, t, (const float *)p->stage.p, p->pts1, s)) return e;
  HIP_TRY(launch_nupc_stage(x, in_stride, (float *)p->stage.p, p->pts1, off, pts0, p->inputs, s));
  NupmMacJob jobs[kNupmMacJobs];
  int njobs = 0;
  jobs[njobs++] = nupm_job(p, 0, a, h.w, 0, hb0);
  jobs[njobs++] = nupm_job(p, 0, b, h.w, 0, hb0);
  if (P >= 1) {
    jobs[njobs++] = nupm_job(p, 1, a, t.w, sa * hb0, hb0);
    jobs[njobs++] = nupm_job(p, 1, b, t.w, sa * hb0, hb0);
  }
  HIP_TRY(launch_nupm_mac(jobs, njobs, p->inputs, p->outputs, s));
  HIP_TRY(launch_nupm_reduce(jobs, njobs, p->outputs, s));
  int e;
  if ((e = nupm_inverse(p, 0, a, o, out_stride, s)) || (e = nupm_inverse(p, 0, b, (float *)p->headb.p, pts0, s))) return e;
  h.w = (h.w + 1) % h.ring;
  HIP_TRY(launch_nupc_fade_mix(o, out_stride, (const float *)p->headb.p, (const float *)a.pend.p, (const float *)b.pend.p, p->pts1,
                               off, pts0, p->outputs, p->fade_done * pts0, (float)(p->fade_len * pts0), s));
  if (P >= 1 && sa == m - 1) {
    if ((e = nupm_inverse(p, 1, a, (float *)a.pend.p, p->pts1, s)) || (e = nupm_inverse(p, 1, b, (float *)b.pend.p, p->pts1, s)))
      return e;
    t.w = (t.w + 1) % t.ring;
  }
  p->c++;
  if (++p->fade_done == p->fade_len) {
    p->cur ^= 1;
    p->fade_len = p->fade_done = 0;
  }
  return CLFA_SUCCESS;
}

// The second set's history at position c = P * m + sa, recomputed under its responses from the rings alone with the plain
// path's kernels, hence with its bits: the head's tail from head block c - 1; the tail level's tail, pending rows and tail
// again from tail blocks P - 3 and P - 2 (whole blocks in one multiply-accumulate: the segments cut the term sequence, not
// the bins, so a bin's sums do not depend on how the bins are cut into slices); slices [0, sa) of tail block P - 1, in
// progress.  A block of negative index is not computed: what it would have left is the +0 the rows are cleared to.  Tail
// block P - 3 reads back to input block P - 2 - n1, which is why the tail's ring keeps n1 + 2 frames; head block c - 1
// reads frames w - 2m .. w - 1, all intact in a ring of 2m.
static int nupm_prime(clfa_nupconv_matrix *p, hipStream_t s) {
  NupmLevel &h = p->lv[0], &t = p->lv[1];
  NupmSet &b = p->second();
  const int hb0 = p->pts0 / 2;
  const long P = p->c / p->m;
  const int sa = (int)(p->c % p->m);
  HIP_TRY(b.clear_history(s));
  const auto back = [](const NupmLevel &l, int k) { return (l.w - k + l.ring) % l.ring; };   // the frame k blocks before frame w
  // items [0, nitems) of level k's block in frame w: multiply-accumulate and the segments' sums
  const auto mac = [&](int k, int w, int nitems) {
    const NupmMacJob job = nupm_job(p, k, b, w, 0, nitems);
    HIP_TRY(launch_nupm_mac(&job, 1, p->inputs, p->outputs, s));
    HIP_TRY(launch_nupm_reduce(&job, 1, p->outputs, s));
    return (int)CLFA_SUCCESS;
  };
  // a whole block: then its inverse (the samples: to `out`, rows of the level's block length)
  const auto block = [&](int k, int w, float *out) {
    if (int e = mac(k, w, p->lv[k].bins / 2)) return e;
    return nupm_inverse(p, k, b, out, p->lv[k].bins, s);
  };
  int e;
  if (p->c >= 1 && (e = block(0, back(h, 1), (float *)p->headb.p))) return e;
  if (P >= 3 && (e = block(1, back(t, 2), (float *)b.pend.p))) return e;
  if (P >= 2 && (e = block(1, back(t, 1), (float *)b.pend.p))) return e;
  if (P >= 1 && sa > 0 && (e = mac(1, t.w, sa * hb0))) return e;
  return CLFA_SUCCESS;
}

extern "C" {

int clfa_nupconv_matrix_create(clfa_nupconv_matrix **pc, int device, int cvs, int pts0, int pts1, int inputs, int outputs) {
  return create_object(pc, [&](clfa_nupconv_matrix *p) { return nupm_setup(p, device, cvs, pts0, pts1, inputs, outputs); });
}

void clfa_nupconv_matrix_destroy(clfa_nupconv_matrix *p) { destroy_object(p); }

int clfa_nupconv_matrix_get_error(const clfa_nupconv_matrix *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_nupconv_matrix_get_log(const clfa_nupconv_matrix *p) { return p ? p->log : ""; }
int clfa_nupconv_matrix_nparts(const clfa_nupconv_matrix *p, int level) {
  return p && !p->err && (level == 0 || level == 1) ? p->lv[level].nparts : 0;
}
int clfa_nupconv_matrix_segments(const clfa_nupconv_matrix *p, int level) {
  return p && !p->err && (level == 0 || level == 1) ? p->lv[level].segs : 0;
}
long clfa_nupconv_matrix_position(const clfa_nupconv_matrix *p) { return p ? p->c : 0; }
size_t clfa_nupconv_matrix_state_bytes(const clfa_nupconv_matrix *p) {
  if (!p) return 0;
  return p->lv[0].ringA.bytes + p->lv[1].ringA.bytes + p->stage.bytes + p->sets[0].state_bytes() + p->sets[1].state_bytes();
}
size_t clfa_nupconv_matrix_workspace_bytes(const clfa_nupconv_matrix *p) {
  if (!p) return 0;
  return p->sets[0].workspace_bytes() + p->sets[1].workspace_bytes() + p->headb.bytes + p->bX.bytes + p->bY.bytes + p->bP.bytes +
         p->btail.bytes;
}
long clfa_nupconv_matrix_fade_remaining(const clfa_nupconv_matrix *p) { return p ? p->fade_len - p->fade_done : 0; }
const char *clfa_nupconv_matrix_kernel_name(const clfa_nupconv_matrix *p) { return !p || p->err ? "" : "k_nupm_mac"; }

int clfa_nupconv_matrix_push_ir_dev(clfa_nupconv_matrix *p, const void *ir, long row_stride, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || row_stride < nupm_ir_len(p)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: the responses are one end of it
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  return nupm_push_levels(p, p->first(), (const float *)ir, row_stride, s);
}

int clfa_nupconv_matrix_push_ir(clfa_nupconv_matrix *p, const float *ir) {
  if (int e = obj_error(p)) return e;
  if (!ir) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const long len = nupm_ir_len(p);
  return push_host(p, ir, sizeof(float) * (size_t)p->outputs * p->inputs * len,
                   [&](const void *rows) { return clfa_nupconv_matrix_push_ir_dev(p, rows, len, p->stream); });
}

int clfa_nupconv_matrix_push_ir_fade_dev(clfa_nupconv_matrix *p, const void *ir, long row_stride, long fade_blocks, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || row_stride < nupm_ir_len(p) || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts0)
    return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // one fade at a time
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // everything the fade needs is allocated here, so that no process call allocates because of it: refused under capture
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  NupmSet &b = p->second();
  int e;
  if ((e = nupm_alloc_set(p, b)) || (e = p->headb.ensure(sizeof(float) * (size_t)p->outputs * p->pts0))) return e;
  HIP_TRY(p->order.use(s));
  // the rows' spectra into the second set (as push_ir_dev into the first), then that set's history from the rings
  if ((e = nupm_push_levels(p, b, (const float *)ir, row_stride, s)) || (e = nupm_prime(p, s))) return e;
  p->fade_len = fade_blocks;
  p->fade_done = 0;
  return CLFA_SUCCESS;
}

int clfa_nupconv_matrix_push_ir_fade(clfa_nupconv_matrix *p, const float *ir, long fade_blocks) {
  if (int e = obj_error(p)) return e;
  if (!ir || fade_blocks < 1 || fade_blocks > 0x7fffffffL / p->pts0) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const long len = nupm_ir_len(p);
  return push_host(p, ir, sizeof(float) * (size_t)p->outputs * p->inputs * len,
                   [&](const void *rows) { return clfa_nupconv_matrix_push_ir_fade_dev(p, rows, len, fade_blocks, p->stream); });
}

int clfa_nupconv_matrix_process_dev(clfa_nupconv_matrix *p, void *out, long out_stride, const void *in, long in_stride,
                                    long nblocks, void *stream) {
  if (int e = obj_error(p)) return e;
  const long pts0 = p->pts0;
  long len;
  if (int e = check_blocks_dev(nblocks, pts0, out, out_stride, p->outputs, in, nullptr, in_stride, p->inputs, &len)) return e;
  if (!len) return CLFA_SUCCESS;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // the phase of the schedule is host state, which a replay would not advance
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  // a fade's blocks run one at a time; what follows the fade in the same call takes the usual route
  const long fade = p->fade_len - p->fade_done, nf = nblocks < fade ? nblocks : fade, rest = nblocks - nf;
  if (rest > 1 && rest > p->hcap) {
    const int cap = (int)(rest < p->bcap ? rest : p->bcap);
    if (cap > p->hcap) {
      const size_t frames = sizeof(cpx) * (size_t)cap * (size_t)pts0;
      if (int e = ensure_workspaces({{&p->bX, frames * p->inputs},
                                     {&p->bY, frames * p->outputs},
                                     {&p->bP, frames * p->outputs * (size_t)(p->lv[0].segs - 1)},
                                     {&p->btail, sizeof(float) * (size_t)p->outputs * (size_t)pts0}},
                                    s))
        return e;
      p->hcap = cap;
    }
  }
  HIP_TRY(p->order.use(s));
  const float *x = (const float *)in;
  float *o = (float *)out;
  for (long j = 0; j < nf; j++)
    if (int e = nupm_fade_block(p, o + j * pts0, out_stride, x + j * pts0, in_stride, s)) return e;
  return rest ? nupm_blocks(p, o + nf * pts0, out_stride, x + nf * pts0, in_stride, rest, s) : CLFA_SUCCESS;
}

int clfa_nupconv_matrix_convolution(clfa_nupconv_matrix *p, float *out, const float *in, long nblocks) {
  return blocks_host(p, out, in, nullptr, nblocks, [&](void *o, long len, const void *i1, const void *) {
    return clfa_nupconv_matrix_process_dev(p, o, len, i1, len, nblocks, p->stream);
  });
}

int clfa_nupconv_matrix_reset(clfa_nupconv_matrix *p, void *stream) {
  if (int e = obj_error(p)) return e;
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: finish it first
  HIP_TRY(p->order.use(s));
  // the input history, the tails and the blocks in progress; the responses stay
  for (NupmLevel &l : p->lv) {
    HIP_TRY(hipMemsetAsync(l.ringA.p, 0, l.ringA.bytes, s));
    l.w = 0;
  }
  HIP_TRY(hipMemsetAsync(p->stage.p, 0, p->stage.bytes, s));
  HIP_TRY(p->first().clear_history(s));
  p->c = 0;
  return CLFA_SUCCESS;
}

}  // extern "C"
