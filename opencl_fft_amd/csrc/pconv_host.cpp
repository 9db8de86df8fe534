// pconv_host.cpp — C ABI of the partitioned convolution (see include/clfft_amd.h): Clpconv, one block per call, and its
// multi-block route.  Shared plumbing: conv_host.hpp and, below it, host.hpp.
#include "fft_launch.hpp"
#include "fft_route.hpp"
#include "fft_tables.hpp"
#include "pconv_args.hpp"

using namespace clfa;

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
  PconvBlocks a = pconv_blocks_args(p->g, p->bcap, p->bkt, p->half, p->w2f, p->w2i, p->ringA, p->ringB, p->tail, p->bX, p->bXB,
                                    p->bY, p->btail);
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = rows_aligned8(in1, in_stride) && rows_aligned8(in2, in_stride);
  a.aligned_out = rows_aligned8(out, out_stride);
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
