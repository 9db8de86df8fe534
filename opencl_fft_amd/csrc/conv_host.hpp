// conv_host.hpp — what the host sides of the convolutions share (pconv_host.cpp, dconv_host.cpp, pconv_matrix_host.cpp,
// nupconv_host.cpp), on top of host.hpp: the zero-copy and staged blocking forms of a block call, the checks of the
// multi-block calls, the blocking multi-block forms and pushes.  Every object stages its blocking calls in members in1,
// in2, out and its responses in ir.  No launch header is included here: each host source adds the ones it uses.
// Everything here is inline and hidden, as in host.hpp.
#pragma once
#include "host.hpp"

namespace clfa {

// zero-copy staging of single blocks (mapped pinned host memory)
struct ZeroCopy {
  HostBuf in1, in2, out;
};

// bytes per block up to which the convolutions' blocking host calls go zero-copy: the kernels read the input from, and
// write the output to, mapped pinned host memory (one pass each way), instead of two hipMemcpyAsync calls of 10-15 us
// each around a kernel of a few microseconds
inline constexpr size_t kZeroCopyMaxConv = (size_t)256 << 10;   // the convolutions' blocks (measured at this size only)
// Cldconv only for blocks of up to 4096 samples: every workgroup whose ring window meets the new block reads it from there
inline constexpr size_t kZeroCopyMaxDconv = (size_t)16 << 10;

// The arrays of a blocking call of object T, packed, in the order their staging is ensured: in1, out, in2 (ibytes per
// input, a NULL in2 is not used; obytes of output) ...
template <class T>
inline HostArrays<T, 3> conv_arrays(void *out, size_t obytes, const void *in1, const void *in2, size_t ibytes) {
  return {{{in1, ibytes, 4, false, &T::in1}, {out, obytes, 4, true, &T::out}, {in2, ibytes, 4, false, &T::in2, in2 != nullptr}}};
}
// ... and the staged form around run(out, in1, in2), its one synchronisation the blocking read of cl_conv.cpp:455
template <class T, class Run>
inline int conv_staged(T *p, const HostArrays<T, 3> &io, Run run) {
  return staged_call(p, io.a, [&](const void *const *d) { return run(const_cast<void *>(d[1]), d[0], d[2]); });
}

// A blocking host call of one audio block (blk bytes per input and output): up to zc_max bytes the kernels read the
// inputs from, and write the output to, mapped pinned host memory — no copy calls, one synchronisation (cl_conv.cpp:399,
// 455); larger blocks take the staged form
template <class T, class Run>
inline int block_call(T *p, size_t zc_max, float *out, const float *in1, const float *in2, size_t blk, Run run) {
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

// tables of the pts-bin transforms of Clpconv, the matrix and the levels of the non-uniform objects (cl_conv.cpp:263-287)
inline int upload_conv_tables(int pts, DevBuf &half, DevBuf &w2f, DevBuf &w2i) {
  int e;
  if ((e = upload_half(half, pts)) || (e = upload_w2(w2f, pts, -1.f)) || (e = upload_w2(w2i, pts, 1.f))) return e;
  return CLFA_SUCCESS;
}

// blocks per multi-block sub-batch: workspaces of per_block bytes per block within ~384 MiB, at most 1024 blocks; the
// tuning switch `env` (read per object) may lower it
inline int subbatch_cap(long per_block, const char *env_name) {
  long cap = (384L << 20) / per_block;
  const char *env = getenv(env_name);
  if (env && atol(env) > 0 && atol(env) < cap) cap = atol(env);
  return (int)(cap < 1 ? 1 : (cap > 1024 ? 1024 : cap));
}

// rows of floats in device memory, looked at alone: the shared check's NULL and alignment answers
inline bool device_rows_ok(const void *rows) {
  const CallArray<int> a[] = {{rows, sizeof(float), 4, false, 0}};
  return arrays_ok(a, true);
}

// every row of `stride` floats from q starts 8-byte aligned (what the sub-batch kernels' two-float accesses ask); rows
// that are not there (q NULL) count as aligned
inline bool rows_aligned8(const void *q, long stride) { return ((uintptr_t)q & 7) == 0 && (stride & 1) == 0; }

// the length of a timed crossfade, in blocks of pts samples: at least one, its samples countable in an int
inline bool fade_blocks_ok(long fade_blocks, long pts) { return fade_blocks >= 1 && fade_blocks <= 0x7fffffffL / pts; }

// the count check of a multi-block call: *len = nblocks * pts floats per row, 0 when there is nothing to do
inline int blocks_len(long nblocks, long pts, long *len) {
  *len = 0;
  if (nblocks < 0 || nblocks > 0x7fffffffL / pts) return CLFA_INVALID_VALUE;
  *len = nblocks * pts;
  return CLFA_SUCCESS;
}

// ... and the checks of a device-resident one: out_rows rows of out and in_rows rows of in1 (and in2, where given), there
// and 4-byte aligned, strides of at least *len floats, out overlapping no input row even partly
inline int check_blocks_dev(long nblocks, long pts, const void *out, long out_stride, long out_rows, const void *in1,
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
inline int blocks_host(T *p, float *out, const float *in1, const float *in2, long nblocks, Dev dev) {
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
inline int push_host(T *p, const float *ir, size_t bytes, Push push) {
  const HostArray<T> rows[] = {{ir, bytes, 4, false, &T::ir}};
  return staged_call(p, rows, [&](const void *const *d) { return push(d[0]); });
}

}  // namespace clfa
