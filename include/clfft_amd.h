/* clfft_amd.h — C ABI of libclfft_amd.so (MI355X / gfx950 native FFT and
 * partitioned-convolution engine).
 *
 * This is the drop-in boundary for the hot path of vlazzarini/opencl_fft:
 * the reference has no FFI of its own — its public surface is the C++ classes
 * cl_fft::Clcfft / Clrfft (cl_fft.h:29-111), cl_conv::Clpconv (cl_conv.h:124-188)
 * and cl_conv::Cldconv (cl_dconv.h:17-66).  Every entry point below names the
 * reference member it replaces (file:line relative to the reference tree).
 * include/cl_fft.h, cl_conv.h and cl_dconv.h rebuild those classes as
 * header-only wrappers over this ABI; opencl_fft_amd/ binds it with ctypes.
 *
 * Conventions kept from the reference:
 *   - every call returns an OpenCL-numbered status: 0 = CL_SUCCESS, negative =
 *     error (cl_fft.cpp:298-395); nothing throws across this boundary;
 *   - complex data are interleaved float32 (re, im), batch-major contiguous;
 *   - "host" entry points copy in/out and block, like the reference's
 *     blocking clEnqueueWrite/ReadBuffer (cl_fft.cpp:155-159);
 *   - forward c2c is scaled by 1/N, inverse is unscaled (cl_fft.cpp:39-40);
 *     r2c uses the reference's packed amplitude layout incl. the untouched
 *     self-paired bin M/2 (cl_fft.cpp:178-205).
 * Extensions (the reference does one transform per call): a batch count, and
 * "_dev" entry points that work in place on device-resident buffers on a
 * caller-supplied hipStream_t (passed as void*; NULL is the HIP default stream, as
 * everywhere in HIP).  Work is ordered by that stream only; nothing blocks.
 * A plan / convolution object owns ONE device workspace, so it may have work in flight on one
 * stream at a time: when a call names another stream than the object's previous call, the library
 * first waits (on the host) for that previous stream (not while the new stream is being captured into
 * a hipGraph: a captured launch is ordered by its graph, and the object's earlier work must be complete
 * when the graph is replayed).  Every entry point leaves the calling
 * thread's current HIP device as it found it.
 */
#ifndef CLFFT_AMD_H
#define CLFFT_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLFA_API __attribute__((visibility("default")))

/* status codes: the OpenCL numbers the reference returns (CL/cl.h) */
#define CLFA_SUCCESS 0
#define CLFA_DEVICE_NOT_FOUND (-1)
#define CLFA_DEVICE_NOT_AVAILABLE (-2)
#define CLFA_MEM_OBJECT_ALLOCATION_FAILURE (-4)
#define CLFA_OUT_OF_RESOURCES (-5)
#define CLFA_OUT_OF_HOST_MEMORY (-6)
#define CLFA_INVALID_VALUE (-30)
#define CLFA_INVALID_DEVICE (-33)
#define CLFA_INVALID_COMMAND_QUEUE (-36)
#define CLFA_INVALID_MEM_OBJECT (-38)
#define CLFA_INVALID_KERNEL_ARGS (-52)
#define CLFA_INVALID_OPERATION (-59)
#define CLFA_INVALID_BUFFER_SIZE (-61)

typedef struct clfa_fft clfa_fft;     /* c2c or r2c/c2r plan: Clcfft / Clrfft object */
typedef struct clfa_pconv clfa_pconv; /* Clpconv object, `channels` independent instances */
typedef struct clfa_dconv clfa_dconv; /* Cldconv object */
typedef struct clfa_stft clfa_stft;   /* short-time analysis / overlap-add synthesis plan (extension) */
typedef struct clfa_pconv_matrix clfa_pconv_matrix; /* convolution matrix: inputs mixed into outputs (extension) */
typedef struct clfa_nupconv clfa_nupconv;           /* non-uniformly partitioned convolution, two levels (extension) */
typedef struct clfa_nupconv_matrix clfa_nupconv_matrix; /* ... many inputs into many outputs (extension) */
typedef struct clfa_pvoc clfa_pvoc;   /* phase vocoder on the clfa_stft spectra: (amp, freq) frames both ways (extension) */

/* ---- library / devices ---------------------------------------------------- */
/* replaces clGetDeviceIDs(NULL, CL_DEVICE_TYPE_ALL, ...) at test_cfft.cpp:31,
 * opencl.cpp call sites opcode.cpp:57,113,172,269: HIP device ordinals */
CLFA_API int clfa_device_count(int *count);
/* replaces clGetDeviceInfo(id, CL_DEVICE_NAME, ...) at test_cfft.cpp:37 */
CLFA_API int clfa_device_name(int device, char *buf, size_t len);
/* cl_fft::cl_error_string (cl_fft.cpp:298-395) / cl_conv::cl_string (cl_conv.h:25-122) */
CLFA_API const char *clfa_error_string(int err);
CLFA_API const char *clfa_version(void);

/* ---- tables (host, exact reference formulas) ------------------------------- */
/* bit-reversal index table, cl_fft.cpp:96-101 (twin cl_conv.cpp:290-295) */
CLFA_API int clfa_bitrev_table(int n, int *out);
/* w[i] = (cos(2 pi i/n), -/+ sin(2 pi i/n)), i in [0,n): cl_fft.cpp:86-91 */
CLFA_API int clfa_twiddle_table(int n, int forward, float *out);
/* w2[i] = (cos(pi i/m), -/+ sin(pi i/m)), i in [0,m): cl_fft.cpp:233-238 */
CLFA_API int clfa_r2c_twiddle_table(int m, int forward, float *out);

/* ---- complex FFT: cl_fft::Clcfft ------------------------------------------- */
/* Clcfft::Clcfft(device_id, size, fwd), cl_fft.cpp:44-125.  n = 2^k, 2..65536 is the reference's
 * range (its stage kernel overflows int32 above that, cl_fft.cpp:32); as an extension n up to 2^24
 * is accepted (two passes up to 2^22, three above; 256 MiB of workspace), and so is any length 2..2^22
 * that is not a power of two (the reference's callers pad those, opcode.cpp:30-35): exact DFT by Bluestein's
 * algorithm around two power-of-two plans, same scaling conventions.
 * On failure *plan is still a valid handle whose clfa_fft_get_error() reports
 * the setup error (the reference's constructors never throw, cl_fft.h:65). */
CLFA_API int clfa_cfft_create(clfa_fft **plan, int device, int n, int forward);
/* Clrfft::Clrfft(device_id, size, fwd), cl_fft.cpp:208-259.  size real points
 * = 2^k, 4..131072 (extension: up to 2^25, and multiples of 4 that are not powers of two up to 2^23);
 * the inner complex length is M = size/2 (cl_fft.cpp:210). */
CLFA_API int clfa_rfft_create(clfa_fft **plan, int device, int size, int forward);
/* Clcfft::~Clcfft / Clrfft::~Clrfft, cl_fft.cpp:127-136, 261-265 */
CLFA_API void clfa_fft_destroy(clfa_fft *plan);
/* Clcfft::get_error(), cl_fft.h:65; Clcfft::get_log(), cl_fft.h:69 */
CLFA_API int clfa_fft_get_error(const clfa_fft *plan);
CLFA_API const char *clfa_fft_get_log(const clfa_fft *plan);
/* Clcfft::transform(c), cl_fft.cpp:153-161: in place on `batch` host arrays of
 * n complex (batch = 1 is the reference call). */
CLFA_API int clfa_cfft_transform(clfa_fft *plan, float *c, long batch);
/* Clrfft::transform(c, r), cl_fft.cpp:267-296.  forward: r (size floats per
 * batch) -> c (M complex per batch); inverse: c -> r.  c and r may alias. */
CLFA_API int clfa_rfft_transform(clfa_fft *plan, float *c, float *r, long batch);
/* Extension to the two host calls above, which replace the reference's blocking clEnqueueWriteBuffer / ReadBuffer around
 * every transform (cl_fft.cpp:155-158, 275-291): a caller that keeps ONE array for the plan's life (the Csound opcodes keep
 * one buffer per instance, csound/opcode.cpp) takes it from the plan — page-locked host memory the device sees.  transform
 * calls on arrays INSIDE such a buffer run on that memory directly: the kernels read and write it over PCIe, one pass each
 * way, no staging copy (up to 8 MiB per call and on the routes that touch source and destination once; otherwise the usual
 * copies, by DMA).  Results are bit-identical to the copying call.  The memory lives until clfa_fft_host_free or the plan's
 * destruction.  Real plans, out of place: both arrays must come from the plan for the direct route.  (Pinning the caller's
 * own heap array — hipHostRegister — was measured and is not offered: clfft_amd.cpp, profiles/host_path_r05.txt.) */
CLFA_API int clfa_fft_host_alloc(clfa_fft *plan, size_t bytes, void **ptr);
CLFA_API int clfa_fft_host_free(clfa_fft *plan, void *ptr);
/* device-resident, in place, asynchronous on `stream`: the body of
 * Clcfft::fft() (cl_fft.cpp:138-151) / the kernel part of Clrfft::transform.
 * data: batch * n complex64 (c2c) or batch * size float32 (r2c, packed in place).  data (and src / dst below) must be
 * 8-byte aligned, for real plans too: the kernels move complex64 values, and real samples in pairs, as 8-byte words;
 * 16 bytes are not required. */
CLFA_API int clfa_fft_exec_dev(clfa_fft *plan, void *data, long batch, void *stream);
/* the same from `src` to `dst` (extension).  The reference's device side is itself out of place — its `reorder` gathers
 * data1 -> data2 and the stages then run on data2, cl_fft.cpp:138-151.  Every plan runs
 * src -> dst natively, at the cost of the in-place call: the kernels read the source and write the destination, routes of
 * several passes put their first pass there.  src == dst is clfa_fft_exec_dev; partly overlapping buffers, and buffers
 * that are not a whole number of complex values apart, are CLFA_INVALID_VALUE.  `src` is left untouched. */
CLFA_API int clfa_fft_exec_dev_oop(clfa_fft *plan, const void *src, void *dst, long batch, void *stream);
/* The reference's protected members for subclasses (cl_fft.h:35-44): data1 / data2 = the object's own device buffers of one
 * transform each (n complex64; real plans: size floats), allocated on first request and released with the plan;
 * commands = the plan's hipStream_t (the reference's cl_command_queue). */
CLFA_API int clfa_fft_device_buffers(clfa_fft *plan, void **data1, void **data2, void **commands);
/* ... and its tables (cl_fft.h:35; cl_fft.cpp:86-104): w = n complex64 twiddles of the plan's direction, b = n int32
 * bit reversals (c2c plans of the reference's range only, n <= 65536), device copies made on first request */
CLFA_API int clfa_fft_device_tables(clfa_fft *plan, void **w, void **b);
/* clEnqueueWriteBuffer / clEnqueueReadBuffer / clFinish as the reference uses them on its queue (cl_fft.cpp:155-158):
 * host <-> device copies on a hipStream_t (NULL: the default stream), blocking or not */
CLFA_API int clfa_copy_to_device(void *stream, void *dst, const void *src, size_t bytes, int blocking);
CLFA_API int clfa_copy_from_device(void *stream, void *dst, const void *src, size_t bytes, int blocking);
CLFA_API int clfa_stream_synchronize(void *stream);
/* Clcfft::fft(), cl_fft.cpp:138-151: one transform data1 -> data2 on the plan's stream; like the reference it only
 * enqueues (synchronise the stream before reading data2).  Real plans run their whole r2c / c2r. */
CLFA_API int clfa_fft_run_buffers(clfa_fft *plan);
/* bytes of device workspace a plan holds (0 for single-pass sizes) */
CLFA_API size_t clfa_fft_workspace_bytes(const clfa_fft *plan);
/* name of the HIP kernel that does the work for this plan (for profiles) */
CLFA_API const char *clfa_fft_kernel_name(const clfa_fft *plan);
/* measurement aid (complex n = 65536 plans, CLFA_INVALID_OPERATION for others): with on != 0 every later launch of the
 * resident kernel k_fft_res16 leaves one 16-byte record per workgroup — { uint32 transforms it processed, uint32
 * workgroup index % 8, uint64 wall clock (100 MHz) at its exit } — at the price of one store per
 * workgroup; on = 0 stops it.  clfa_fft_balance_read waits for the device and copies the last launch's records, in
 * workgroup order (workgroup i runs on XCD i % 8), up to max_records of them; *count = how many.  Both calls block. */
CLFA_API int clfa_fft_balance_record(clfa_fft *plan, int on);
CLFA_API int clfa_fft_balance_read(clfa_fft *plan, void *records, int max_records, int *count);
/* test aid (the same plans, CLFA_INVALID_OPERATION for others): waits for the device and copies the 352 32-bit words around
 * the shared assignment's counters in the plan's workspace, up to max_words of them; *count = how many.  Words 0..31 and
 * 320..351 are the guard lines in front of and behind the counters and always hold 0xA5A5A5A5; words 32..319 are the nine
 * 128-byte counter lines, all zero whenever no launch is running. */
CLFA_API int clfa_fft_balance_counters(clfa_fft *plan, unsigned *words, int max_words, int *count);

/* measurement aid (nothing of the reference's): sustained device-memory bandwidth in TB/s over
 * `launches` launches on two buffers of `bytes` each (a multiple of 512 KiB, far beyond the 256 MiB
 * Infinity Cache for a meaningful number).  what: 0 read, 1 write, 2 copy (all 16-byte non-temporal
 * accesses, contiguous), 3 copy in the four-step FFT's own shape (256 x 256 matrices of 8-byte elements
 * moved in blocks of 16 columns: 128-byte segments 2 KiB apart).  Copies count bytes read + written. */
CLFA_API int clfa_bandwidth_probe(int device, int what, size_t bytes, int launches, double *tb_per_s);

/* the reference's `reorder` kernel as a stand-alone op (cl_fft.cpp:24-27):
 * out[b*n + k] = in[b*n + bitrev(k)], exact gather of complex64, out != in */
CLFA_API int clfa_reorder_dev(int device, void *out, const void *in, int n, long batch, void *stream);

/* ---- partitioned convolution: cl_conv::Clpconv ------------------------------ */
/* Clpconv::Clpconv(device_id, cvs, pts, ...), cl_conv.cpp:140-320, for
 * `channels` independent instances (channels = 1 is the reference object).
 * bins = pts, nparts = cvs / pts (floor, cl_conv.cpp:143). */
CLFA_API int clfa_pconv_create(clfa_pconv **pc, int device, int cvs, int pts, int channels);
CLFA_API void clfa_pconv_destroy(clfa_pconv *pc);            /* cl_conv.cpp:322-347 */
CLFA_API int clfa_pconv_get_error(const clfa_pconv *pc);     /* Clpconv::get_cl_err, cl_conv.h:187 */
/* state readers (ring indices must match the reference bit for bit, cl_conv.cpp:144,424,385,519) */
CLFA_API int clfa_pconv_nparts(const clfa_pconv *pc);
CLFA_API int clfa_pconv_wp(const clfa_pconv *pc);
CLFA_API int clfa_pconv_wp2(const clfa_pconv *pc);
/* Clpconv::push_ir(ir), cl_conv.cpp:353-388: ir = channels x (nparts*pts) floats */
CLFA_API int clfa_pconv_push_ir(clfa_pconv *pc, const float *ir);
/* device-resident form: channel c's response starts at ir + c * channel_stride floats
 * (channel_stride >= nparts*pts; a (channels, cvs) tensor passes cvs), nparts*pts floats are read of each */
CLFA_API int clfa_pconv_push_ir_dev(clfa_pconv *pc, const void *ir, long channel_stride, void *stream);
/* Clpconv::convolution(out, in), cl_conv.cpp:393-458: channels x pts floats each */
CLFA_API int clfa_pconv_convolution(clfa_pconv *pc, float *out, const float *in);
/* Clpconv::convolution(out, in1, in2), cl_conv.cpp:460-548 (time-varying) */
CLFA_API int clfa_pconv_convolution_tv(clfa_pconv *pc, float *out, const float *in1, const float *in2);
/* device-resident variants; in2 may be NULL (static IR).  `out` must not overlap an input, not even partly, on the one-launch
 * routes (clfa_pconv_kernel_name() = k_pconv_fused or k_pconv_coop: partitions up to 4096 samples), where workgroups of
 * other channels may still be reading: CL_INVALID_VALUE.  The launch chain of larger partitions reads every input before it
 * writes `out`; in place is accepted there.  out, in1 and in2 are 8-byte aligned (the kernels move real samples in pairs,
 * as for the real FFT plans above); 16 bytes are not required. */
CLFA_API int clfa_pconv_process_dev(clfa_pconv *pc, void *out, const void *in1, const void *in2, void *stream);
CLFA_API size_t clfa_pconv_state_bytes(const clfa_pconv *pc);
/* which launch structure a block of this object takes (diagnostics and tests): "k_pconv_fused" (one launch, one
 * workgroup per channel), "k_pconv_coop" (one launch, a few channels), "chain" (forward / MAC / inverse launches) */
CLFA_API const char *clfa_pconv_kernel_name(const clfa_pconv *pc);
/* Many blocks per call (extension): a whole signal, or a long stretch of it, per channel.
 * nblocks consecutive blocks per channel: block j of channel c is in1 + c*in_stride + j*pts (pts floats), same for in2
 * and out.  The call equals nblocks calls of clfa_pconv_process_dev, one per block j in ascending order, where call j gets
 * the channels x pts gather of block j (and of in2 when it is non-NULL, the time-varying form); the object's state
 * afterwards (wp, wp2, both rings, the overlap-add tail) is the state those calls leave, so single-block calls and
 * push_ir mix freely with it.  Every output bin sums the partitions in ascending order with one accumulator: results are
 * bit-identical however a signal is split into calls, and across repeated calls, streams and graph replay; against the
 * single-block calls they agree to rounding (which routes match them bit for bit: DESIGN.md, section 4.5).
 * Arguments: nblocks == 0 succeeds and does nothing; in_stride >= nblocks*pts and out_stride >= nblocks*pts; addresses
 * 4-byte aligned, any stride.  out overlapping an input even partly, or any other bad argument: CLFA_INVALID_VALUE, and
 * the state is untouched.  Streams, the current device and hipGraph capture work as for clfa_pconv_process_dev.
 * Workspace: allocated by the first call that needs it (clfa_pconv_blocks_workspace_bytes() = what is held), released
 * with the object; a call under capture that would have to allocate it returns CLFA_INVALID_OPERATION.  Long calls run
 * in sub-batches of an internal cap (time-varying: at most nparts blocks each). */
CLFA_API int clfa_pconv_process_blocks_dev(clfa_pconv *pc, void *out, long out_stride, const void *in1, const void *in2,
                                           long in_stride, long nblocks, void *stream);
/* host form: rows contiguous (stride nblocks*pts), blocking */
CLFA_API int clfa_pconv_convolution_blocks(clfa_pconv *pc, float *out, const float *in1, const float *in2, long nblocks);
CLFA_API size_t clfa_pconv_blocks_workspace_bytes(const clfa_pconv *pc);
/* "k_pconvb_mac" (partitions of 32..4096 samples: four launches per sub-batch), "loop" (other sizes: the single-block
 * route once per block inside the call) */
CLFA_API const char *clfa_pconv_blocks_kernel_name(const clfa_pconv *pc);

/* ---- direct convolution: cl_conv::Cldconv ----------------------------------- */
/* Cldconv::Cldconv(device_id, cvs, vsize, ...), cl_dconv.cpp:46-98 */
CLFA_API int clfa_dconv_create(clfa_dconv **dc, int device, int irsize, int vsize);
CLFA_API void clfa_dconv_destroy(clfa_dconv *dc);            /* cl_dconv.cpp:100-107 */
CLFA_API int clfa_dconv_get_error(const clfa_dconv *dc);     /* cl_dconv.h:65 */
CLFA_API int clfa_dconv_push_ir(clfa_dconv *dc, const float *ir);                 /* cl_dconv.cpp:150-153 */
CLFA_API int clfa_dconv_convolution(clfa_dconv *dc, float *out, const float *in); /* cl_dconv.cpp:109-132 */
CLFA_API int clfa_dconv_convolution_tv(clfa_dconv *dc, float *out, const float *in1, const float *in2); /* :134-148 */
/* device-resident variant of both (in2 may be NULL): vsize floats each, asynchronous on `stream`, one launch per
 * block; out must not be in1 or in2 */
CLFA_API int clfa_dconv_process_dev(clfa_dconv *dc, void *out, const void *in1, const void *in2, void *stream);
/* Many channels and many blocks per call (extension).
 * clfa_dconv_create_channels: `channels` independent instances (1..65535) in one object — `channels` delay rings and
 * coefficient rings of end = irsize + vsize floats each, one write point wp for all of them (clfa_dconv_wp).
 * clfa_dconv_create is channels = 1.  On an object with channels > 1, clfa_dconv_push_ir takes channels x irsize floats,
 * and clfa_dconv_convolution, clfa_dconv_convolution_tv and clfa_dconv_process_dev take channels x vsize contiguous floats
 * and are the block call below with nblocks = 1; on channels == 1 those calls are what they were. */
CLFA_API int clfa_dconv_create_channels(clfa_dconv **dc, int device, int irsize, int vsize, int channels);
/* device-resident push_ir: channel c's response starts at ir + c * channel_stride floats (channel_stride >= irsize, ir
 * 4-byte aligned), irsize floats are read of each; asynchronous on `stream` */
CLFA_API int clfa_dconv_push_ir_dev(clfa_dconv *dc, const void *ir, long channel_stride, void *stream);
/* nblocks consecutive blocks per channel: channel c's samples are in1 + c*in_stride (nblocks*vsize floats), same for in2
 * and out.  Write wp0 for the write point when the call starts, and x_c[tau] for sample tau >= 0 of channel c's in1 row,
 * for -irsize <= tau < 0 the delay ring's content at index (wp0 + tau) mod end.
 * Static form (in2 == NULL), 0 <= t < nblocks*vsize:
 *     out_c[t] = sum_{k=0}^{irsize-1} coef_c[k] * x_c[t - 1 - k]
 * (the one-sample delay is the reference's, cl_dconv.cpp:40-41).
 * Time-varying form (in2 != NULL): output block j uses coef_c^(j)[k] in that sum: with last = (j+1)*vsize - 1 and
 * tau' = last - ((last - (k - wp0)) mod end) (non-negative mod), coef_c^(j)[k] = in2_c[tau'] when tau' >= 0, else the
 * coefficient ring's content at index k — the reference's ring write of in2 at the write point (cl_dconv.cpp:134-147)
 * followed by its reads of coefs[irsize-1-h].
 * State after the call: exactly what nblocks single-block calls leave — both rings hold the last `end` samples of in1
 * (and of in2 in the two-input form) at indices (wp0 + tau) mod end, earlier content stays where fewer than `end`
 * samples came, and wp = (wp0 + nblocks*vsize) mod end.  So single-block calls, block calls and push_ir mix freely.
 * Static form: one kernel over (channel, tile of consecutive outputs of the whole call, tap segment) and a launch that
 * files the samples in the rings, per sub-batch (responses longer than 4096 taps: the segments' partial sums go to a
 * workspace and a third launch adds them).  Every output sums its taps in ascending k in chunks of 256 taps, the chunks'
 * sums in ascending order, then the segments' in ascending order: results are bit-identical however a signal is split
 * into calls and sub-batches, and across repeated calls, streams and graph replay; against the single-block kernel of
 * a one-channel object (k_dconv_block, another order) they agree to rounding.
 * Time-varying form: the "loop" route — per block and per channel one launch of the single-block kernel, serial on the
 * stream.  It is correct and it is not fast (nblocks x channels launches).
 * Arguments: nblocks == 0 succeeds and does nothing; in_stride >= nblocks*vsize and out_stride >= nblocks*vsize;
 * addresses 4-byte aligned, any stride.  out overlapping an input even partly, or any other bad argument:
 * CLFA_INVALID_VALUE, and the state is untouched.  Streams, the current device and hipGraph capture work as for
 * clfa_dconv_process_dev.  Workspace (segmented static route only): allocated by the first call that needs it
 * (clfa_dconv_blocks_workspace_bytes() = what is held), released with the object; a call under capture that would have to
 * allocate it returns CLFA_INVALID_OPERATION.  Long calls of segmented responses run in sub-batches of an internal cap. */
CLFA_API int clfa_dconv_process_blocks_dev(clfa_dconv *dc, void *out, long out_stride, const void *in1, const void *in2,
                                           long in_stride, long nblocks, void *stream);
/* host form: rows contiguous (stride nblocks*vsize), blocking */
CLFA_API int clfa_dconv_convolution_blocks(clfa_dconv *dc, float *out, const float *in1, const float *in2, long nblocks);
/* diagnostics: channels, the write point, bytes of the rings, bytes of the block calls' workspace, and the route of a
 * block call: "k_dconvb_fir" (static form) or "loop" (time_varying != 0) */
CLFA_API int clfa_dconv_channels(const clfa_dconv *dc);
CLFA_API int clfa_dconv_wp(const clfa_dconv *dc);
CLFA_API size_t clfa_dconv_state_bytes(const clfa_dconv *dc);
CLFA_API size_t clfa_dconv_blocks_workspace_bytes(const clfa_dconv *dc);
CLFA_API const char *clfa_dconv_blocks_kernel_name(const clfa_dconv *dc, int time_varying);

/* ---- short-time transforms (extension: nothing of the reference's) ----------- */
/* A plan has size = 2^k, 64 <= size <= 16384 (the packed real sizes whose transform runs in one workgroup), a hop
 * 1 <= hop <= size, a window w of size floats (copied at creation; NULL = rectangular) and a direction.  M = size / 2.
 *
 * Analysis: `channels` rows of `samples` floats, row c at signal + c * signal_stride floats (signal_stride >= samples).
 * F = samples < size ? 0 : 1 + (samples - size) / hop frames per row (trailing samples ignored, no padding or centring:
 * torch.stft(center=False)).  Frame (c, f) is what clfa_rfft_transform (size, forward) returns for the float32 vector
 * fl(w[t] * x_c[f * hop + t]), t < size: the reference's packed amplitude layout and scaling (bin 0 = (DC, Nyquist), bin
 * M/2 never conjugated).  Spectra out: channels x F x M complex64, contiguous.
 *
 * Synthesis: spectra channels x F x M complex64, contiguous -> rows of L = (F - 1) * hop + size floats at signal_stride.
 * With r_f = the clfa_rfft_transform (size, inverse) output of frame f (unscaled: it gives back the windowed frame after
 * analysis), y_c[t] = sum over the frames f that cover t, in ascending f, of w[t - f hop] * r_f[t - f hop].  normalize != 0:
 * y_c[t] is divided by env[t] = sum of w[t - f hop]^2 over the same frames wherever env[t] > 1e-11, kept elsewhere.  The
 * env[t] used is the float64 sum rounded once to float32, for every frame count (calls of fewer frames than size / hop
 * included), so the division adds two float32 roundings to y_c[t] and nothing else.
 *
 * Device calls follow the other objects: asynchronous on `stream`, one object = one stream at a time (a change of stream
 * waits for the previous one), capturable into a hipGraph, the current device left as found.  A direction that is not the
 * plan's, and an output that overlaps an input even partly, are CLFA_INVALID_VALUE; F = 0 or channels = 0 is a successful
 * no-op.  signal: any 4-byte aligned address, any stride, any hop; spectra: 8-byte aligned.  The synthesis is
 * deterministic (no atomics): repeated calls, other streams and graph replays give the same bits.
 * CLFA_STFT_GRID_MAX, read at creation, lowers the number of workgroups a launch of either direction may have (a tuning
 * and test switch: 0 or unset = no cap; the results do not depend on it). */
/* argument errors (size, hop) are CLFA_INVALID_VALUE before any device lookup; a failed create still returns a handle */
CLFA_API int clfa_stft_create(clfa_stft **st, int device, int size, int hop, const float *window, int forward);
CLFA_API void clfa_stft_destroy(clfa_stft *st);
CLFA_API int clfa_stft_get_error(const clfa_stft *st);
CLFA_API const char *clfa_stft_get_log(const clfa_stft *st);
/* F of `samples`, and L of `frames` (0 for frames = 0) */
CLFA_API long clfa_stft_frames(const clfa_stft *st, long samples);
CLFA_API long clfa_stft_samples(const clfa_stft *st, long frames);
/* device-resident: one launch each */
CLFA_API int clfa_stft_analyze_dev(clfa_stft *st, const void *signal, long signal_stride, long samples, long channels,
                                   void *spectra, void *stream);
CLFA_API int clfa_stft_synthesize_dev(clfa_stft *st, const void *spectra, long frames, long channels, void *signal,
                                      long signal_stride, int normalize, void *stream);
/* host arrays, copied in and out, blocking (like clfa_rfft_transform) */
CLFA_API int clfa_stft_analyze(clfa_stft *st, const float *signal, long signal_stride, long samples, long channels,
                               float *spectra);
CLFA_API int clfa_stft_synthesize(clfa_stft *st, const float *spectra, long frames, long channels, float *signal,
                                  long signal_stride, int normalize);
CLFA_API size_t clfa_stft_workspace_bytes(const clfa_stft *st);
CLFA_API const char *clfa_stft_kernel_name(const clfa_stft *st);

/* ---- phase vocoder on the short-time spectra (extension: nothing of the reference's) ---- */
/* An object has size = 2^k, 64 <= size <= 16384, M = size / 2, a hop 1 <= hop <= size, a sample rate sr > 0 (finite) and
 * channels >= 1.  It converts between
 *   spectra: channels x F x M complex64, contiguous — what clfa_stft_analyze_dev writes and clfa_stft_synthesize_dev reads;
 *   frames:  channels x F x (M + 1) x 2 float32, contiguous — bin k = 0..M holds (amp, freq in Hz): the amp / freq frame of
 *            a phase vocoder (Csound's pvs streams).
 * Both 8-byte aligned.  F frames per channel in every call; F == 0 succeeds and does nothing.
 *
 * Bins as complex numbers: z[k] of a packed spectrum P is (Re P[0], 0) for k = 0, (Im P[0], 0) for k = M, conj(P[M/2]) for
 * k = M/2 and P[k] otherwise.  Synthesis inverts the map: bin M/2 is conjugated back, Re P[0] = Re z[0], Im P[0] = Re z[M]
 * (the imaginary parts of z[0] and z[M] are dropped).
 *
 * Analysis (spectra -> frames).  State: prev, M + 1 complex per channel, (1, 0) in every bin at creation and after reset;
 * after a call it is z of the call's last frame.  Table: e[k] = exp(-2 pi i ((k hop) mod size) / size), computed in double,
 * stored as float32 pairs.  For frame f and bin k, with z_{-1} = prev:
 *   amp = |z_f[k]|;  d = z_f[k] conj(z_{f-1}[k]) e[k];  dev = atan2f(Im d, Re d) / (2 pi) turns, 0 where d = (0, 0);
 *   freq = (k + dev size / hop) sr / size.
 * A frame depends on its own spectrum and the one before: the results are the same bits however a stream of frames is cut
 * into calls.  The products are plain float32: spectra whose |P|^2 overflows float32 are outside the contract.  One launch.
 *
 * Synthesis (frames -> spectra).  State: theta, one uint32 per channel and bin, in units of 2^-32 turn; 0 at creation and
 * after reset.  kf = (float)(hop / sr), divided in double.  For frame f, every float32 operation rounded on its own:
 *   t = freq kf;  r = t - rintf(t);  inc = (uint32)(int64)rint((double)r 2^32);  inc = 0 where freq (or t) is not finite;
 *   theta_f = theta_{f-1} + inc (mod 2^32);  z_f[k] = amp (cos, sin)(2 pi theta_f / 2^32).
 * The phase is an integer, so a parallel scan over frames gives the bits of the serial sum: the phase never drifts, and
 * cutting a stream into calls changes neither the spectra nor the state.  Three launches per sub-batch: the sums of the
 * increments per chunk of clfa_pvoc_scan_chunk() frames; per channel and bin, the chunks' bases and the new state; the
 * walk of every chunk from its base.  No atomics, no waiting between workgroups.  With both states as defined, the
 * synthesis of an analysis reproduces the phases of the spectra (frame 0 from the zero phase on both sides).
 *
 * Device calls follow the other objects: asynchronous on `stream`, one object = one stream at a time (a change of stream
 * waits for the previous one), capturable into a hipGraph (a replay advances the states like the call it recorded), the
 * current device left as found.  A bad argument, or an output that overlaps the input even partly, is CLFA_INVALID_VALUE
 * and leaves both states untouched.  Workspace (the chunk sums of one sub-batch, at most about 64 MiB;
 * CLFA_PVOC_CHUNKS_MAX, read at creation, lowers the chunks per sub-batch): allocated whole by the first synthesis, so its
 * address never changes; workspace_bytes() = what is held; released with the object; a synthesis under capture that would
 * have to allocate it returns CLFA_INVALID_OPERATION.  Longer calls run in sub-batches.
 * Argument errors of create (size, hop, sr, channels) are CLFA_INVALID_VALUE before any device lookup; a failed create
 * still returns a handle. */
CLFA_API int clfa_pvoc_create(clfa_pvoc **pv, int device, int size, int hop, double sr, int channels);
CLFA_API void clfa_pvoc_destroy(clfa_pvoc *pv);
CLFA_API int clfa_pvoc_get_error(const clfa_pvoc *pv);
CLFA_API const char *clfa_pvoc_get_log(const clfa_pvoc *pv);
/* every state as at creation; blocking (CLFA_INVALID_OPERATION while the object's stream is being captured) */
CLFA_API int clfa_pvoc_reset(clfa_pvoc *pv);
CLFA_API int clfa_pvoc_analyze_dev(clfa_pvoc *pv, const void *spectra, void *frames_out, long F, void *stream);
CLFA_API int clfa_pvoc_synthesize_dev(clfa_pvoc *pv, const void *frames, void *spectra_out, long F, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_analyze(clfa_pvoc *pv, const float *spectra, float *frames_out, long F);
CLFA_API int clfa_pvoc_synthesize(clfa_pvoc *pv, const float *frames, float *spectra_out, long F);
/* "k_pvoc_analyze", or with synthesis != 0 "k_pvoc_walk" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_kernel_name(const clfa_pvoc *pv, int synthesis);
CLFA_API size_t clfa_pvoc_workspace_bytes(const clfa_pvoc *pv);
CLFA_API int clfa_pvoc_scan_chunk(void);
/* state diagnostics, blocking: channels x (M + 1) phases; channels x (M + 1) x (re, im) of prev */
CLFA_API int clfa_pvoc_read_phase(clfa_pvoc *pv, unsigned *host);
CLFA_API int clfa_pvoc_read_prev(clfa_pvoc *pv, float *host);

/* ---- oscillator-bank resynthesis: (amp, freq) frames straight to samples ---- */
/* The additive synthesiser next to the inverse transform (Csound's pvsadsyn): every selected bin drives an oscillator, its
 * amplitude and frequency are interpolated sample by sample across the hop, and the output is the sum of the
 * oscillators.  frames: channels x F x (M + 1) x 2 float32 as above.  signal: channels rows of F hop floats, row c at
 * signal + c signal_stride, signal_stride >= F hop; frame f yields the samples [f hop, (f + 1) hop).
 *   fmod: F float32, one per frame, shared by the channels, or NULL: no multiplication at all;
 *   the oscillators are the bins first_bin + i step, i < nbins; step >= 1, nbins >= 1, first_bin >= 0, the last bin <= M;
 *   gain: a float.
 * State of its own, per channel and bin: the phase P, a uint64 in units of 2^-64 turn; W, an int32, the frequency in
 * 2^-32 turn per sample; A, a float32 amplitude.  All 0 at creation and after clfa_pvoc_reset.  prev and theta are never
 * touched, and the state of a bin outside the selection is left bit for bit as it was.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.
 * ks = (float)(1 / sr), divided in double; w_j = (float)((double)j / hop), j = 1..hop, a table made at creation.
 *   Endpoint of frame f: t = fl(fl(freq fmod[f]) ks), without fmod t = fl(freq ks).  Where |t| < 0.5 holds,
 *     W_f = (int32)rint((double)t 2^32) and A_f = amp (a NaN amp is kept: it reaches the samples of its own channel
 *     only).  Where it does not — NaN, infinities, anything at or above Nyquist — the endpoint is silent: W_f = 0, A_f = 0.
 *   Start of the segment: A0, W0 = the previous frame's endpoint, or the state for the call's first frame.  Where
 *     A0 == 0, W0 := W_f: an oscillator that was silent starts at its new frequency, without a glide.  A rule on values.
 *   Phase, exact: with int64 d = W_f - W0, D = floor_div(d 2^30, hop) 4, the floor towards minus infinity;
 *     phase(j) = P + j (W0 2^32) + (j (j + 1) / 2) D mod 2^64 for sample j = 1..hop; the next frame starts from
 *     phase(hop).  The advance of a frame depends on that frame and the one before only.
 *   Amplitude: a(j) = fl(A0 + fl(fl(A_f - A0) w_j)); a(hop) = A_f exactly, since w_hop = 1.
 *   Sample: y = fl(gain S), S the float32 sum, from 0 and in ascending order of the selected bins, of
 *     fl(a(j) cospif(x)), x = (float)(int32)(phase(j) >> 32) 2^-31: the top 32 bits of the phase as a signed number of
 *     half turns, as in the synthesis.  cospif returns exactly 0, 1, -1 at the multiples of a quarter turn.
 *   After the call the state of a selected bin is (phase(hop), W, A) of the call's last frame.
 * Addition mod 2^64 is associative, so the chunked scan of the synthesis applies: the samples and the state are the same
 * bits however a stream of frames is cut into calls, on any stream, under graph replay and for any grid cap.  The order of
 * the sum depends on the selection alone.  tests/pvoc_adsyn_model.py restates all of it; the integer part is
 * opencl_fft_amd/csrc/pvoc_adsyn_plan.hpp, shared by the kernels and the CPU test.
 *
 * Three launches per sub-batch: "k_adsyn_sums" (the uint64 sums of the frames' advances per chunk of
 * clfa_pvoc_scan_chunk() frames), "k_adsyn_scan" (the chunks' bases in place and the new state), "k_adsyn_osc" (a
 * workgroup per channel and chunk: tiles of clfa_pvoc_adsyn_tile_bins() oscillators in LDS, visited in ascending order
 * into one accumulator per sample).  No atomics, no waiting between workgroups.  CLFA_PVOC_ADSYN_GRID_MAX, read at
 * creation, lowers the number of workgroups a launch may have (a tuning and test switch: the results do not depend on it).
 *
 * The calls follow the object's rules: asynchronous on `stream`, one stream at a time, capturable, the current device left
 * as found.  Argument errors that need no device come first (on an object whose creation found no device a bad argument
 * is still CLFA_INVALID_VALUE, a good one the object's error): a bad argument, or an output that overlaps the frames or
 * fmod even partly, is CLFA_INVALID_VALUE and leaves the state untouched.  F == 0 succeeds and does nothing.  Device
 * pointers: frames 8-byte aligned, fmod and signal 4-byte.  Workspace: an allocation of its own (the 64-bit chunk sums of
 * one sub-batch, at most about 64 MiB, CLFA_PVOC_CHUNKS_MAX lowers the chunks per sub-batch; and the endpoints a sub-batch
 * starts from), made whole by the first call; a first call under capture returns CLFA_INVALID_OPERATION; reported by
 * clfa_pvoc_adsyn_workspace_bytes — clfa_pvoc_workspace_bytes keeps reporting the synthesis' alone. */
CLFA_API int clfa_pvoc_adsyn_dev(clfa_pvoc *pv, const void *frames, long F, const void *fmod, int first_bin, int nbins,
                                 int step, float gain, void *signal, long signal_stride, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_adsyn(clfa_pvoc *pv, const float *frames, long F, const float *fmod, int first_bin, int nbins,
                             int step, float gain, float *signal, long signal_stride);
/* state diagnostics, blocking: channels x (M + 1) each of P, W, A */
CLFA_API int clfa_pvoc_adsyn_read_state(clfa_pvoc *pv, unsigned long long *phase, int *w, float *amp);
CLFA_API size_t clfa_pvoc_adsyn_workspace_bytes(const clfa_pvoc *pv);
/* oscillators per LDS tile of k_adsyn_osc (fixed) */
CLFA_API int clfa_pvoc_adsyn_tile_bins(void);
/* "k_adsyn_osc" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_adsyn_kernel_name(const clfa_pvoc *pv);

/* ---- operations on (amp, freq) frames: pitch scale, frequency shift, timed read ---- */
/* Stateless: they read frames and write frames of the layout above, never touch prev or theta, and allocate nothing
 * in a device call (their tables are built by clfa_pvoc_create), so every device call can be captured.  Rules of the
 * object's other calls: asynchronous on `stream`, one stream at a time, the current device left as found; a frame
 * count of 0 succeeds and does nothing; a bad argument, or an output that overlaps an input (the frames or the
 * per-frame array) even partly, is CLFA_INVALID_VALUE and writes nothing.  Argument checks that need no device come
 * first: on an object whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the
 * object's error.  The blocking forms take host arrays and also check the per-frame values; the device forms cannot.
 *
 * cf = (float)(sr / size), bpf = (float)(size / sr), both divided in double.  Every float32 operation below is rounded
 * on its own (no fused multiply-add); fl() marks a rounding.  An EMPTY output bin j is (0, fl(j cf)): silent, at its
 * bin centre.  tests/pvoc_ops_model.py restates all of it in numpy.
 *
 * Pitch scale.  scale: F float32, one per frame, shared by the channels; every value finite and in [0.25, 4] (the
 * blocking form checks; in the device form a value outside the range, or a NaN, makes bins 1..M-1 of that frame EMPTY).
 * coefs is used with keepform only, and then 1 <= coefs < M.  Per channel and frame, s = scale[f]:
 *   bins 0 and M are copied unchanged;
 *   for k = 1..M-1 ascending, j = (int)floorf(fl(k s) + 0.5f); if 1 <= j <= M-1, bin j takes source k, a later k
 *   replacing an earlier one; a bin j in 1..M-1 that no k reaches is EMPTY;
 *   out[j] = (fl(gain amp[k]), fl(freq[k] s)), or with keepform (fl(fl(fl(gain amp[k]) / env[k]) env[j]), fl(freq[k] s)).
 * The kernels compute the map as a gather (j -> the largest k that reaches it; k -> j is monotone): deterministic, no
 * atomics.
 *
 * env, the cepstrally smoothed amplitude of the INPUT frame: L[k] = logf(fmaxf(amp[k], 1e-20f)), k = 0..M (a NaN amp
 * takes the floor); Lext[n] = L[min(n, size - n)], n < size; c0 = mean(Lext), a_q = (2 / size) sum_n Lext[n]
 * cos(2 pi n q / size); logE[k] = c0 + sum_{q = 1..coefs} a_q cos(2 pi k q / size); env[k] = expf(logE[k]).  The kernel
 * computes it as the packed forward real transform of Lext (Clrfft's, scaled), every bin above coefs and the Nyquist half
 * of bin 0 set to zero, and the unscaled inverse, both in LDS; the frame is read once and written once, no workspace.
 *
 * Frequency shift.  shift: F float32 in Hz, finite (the blocking form checks).  1 <= lowest_bin <= M-1.  Per frame,
 * t = fl(shift[f] bpf), d = (int)rintf(t):
 *   bins 0, M and 1 <= j < lowest_bin are copied unchanged;
 *   for lowest_bin <= j <= M-1 the source is k = j - d; if lowest_bin <= k <= M-1 the bin takes the amp of k exactly as
 *   in the pitch scale (with or without keepform) and freq = fl(freq[k] + shift[f]); otherwise it is EMPTY.  Where
 *   |t| <= M does not hold (a shift past every bin, or a NaN in the device form) every such bin is EMPTY.
 *
 * Timed read.  frames_in holds Fin frames per channel, 1 <= Fin <= 2^24; pos: Fout float32 positions in frames, shared
 * by the channels; frames_out holds Fout frames per channel.  Per output frame g:
 *   p = fminf(fmaxf(pos[g], 0), (float)(Fin - 1)) (a NaN position reads frame 0); i = (int)floorf(p); a = p - (float)i;
 *   i1 = min(i + 1, Fin - 1); where a == 0 amp and freq of every bin are those of frame i, copied; otherwise each is
 *   fl(x0 + fl(a fl(x1 - x0))), x0 = in[i], x1 = in[i1].
 *
 * Kernels: "k_pvoc_map" (scale and shift without keepform), "k_pvoc_formant" (with keepform: one workgroup holds the
 * frames of a group in LDS, transforms, lifters, transforms back and applies the map), "k_pvoc_read".  One launch per
 * call.  CLFA_PVOC_OPS_GRID_MAX, read at creation, lowers the number of workgroups a launch may have (a tuning and test
 * switch: the results do not depend on it). */
CLFA_API int clfa_pvoc_scale_dev(clfa_pvoc *pv, const void *frames_in, void *frames_out, long F, const void *scale,
                                 int keepform, float gain, int coefs, void *stream);
CLFA_API int clfa_pvoc_shift_dev(clfa_pvoc *pv, const void *frames_in, void *frames_out, long F, const void *shift,
                                 int lowest_bin, int keepform, float gain, int coefs, void *stream);
CLFA_API int clfa_pvoc_read_dev(clfa_pvoc *pv, const void *frames_in, long Fin, const void *pos, void *frames_out,
                                long Fout, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_scale(clfa_pvoc *pv, const float *frames_in, float *frames_out, long F, const float *scale,
                             int keepform, float gain, int coefs);
CLFA_API int clfa_pvoc_shift(clfa_pvoc *pv, const float *frames_in, float *frames_out, long F, const float *shift,
                             int lowest_bin, int keepform, float gain, int coefs);
CLFA_API int clfa_pvoc_read(clfa_pvoc *pv, const float *frames_in, long Fin, const float *pos, float *frames_out,
                            long Fout);
/* op: 0 = scale, 1 = shift, 2 = read; the kernel's name as above ("" for a failed object or an unknown op) */
CLFA_API const char *clfa_pvoc_ops_kernel_name(const clfa_pvoc *pv, int op, int keepform);

/* ---- analysis of a stored signal at any time points (Csound's pvstanal, mincer, temposcal) ---- */
/* Every output frame is analysed at its own time point, straight from the signal: the window is laid at starts[g] and once
 * more one hop earlier, and the frequencies come from the phase difference of those two spectra.  Reading a stored signal
 * at another speed is then one call (starts[g] = floor(g hop / factor)) followed by the synthesis; the timed read above
 * can only blend the two frames of the hop grid around a time point.  Stateless: prev, theta and every other state of the
 * object are untouched, the call allocates nothing and can be captured.
 *   signal:     `channels` rows of `samples` floats, row c at signal + c * signal_stride; signal_stride >= samples,
 *               1 <= samples <= 2^31 - 1; any 4-byte aligned address;
 *   window:     size floats, 4-byte aligned; required (NULL is CLFA_INVALID_VALUE);
 *   starts:     Fout int32, one per output frame, shared by the channels; any value, in any order;
 *   frames_out: channels x Fout x (M + 1) x 2 float32, contiguous, 8-byte aligned.
 * For channel c and output frame g, with s = starts[g] and all index arithmetic in 64 bits:
 *   x_c[n] is the row's sample for 0 <= n < samples and +0 otherwise;
 *   a[t] = fl(w[t] * x_c[s - hop + t]) and b[t] = fl(w[t] * x_c[s + t]), t < size: a sample outside the row is multiplied
 *   by the window like any other (a negative window value gives -0 there);
 *   PA, PB = what clfa_rfft_transform (size, forward) returns for a and b, zA, zB their bins under the map above;
 *   the frame is the Analysis formula above with z_f = zB and z_{f-1} = zA:
 *     amp = |zB[k]|;  d = zB[k] conj(zA[k]) e[k];  dev = atan2f(Im d, Re d) / (2 pi), 0 where d = (0, 0);
 *     freq = (k + dev size / hop) sr / size.
 * Equivalently, frame (c, g) is frame 1 of what clfa_pvoc_analyze_dev of a fresh object returns for the two spectra that
 * clfa_stft_analyze_dev (size, hop, w) gives for the size + hop floats x_c[s - hop .. s + size): the same bits (the kernel
 * runs the same code).  With starts[g] = g hop every frame g >= 1 is the frame that Stft's and Pvoc's analysis return for
 * the whole signal; frame 0 differs, because its earlier window lies before the signal and prev plays no part.  A NaN
 * sample reaches only the frames whose two windows cover it, in its own channel.
 *
 * The rules of the stateless frame operations hold: argument checks that need no device come first (on an object whose
 * creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the object's error); Fout == 0 succeeds
 * and does nothing; a NULL or misaligned pointer, samples < 1, signal_stride < samples, or frames_out overlapping the
 * signal (its whole strided extent), the window or starts, even partly, is CLFA_INVALID_VALUE and writes nothing.
 * Asynchronous on `stream`, one stream at a time, the current device left as found.  One launch, "k_pvoc_tanal": a
 * workgroup holds a group of output frames in LDS, transforms both windows there, keeps zA in a second LDS buffer and
 * writes the frames; no spectra and no gathered copy of the signal in memory, no atomics, no waiting between workgroups.
 * CLFA_PVOC_OPS_GRID_MAX caps the launch's workgroups as for the other one-launch operations; the result does not depend
 * on it. */
CLFA_API int clfa_pvoc_tanal_dev(clfa_pvoc *pv, const void *signal, long signal_stride, long samples, const void *window,
                                 const void *starts, void *frames_out, long Fout, void *stream);
/* host arrays, staged, blocking */
CLFA_API int clfa_pvoc_tanal(clfa_pvoc *pv, const float *signal, long signal_stride, long samples, const float *window,
                             const int *starts, float *frames_out, long Fout);
/* "k_pvoc_tanal" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_tanal_kernel_name(const clfa_pvoc *pv);

/* ---- operations on two streams of (amp, freq) frames: cross, morph, filter, mix, vocode ---- */
/* Csound's pvscross, pvsmorph, pvsfilter, pvsmix and pvsvoc.  frames_a, frames_b and frames_out: channels x F x (M + 1) x 2
 * float32 in the layout above, 8-byte aligned; p and q: F float32 each, one value per frame, shared by the channels,
 * 4-byte aligned.  MIX reads neither p nor q, and they may be NULL; every other op needs both.  coefs is used by VOCODE
 * only, and there 1 <= coefs < M.
 *
 * The rules of the frame operations above hold: stateless (prev, theta and the oscillator bank's state are never
 * touched), no allocation in a device call (every call can be captured), asynchronous on `stream`, one stream at a time,
 * the current device left as found; F == 0 succeeds and does nothing.  Argument checks that need no device come first: on
 * an object whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the object's error.
 * An output that overlaps either input, p or q, even partly, is CLFA_INVALID_VALUE and writes nothing; the two inputs
 * may overlap or be the same buffer, and p and q may be the same array.  The blocking form also checks the per-frame
 * values (the device form cannot): every value of p and q finite, weights and depths in [0, 1] — both arrays for MORPH,
 * p for FILTER and VOCODE; anything else is CLFA_INVALID_VALUE.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.
 * clamp(x) = fminf(fmaxf(x, 0), 1), so a NaN gives 0.  Per channel, frame f and bin k = 0..M, every bin alike, with
 * a = frames_a, b = frames_b, P = p[f], Q = q[f]:
 *   CROSS   amp = fl(fl(a.amp P) + fl(b.amp Q)); freq = a.freq, a copy of the bits.
 *   MORPH   wa = clamp(P), wf = clamp(Q); amp = a.amp (bits) where wa == 0, b.amp (bits) where wa == 1, otherwise
 *           fl(a.amp + fl(wa fl(b.amp - a.amp))); freq follows the same rule with wf.  A value with weight 0 is not
 *           used, so a NaN there stays out.
 *   FILTER  d = clamp(P); m = 1 where d == 0, otherwise fl(fl(1 - d) + fl(d b.amp)); amp = fl(Q fl(a.amp m));
 *           freq = a.freq (bits).
 *   MIX     the whole pair of b (bits) where b.amp > a.amp, otherwise the pair of a.  Any comparison with a NaN is
 *           false, so a wins.
 *   VOCODE  (a gives the formants, b the excitation) envA, envB = env of the respective input frame, the cepstral
 *           envelope defined above for keepform, with coefs; both are always computed.  d = clamp(P);
 *           r = fl(envA[k] / envB[k]); m = fl(fl(1 - d) + fl(d r)); amp = fl(Q fl(b.amp m)); freq = b.freq (bits).
 * tests/pvoc_pair_model.py restates all of it in numpy.
 *
 * Kernels: "k_pvoc_pair" (ops 0..3: a lane per output bin, 16 bytes in and 8 out, no LDS), "k_pvoc_vocode" (a workgroup
 * holds whole frames in LDS and runs the envelope stages of k_pvoc_formant on the a-frames and then on the b-frames; each
 * input frame is read once, the output written once, no workspace).  One launch per call.  CLFA_PVOC_OPS_GRID_MAX caps
 * the workgroups of both. */
enum { CLFA_PVOC_CROSS = 0, CLFA_PVOC_MORPH = 1, CLFA_PVOC_FILTER = 2, CLFA_PVOC_MIX = 3, CLFA_PVOC_VOCODE = 4 };
CLFA_API int clfa_pvoc_pair_dev(clfa_pvoc *pv, int op, const void *frames_a, const void *frames_b, void *frames_out, long F,
                                const void *p, const void *q, int coefs, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_pair(clfa_pvoc *pv, int op, const float *frames_a, const float *frames_b, float *frames_out, long F,
                            const float *p, const float *q, int coefs);
/* "k_pvoc_pair", "k_pvoc_vocode" for op 4 ("" for a failed object or an unknown op) */
CLFA_API const char *clfa_pvoc_pair_kernel_name(const clfa_pvoc *pv, int op);

/* ---- operations that reshape one stream of (amp, freq) frames along the bins: band, mask, stencil, arp, lock, warp ---- */
/* Csound's pvsbandp / pvsbandr, pvsmaska, pvstencil, pvsarp, pvslock and pvswarp.  frames_in and frames_out: channels x F x
 * (M + 1) x 2 float32 in the layout above, 8-byte aligned.  par: F rows of 4 float32, one row per frame, shared by the
 * channels, 4-byte aligned, required for every op; the columns an op does not name are not read.  table: M + 1 float32,
 * one per bin, shared by channels and frames, 4-byte aligned; required for MASK and STENCIL, not read by the other ops
 * (it may be NULL for them, and is not looked at).  flags: bit 0 = reject, BAND only; any other bit, or bit 0 on another
 * op, is CLFA_INVALID_VALUE.  lowest_bin (1..M-1) and coefs (1..M-1) are used and checked for WARP only.
 *
 * The rules of the frame operations above hold: stateless (prev, theta, the oscillator bank's state and the states of the
 * operations along the frames are never touched), no allocation in a device call (every call can be captured),
 * asynchronous on `stream`, one stream at a time, the current device left as found; F == 0 succeeds and does nothing.
 * Argument checks that need no device come first: on an object whose creation found no device a bad argument is still
 * CLFA_INVALID_VALUE, a good one the object's error.  An output that overlaps the input, par or (MASK, STENCIL) table, even
 * partly, is CLFA_INVALID_VALUE and writes nothing.  The blocking form also checks the per-frame values (the device form
 * cannot): every value the op names finite; BAND 0 <= lc <= lf <= hf <= hc; depths and pos in [0, 1]; tol >= 0; s in
 * [0.25, 4]; anything else is CLFA_INVALID_VALUE.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding; a division is the correctly
 * rounded one, denormals kept.  clamp(x) = fminf(fmaxf(x, 0), 1), so a NaN gives 0.  "bits" is the input's value copied
 * unchanged.  Per channel, frame f and bin k = 0..M, with (amp, freq) the input's pair; every op copies the freq column as
 * bits, except LOCK:
 *   BAND     (pvsbandp; with reject, pvsbandr)  row (lc, lf, hf, hc) in Hz; x = fabsf(freq[k]); every bin alike.  The gain:
 *            g = 0 where lc <= lf && lf <= hf && hf <= hc does not hold (NaNs included), and where x >= lc && x <= hc does
 *            not hold; g = fl(fl(x - lc) / fl(lf - lc)) where x < lf; g = 1 where x <= hf; otherwise
 *            g = fl(fl(hc - x) / fl(hc - hf)).  With reject g := fl(1 - g).  amp = bits where g == 1, +0 where g == 0 (the
 *            input is not used, so a NaN stays out), otherwise fl(amp g).  Csound's exponential ramp is not offered.
 *   MASK     (pvsmaska)  row (depth); d = clamp(depth); amp = bits where d == 0, otherwise fl(amp m),
 *            m = fl(fl(1 - d) + fl(d table[k])).
 *   STENCIL  (pvstencil)  row (gain, level); thr = fl(table[k] level); amp = fl(amp gain) where amp < thr, otherwise bits
 *            (any comparison with a NaN is false).
 *   ARP      (pvsarp)  row (pos, depth, gain); t = (int)floorf(fl(clamp(pos) (float)M)), m = fl(1 - clamp(depth));
 *            amp = fl(amp gain) at k == t; elsewhere bits where m == 1, otherwise fl(amp m).
 *   LOCK     (pvslock)  row (lock, tol) (Csound's tol is 0.01).  Where lock != 0 does not hold the frame is copied as bits
 *            (a NaN locks, as in FREEZE).  Otherwise bin c is a PEAK iff 2 <= c <= M-2 and amp[c] is strictly greater than
 *            amp[c-2], amp[c-1], amp[c+1] and amp[c+2] (a NaN makes a comparison false).  For output bin j in 1..M-1 the
 *            candidate c is j+1 if that is a peak, else j-1 if that is a peak; with a candidate, Fc = freq[c],
 *            d = fl(tol fabsf(Fc)), and freq = Fc (bits) where fabsf(fl(freq[j] - Fc)) < d, otherwise the bits of freq[j].
 *            Amps are always bits; bins 0, M and every bin without a candidate are copied.  Two peaks are at least 3 bins
 *            apart, so no bin neighbours two: the gather equals the serial loop over the peaks, in any order.
 *   WARP     (pvswarp: the spectral envelope moves, the partials stay)  row (s, shift in Hz, gain).  env is the cepstral
 *            envelope of the INPUT frame, exactly as defined above for keepform, with coefs.  t = fl(shift bpf),
 *            d = (int)rintf(t); the frame is WARPED iff s is in [0.25, 4] and |t| <= M (a NaN fails either test).  Bins
 *            0, M and j < lowest_bin are copied as bits.  For j in lowest_bin..M-1 of a warped frame with 1 <= j - d <= M-1
 *            (the bins of the pitch scale's map that take a source), k is the pitch scale's source of bin j - d: the
 *            largest k in 1..M-1 with floorf(fl(k s) + 0.5f) == j - d.  If there is such a k,
 *            amp = fl(fl(fl(gain amp[j]) / env[j]) env[k]).  Every other such bin, and every such bin of a frame that is
 *            not warped, has amp = fl(gain amp[j]).
 * tests/pvoc_shape_model.py restates all of it in numpy.
 *
 * Kernels: "k_pvoc_shape" (ops 0..3: a lane per output bin, 8 bytes in and 8 out, no LDS), "k_pvoc_lock" (the same items;
 * a locked frame's tile goes through LDS with a halo of 3 bins, a frame with lock == 0 is copied bin by bin),
 * "k_pvoc_warp" (a workgroup holds whole frames in LDS and runs the envelope stages of k_pvoc_formant; one read and one
 * write of the frame, no workspace).  One launch per call.  CLFA_PVOC_OPS_GRID_MAX caps the workgroups of all three. */
enum { CLFA_PVOC_BAND = 0, CLFA_PVOC_MASK = 1, CLFA_PVOC_STENCIL = 2, CLFA_PVOC_ARP = 3, CLFA_PVOC_LOCK = 4, CLFA_PVOC_WARP = 5 };
CLFA_API int clfa_pvoc_shape_dev(clfa_pvoc *pv, int op, const void *frames_in, void *frames_out, long F, const void *par,
                                 const void *table, int flags, int lowest_bin, int coefs, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_shape(clfa_pvoc *pv, int op, const float *frames_in, float *frames_out, long F, const float *par,
                             const float *table, int flags, int lowest_bin, int coefs);
/* "k_pvoc_shape" for ops 0..3, "k_pvoc_lock", "k_pvoc_warp" ("" for a failed object or an unknown op) */
CLFA_API const char *clfa_pvoc_shape_kernel_name(const clfa_pvoc *pv, int op);

/* ---- operations along a stream of (amp, freq) frames, with carried state: blur, smooth, freeze ---- */
/* Csound's pvsblur, pvsmooth and pvsfreeze.  frames_in and frames_out: channels x F x (M + 1) x 2 float32 in the layout
 * above, 8-byte aligned; p and q: F float32 each, one value per frame, shared by the channels, 4-byte aligned.  BLUR reads
 * p only, and q may be NULL; SMOOTH and FREEZE need both, and they may be the same array.
 *
 * Each operation carries a state of its own from call to call, so that the results are the same bits however a stream is
 * cut into calls; a captured call advances the state at every replay.  Each state is EMPTY (the frame operations' EMPTY
 * bin, (0, fl(k cf))) in every bin at creation, after clfa_pvoc_reset, and (blur only) after clfa_pvoc_blur_setup.  prev,
 * theta and the oscillator bank's state are never touched.  The rules of the frame operations above hold: no allocation
 * in a device call, asynchronous on `stream`, one stream at a time, the current device left as found; F == 0 succeeds and
 * does nothing.  Argument checks that need no device come first: on an object whose creation found no device a bad
 * argument is still CLFA_INVALID_VALUE, a BLUR call before clfa_pvoc_blur_setup CLFA_INVALID_OPERATION, a good call the
 * object's error.  An output that overlaps the input, p or q, even partly, is CLFA_INVALID_VALUE.  A failed call writes
 * nothing and leaves every state bit for bit as it was.  The blocking form also checks the per-frame values.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.  An output value is a
 * fixed sequence of such roundings of the stream's values: no parallel float sum or scan is used anywhere.
 *
 * BLUR    a moving average over the last n frames.  clfa_pvoc_blur_setup(pv, max_frames), 1 <= max_frames <= 4096, is
 *         blocking, refused with CLFA_INVALID_OPERATION while the object's stream is being captured, allocates the history
 *         of L = max_frames - 1 frames per channel and a spare of the same size, and may be called again (the history is
 *         resized and reset).  The stream seen by frame f of a call is s = history ++ frames_in: s[L + f] is the call's
 *         frame f.  n = 1 where p[f] >= 1 does not hold (a NaN included), otherwise
 *         n = (int)floorf(fminf(p[f], (float)max_frames)); the blocking form demands p finite and 1 <= p[f] <= max_frames.
 *         rn = (float)(1.0 / n), divided in double.  Per bin, for amp and for freq alike: S starts as the value of frame
 *         L + f - n + 1 (the oldest), the later frames are added in ascending order, one rounded float32 addition each,
 *         and out = fl(S rn); n = 1 returns the input's bits.  After the call the history is the last L frames of s.
 * SMOOTH  a one-pole low-pass along the frames.  State y, one pair per channel and bin.  ca = clamp(p[f]),
 *         cf = clamp(q[f]) (clamp as above: a NaN gives 0); amp = y.amp (bits) where ca == 0, x.amp (bits) where ca == 1,
 *         otherwise fl(y.amp + fl(ca fl(x.amp - y.amp))); freq follows the same rule with cf (MORPH's rule); y := out.
 *         The blocking form demands both arrays finite and in [0, 1].
 * FREEZE  State held, one pair per channel and bin.  The amp column is frozen in frame f where p[f] != 0 (a NaN
 *         freezes), the freq column where q[f] != 0.  out.amp = held.amp (bits) where frozen, else in.amp (bits); freq
 *         follows the same rule; held := out.  Equivalently out.amp[f] = in.amp[g], g the last frame <= f of the stream
 *         with p[g] == 0, or the EMPTY value if there is none since the reset.  The blocking form demands finite values.
 * tests/pvoc_time_model.py restates all of it in numpy.
 *
 * clfa_pvoc_time_read_state (blocking): for BLUR the history, channels x L x (M + 1) x 2, oldest first (nothing is written
 * for L = 0; CLFA_INVALID_OPERATION before the setup); for SMOOTH and FREEZE channels x (M + 1) x 2.
 * clfa_pvoc_time_state_bytes: the device memory of the three states, the blur's spare included.
 *
 * Kernels: "k_pvoc_blur" (a lane per bin walks a run of consecutive frames and forms each sum in the defined order, O(n)
 * additions per output; then the last L frames of s go into the spare, which is copied over the history),
 * "k_pvoc_smooth" (a lane per channel and bin walks the call's frames, the loads of a group of frames in flight ahead of
 * the recurrence), "k_pvoc_freeze" (a workgroup finds g of its run's first frame by searching p and q backwards, then walks
 * forward; held is then taken from the output's last frame).  CLFA_PVOC_OPS_GRID_MAX caps the workgroups of all. */
enum { CLFA_PVOC_BLUR = 0, CLFA_PVOC_SMOOTH = 1, CLFA_PVOC_FREEZE = 2 };
CLFA_API int clfa_pvoc_blur_setup(clfa_pvoc *pv, int max_frames);
CLFA_API int clfa_pvoc_time_dev(clfa_pvoc *pv, int op, const void *frames_in, void *frames_out, long F, const void *p,
                                const void *q, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_time(clfa_pvoc *pv, int op, const float *frames_in, float *frames_out, long F, const float *p,
                            const float *q);
CLFA_API int clfa_pvoc_time_read_state(clfa_pvoc *pv, int op, float *host);
CLFA_API size_t clfa_pvoc_time_state_bytes(const clfa_pvoc *pv);
/* max_frames of the last successful setup, 0 before */
CLFA_API int clfa_pvoc_blur_max_frames(const clfa_pvoc *pv);
/* "k_pvoc_blur", "k_pvoc_smooth", "k_pvoc_freeze" ("" for a failed object or an unknown op) */
CLFA_API const char *clfa_pvoc_time_kernel_name(const clfa_pvoc *pv, int op);

/* ---- per-bin delay with feedback along a stream of (amp, freq) frames, with carried state ---- */
/* Csound's pvsbuffer + pvsbufread2 with a delay time per bin taken from a table, the "spectral delay", and with feedback:
 * echoes that decay per bin.  frames_in and frames_out: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte
 * aligned.  Two tables, shared by the channels, fixed for one call and free to change between calls: delays, M + 1 int32
 * (whole frames), 4-byte aligned; feedback, M + 1 float32, 4-byte aligned, or NULL for none.
 *
 * clfa_pvoc_delay_setup(pv, max_delay), 0 <= max_delay <= 4096 (anything else is CLFA_INVALID_VALUE), sets L = max_delay
 * frames and allocates two histories, xhist (the stream's past input frames) and yhist (its past output frames), channels x
 * L x (M + 1) x 2 float32 each, and one spare of the same size that their commits share; every bin of both histories is
 * EMPTY (the frame operations' EMPTY bin, (0, fl(k cf))) after it, and again after clfa_pvoc_reset.  The setup follows
 * clfa_pvoc_blur_setup's rules: blocking, refused with CLFA_INVALID_OPERATION while the object's stream is being
 * captured, the new buffers allocated before the old ones are replaced (a failed allocation leaves the object as it was),
 * and it may be called again (the histories are resized and reset).  A delay call before the setup is
 * CLFA_INVALID_OPERATION.  No other state of the object is touched by any of this.
 *
 * The device form takes d = min(max(delays[b], 0), L) for bin b and uses feedback[b] as it is, whatever it is.  The
 * blocking form refuses, with CLFA_INVALID_VALUE, a delay outside [0, L] (before the setup: outside [0, 4096]) and a
 * feedback that is not finite or has |g| > 1.
 *
 * The streams are xs = xhist ++ frames_in and ys = yhist ++ frames_out: frame f of the call is index L + f of both.  For
 * channel c, bin b and frame f, with j = L + f - d:
 *   where feedback is NULL or d == 0:  out = xs[j][b], both columns, the bits moved.  (d == 0 is the input's frame itself;
 *                                      a loop without a delay is not defined, so the feedback is off for that bin.)
 *   otherwise, every float32 operation rounded on its own (no fused multiply-add; fl() marks a rounding):
 *     a1 = xs[j][b].amp,  a2 = fl(feedback[b] ys[j][b].amp),  out.amp = fl(a1 + a2),
 *     out.freq = ys[j][b].freq where fabsf(a2) > fabsf(a1) holds, else xs[j][b].freq (so with a NaN on either side the
 *     input's freq); the bits are moved.
 * This is y[t] = x[t - d] + g y[t - d], a comb on the delayed input: the transfer function of a delay line with feedback,
 * without a workspace for the line; an echo carries the freq of the partial it echoes.
 *
 * After the call xhist is the last L frames of xs and yhist the last L frames of ys, whichever kernel ran, so the results
 * are the same bits however a stream is cut into calls and whatever route earlier calls took.  The commit follows the
 * blur's spare-buffer rule: no launch both reads and writes a history, and there is no ring position on the host or on
 * the device.
 *
 * The rules of clfa_pvoc_time_dev hold: F == 0 succeeds and does nothing; the checks that need no device come first (on
 * an object whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a call before the setup
 * CLFA_INVALID_OPERATION, a good call the object's error); an output that overlaps the input or a table, even partly, is
 * CLFA_INVALID_VALUE; a failed call writes nothing and leaves both histories bit for bit as they were; no allocation in a
 * device call; asynchronous on `stream`, one stream at a time; capturable, a replay advancing the state.
 * tests/pvoc_delay_model.py restates all of it in numpy.
 *
 * clfa_pvoc_delay_read_state (blocking): which = 0 xhist, 1 yhist (anything else is CLFA_INVALID_VALUE), channels x L x
 * (M + 1) x 2, oldest frame first (nothing is written for L = 0; CLFA_INVALID_OPERATION before the setup).
 * clfa_pvoc_delay_state_bytes: the device memory of the two histories and the spare; clfa_pvoc_time_state_bytes does not
 * count it.
 *
 * Kernels: "k_pvoc_delay" (feedback NULL: a gather, a lane per bin over a run of consecutive frames) and
 * "k_pvoc_delay_fb" (a lane per channel and bin walks the call's frames in blocks of 8; with d <= 8 the taps of ys are the
 * lane's last 8 outputs, kept in registers; with d > 8 a block's 8 frames do not depend on each other and their taps are
 * loaded together, rows of frames_out the lane stored itself among them); then, for each history, the last L frames of its stream go into the spare, which is copied over it.
 * CLFA_PVOC_OPS_GRID_MAX caps the workgroups of all. */
CLFA_API int clfa_pvoc_delay_setup(clfa_pvoc *pv, int max_delay);
CLFA_API int clfa_pvoc_delay_dev(clfa_pvoc *pv, const void *frames_in, void *frames_out, long F, const void *delays,
                                 const void *feedback, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_delay(clfa_pvoc *pv, const float *frames_in, float *frames_out, long F, const int *delays,
                             const float *feedback);
CLFA_API int clfa_pvoc_delay_read_state(clfa_pvoc *pv, int which, float *host);
CLFA_API size_t clfa_pvoc_delay_state_bytes(const clfa_pvoc *pv);
/* max_delay of the last successful setup, -1 before (0 is a setup too) */
CLFA_API int clfa_pvoc_delay_max_frames(const clfa_pvoc *pv);
/* "k_pvoc_delay", or "k_pvoc_delay_fb" for a call with feedback ("" for a failed object) */
CLFA_API const char *clfa_pvoc_delay_kernel_name(const clfa_pvoc *pv, int feedback);

/* ---- per-frame descriptors of a stream of (amp, freq) frames: magnitude, centroid, flux, peak ---- */
/* Frames to control values: Csound's pvscent, the level and onset detectors built from pvsbin, peak followers.
 * frames_in: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte aligned; only the amp column and, for the
 * peak, the freq column are read.  desc: channels x F x 8 float32, 4-byte aligned, one row per frame, the columns below.
 * first_bin and nbins select the bins lo = first_bin .. hi = first_bin + nbins - 1, 0 <= lo <= hi <= M; rectify is 0 or 1;
 * anything else is CLFA_INVALID_VALUE.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.
 *
 * THE TREE SUM T(t) of the terms t[0..M], a term outside lo..hi being +0 (M is a power of two, 32..8192):
 *   1. W = min(M, 256).  For j < W, p[j] starts as t[j]; then t[j + W], t[j + 2W], ... (indices < M) are added in
 *      ascending order, one rounded addition each.
 *   2. While more than one value is left, s[i] = fl(s[2i] + s[2i+1]): adjacent pairs first, a balanced tree.
 *   3. T = fl(s[0] + t[M]): the Nyquist bin last.
 * The pairing is what is fixed; float addition is commutative, so a butterfly in which every lane of a group ends up with
 * the group's sum gives these bits whichever lane of the sibling group a value is fetched from.
 *
 * The columns of the row of frame f of a channel, with a = amp[k], w[k] = fl((float)k cf) (the EMPTY bin's freq,
 * cf = (float)(sr / size)) and prev = the amp of the same bin in the stream's previous frame:
 *   0  MAG        T(a)
 *   1  POW        T(fl(a a))
 *   2  MOM        T(fl(a w[k]))
 *   3  CENT       +0 where MAG == 0, otherwise fl(MOM / MAG), the correctly rounded division (pvscent's rule)
 *   4  FLUX       T(fl(d d)), d = fl(a - prev); with rectify d = +0 wherever d > 0 does not hold, so a NaN is dropped
 *   5  PEAK_AMP   the amp bits of bin kp
 *   6  PEAK_FREQ  the freq bits of bin kp
 *   7  PEAK_BIN   (float)kp
 * kp is the lowest bin in lo..hi whose amp is not a NaN and is >= every amp of the range that is not a NaN (-0 == +0, so
 * the lower bin wins a tie).  If there is no such bin, columns 5..7 are +0, +0, -1.
 *
 * State `last`, channels x (M + 1) amps: the previous frame of a call's frame 0.  0 (the EMPTY amp) at creation and after
 * clfa_pvoc_reset; after a call the amps of the call's last frame, of all bins and not only lo..hi.  So the rows are the
 * same bits however a stream is cut into calls, on any stream and for any grid cap, and a captured call advances the
 * state at every replay.  prev, theta, the oscillator bank's state and the states of the operations along the frames are
 * never touched.  The state is allocated at creation: a device call allocates nothing.  The rules of the frame operations
 * above hold: asynchronous on `stream`, one stream at a time, the current device left as found; F == 0 succeeds and does
 * nothing.  Argument checks that need no device come first: on an object whose creation found no device a bad argument is
 * still CLFA_INVALID_VALUE, a good one the object's error.  A desc that overlaps the frames, even partly, is
 * CLFA_INVALID_VALUE.  A failed call writes nothing and leaves `last` as it was.
 * tests/pvoc_desc_model.py restates all of it in numpy.
 *
 * Kernels: "k_pvoc_desc" (a group of W lanes takes a run of 4 consecutive frames of a channel and walks the bins
 * outermost, lane j holding p[j] of each frame's four sums and a peak in registers: the input is read 5/4 times, bins
 * outside the range not at all; then the tree, inside a wave with DPP and swizzle moves — at the first four levels a lane
 * and its partner split the 16 sums they hold, each adding the other's partial sum to the half it keeps: the tree's
 * additions, half as many a level — and across the waves of a group through LDS; it only reads the state), then
 * "k_pvoc_tail" on the same stream (the freeze's commit: the call's last frame into the state, which the device keeps as
 * pairs).  No atomics, no waiting between workgroups.  CLFA_PVOC_OPS_GRID_MAX caps the workgroups of both. */
enum {
  CLFA_PVOC_DESC_MAG = 0, CLFA_PVOC_DESC_POW = 1, CLFA_PVOC_DESC_MOM = 2, CLFA_PVOC_DESC_CENT = 3, CLFA_PVOC_DESC_FLUX = 4,
  CLFA_PVOC_DESC_PEAK_AMP = 5, CLFA_PVOC_DESC_PEAK_FREQ = 6, CLFA_PVOC_DESC_PEAK_BIN = 7
};
CLFA_API int clfa_pvoc_desc_dev(clfa_pvoc *pv, const void *frames_in, void *desc, long F, int first_bin, int nbins,
                                int rectify, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_desc(clfa_pvoc *pv, const float *frames_in, float *desc, long F, int first_bin, int nbins,
                            int rectify);
/* state diagnostics, blocking: channels x (M + 1) float32, the amps of the stream's previous frame */
CLFA_API int clfa_pvoc_desc_read_state(clfa_pvoc *pv, float *host);
/* the device memory of the state */
CLFA_API size_t clfa_pvoc_desc_state_bytes(const clfa_pvoc *pv);
/* "k_pvoc_desc" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_desc_kernel_name(const clfa_pvoc *pv);

/* ---- filter bank on (amp, freq) frames: band energies, their log, a DCT of that (mel, MFCC) ---- */
/* Frames to feature vectors: Csound's mfb and dct, the mel spectrum and the cepstral coefficients computed from it.
 * frames_in: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte aligned; only the amp column is read.
 * out: channels x F x N float32, dense, 4-byte aligned, one row per frame; N = B without CLFA_PVOC_BANDS_DCT, N = ncoef
 * with it.
 *
 * THE BANK is configuration of the object, set by clfa_pvoc_bank_setup(pv, nbands, first, count, weights): nbands = B,
 * 1 <= B <= 256; band b covers the bins first[b] .. first[b] + count[b] - 1 with count[b] >= 1, first[b] >= 0 and
 * first[b] + count[b] <= M + 1; its weights w_b are count[b] float32, finite and of any sign, the weights of all bands
 * stored one after the other (host arrays; sum(count) values).  Bands may overlap, repeat, and come in any order.
 * Anything else is CLFA_INVALID_VALUE and leaves the object as it was.  The setup follows clfa_pvoc_blur_setup's rules:
 * blocking, refused with CLFA_INVALID_OPERATION while the object's stream is being captured, the new buffers allocated
 * before the old ones are replaced, and it may be called again.  A bands call before the setup is
 * CLFA_INVALID_OPERATION.  clfa_pvoc_reset leaves the bank alone: it is configuration, not stream state.
 * The setup also builds the DCT table, the orthonormal DCT-II: D[q][b] = (float)(s_q cos(pi q (2b + 1) / (2B))) for q, b < B,
 * evaluated in double, s_0 = sqrt(1 / B), s_q = sqrt(2 / B) for q >= 1.  clfa_pvoc_bank_read_dct (blocking) returns the
 * table the device uses, B x B; the bits of the results are defined GIVEN THAT TABLE (two libms may differ in the last
 * place of a double cosine).
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.
 * Per channel and frame, with a[k] the amp of bin k:
 *   TERM   x[k] = a[k] without CLFA_PVOC_BANDS_POWER, x[k] = fl(a[k] a[k]) with it; t_b[i] = fl(x[first_b + i] w_b[i]),
 *          i < count_b.
 *   BAND   E_b = S16(t_b), the descriptors' TREE SUM at a width that fits a band: for j < 16, p[j] = t[j] (+0 where
 *          j >= count); then t[j + 16], t[j + 32], ... are added in ascending order, one rounded addition each; while
 *          more than one value is left, s[i] = fl(s[2i] + s[2i + 1]); E_b is the one value left.  The Nyquist bin is an
 *          ordinary bin here.
 *   LOG    (CLFA_PVOC_BANDS_LOG) L_b = logf(fmaxf(E_b, floor)); floor finite and > 0, else CLFA_INVALID_VALUE in both
 *          forms; a NaN E_b takes the floor (the envelope's rule).  Without the flag floor is not looked at.
 *   DCT    (CLFA_PVOC_BANDS_DCT, 1 <= ncoef <= B) with v = L where LOG is set, else v = E: C_q = the float32 sum of
 *          fl(D[q][b] v_b) for q < ncoef, starting from +0 and running in ascending b.  Without the flag ncoef must be 0.
 * An unknown flag bit is CLFA_INVALID_VALUE.  Nothing above depends on the grid, on the run of frames a workgroup takes
 * or on which lanes take which band: the rows are the same bits however a stream is cut into calls, on any stream, for
 * any grid cap and under graph replay.  logf is the device's (about an ulp); tests/test_gpu_pvoc_bank.py judges it as
 * the envelope tests judge theirs.
 *
 * Stateless apart from reading the bank, and a device call allocates nothing.  The rules of the frame operations above
 * hold: asynchronous on `stream`, capturable, one launch per call, one stream at a time, the current device left as
 * found; F == 0 succeeds and does nothing.  Argument checks that need no device come first: on an object whose creation
 * found no device a bad argument is still CLFA_INVALID_VALUE, a call before the setup CLFA_INVALID_OPERATION, and a good
 * setup or diagnostic the object's error.  Before the setup ncoef is checked against 256 and the output against rows of
 * one value.  An out that overlaps frames_in, even partly, is CLFA_INVALID_VALUE and nothing is written.
 * tests/pvoc_bank_model.py restates all of it in numpy.
 *
 * Kernel: "k_pvoc_bands" (a workgroup of 256 lanes takes a run of consecutive frames of one channel — 8 up to M = 512,
 * then 4, 2, 1 — and puts their amps, squared with POWER, into LDS; it is sixteen rows of 16 lanes, a row taking a band at
 * a time by a schedule computed at the setup, longest band first; lane j walks i = j, j + 16, ..., reads each weight once
 * for the run and keeps one partial sum per frame, folded with the descriptors' in-wave moves; E goes to LDS, then the
 * log, then the DCT with a lane per (frame, q) and D from cache).  Each frame is read once.  No atomics, no waiting
 * between workgroups.  CLFA_PVOC_OPS_GRID_MAX caps its workgroups. */
enum { CLFA_PVOC_BANDS_POWER = 1, CLFA_PVOC_BANDS_LOG = 2, CLFA_PVOC_BANDS_DCT = 4 };
CLFA_API int clfa_pvoc_bank_setup(clfa_pvoc *pv, int nbands, const int *first, const int *count, const float *weights);
/* B of the last successful setup, -1 before */
CLFA_API int clfa_pvoc_bank_bands(const clfa_pvoc *pv);
/* diagnostics, blocking: B x B float32, D[q][b] as the device uses it (CLFA_INVALID_OPERATION before the setup) */
CLFA_API int clfa_pvoc_bank_read_dct(clfa_pvoc *pv, float *host);
/* the device memory of the bank: bands, schedule, weights, DCT table */
CLFA_API size_t clfa_pvoc_bank_state_bytes(const clfa_pvoc *pv);
CLFA_API int clfa_pvoc_bands_dev(clfa_pvoc *pv, const void *frames_in, void *out, long F, int flags, int ncoef, float floor,
                                 void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_bands(clfa_pvoc *pv, const float *frames_in, float *out, long F, int flags, int ncoef, float floor);
/* "k_pvoc_bands" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_bands_kernel_name(const clfa_pvoc *pv);

/* ---- the N loudest bins of every frame: trace, residual, bin list ---- */
/* Csound's pvstrace with an exact count: the N loudest bins of a range of every frame are kept and the rest of the range
 * is silenced; with CLFA_PVOC_TRACE_RESIDUAL it is the other way round (the noise part of a sines-plus-noise split); and
 * the bins kept can be had as a list.
 * frames_in, frames_out: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte aligned.  n: F float32, one per
 * frame, shared by the channels, 4-byte aligned, required.  bins: NULL, or channels x F x list_n int32, 4-byte aligned;
 * list_n >= 1 where bins is given, not looked at where it is NULL.  first_bin and nbins select the bins first_bin ..
 * first_bin + nbins - 1 as for clfa_pvoc_desc_dev (0 <= first_bin, 1 <= nbins, first_bin + nbins <= M + 1); flags: bit 0
 * is CLFA_PVOC_TRACE_RESIDUAL, any other bit is CLFA_INVALID_VALUE.
 *
 * Per channel and frame f, on the bins of the range:
 *   COUNT      N = 0 where n[f] >= 0 does not hold (a NaN, a negative), else N = (int)floorf(fminf(n[f], (float)nbins)).
 *   ORDER      bin j is LOUDER than bin k iff amp[j] > amp[k] as float32 (so -0 == +0), or the amps are equal and j < k:
 *              the tie rule of the descriptors' peak, the lower bin wins.  The amp is compared as it stands, not its
 *              absolute value.  A bin whose amp is a NaN is never a candidate; every other bin of the range is one.
 *   SELECTION  a bin of the range is SELECTED iff it is a candidate and fewer than N candidates of the range are louder
 *              than it: exactly min(N, number of candidates) bins.  Ties at the cut are broken, not all kept (Csound's
 *              pvstrace keeps every bin >= the N-th loudest amp, a varying number).
 *   FRAMES     the freq column is always the input's bits; a bin outside the range is copied as bits.  Inside the range,
 *              without RESIDUAL a selected bin's amp is the input's bits and every other amp is +0 (the input is not
 *              used: a NaN stays out); with RESIDUAL a selected bin's amp is +0 and every other amp is the input's bits
 *              (a NaN amp passes through).
 *   BIN LIST   (bins != NULL) the frame's selected bins in ascending bin order, the first list_n of them; the remaining
 *              entries of the row are -1.  The same list with and without RESIDUAL.
 * There is no arithmetic and so no rounding in any of it, and the selection is a function of one frame: the outputs are
 * the same bits however a stream is cut into calls, on any stream and for any grid cap.
 *
 * Stateless: no state of the object is read or written, and a device call allocates nothing.  The rules of the frame
 * operations above hold: asynchronous on `stream`, capturable, one launch per call, one stream at a time, the current
 * device left as found; F == 0 succeeds and does nothing.  Argument checks that need no device come first: on an object
 * whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the object's error.  This is the
 * one call with two outputs: frames_out or bins overlapping frames_in, n or each other, even partly, is
 * CLFA_INVALID_VALUE and nothing is written.  The blocking form takes any values of n (each is defined above).
 * tests/pvoc_trace_model.py restates all of it in numpy.
 *
 * Kernel: "k_pvoc_trace" (a group of W = min(M, 256) lanes owns a frame and holds its pairs in registers, so the frame is
 * read once; the cut is found by a radix select on the monotone uint32 image of the amps, four passes of 8 bits over 256
 * integer counters in LDS; the tie rule and the list are one prefix count in bin order, by ballots inside a wave and the
 * per-row counts of the waves through LDS).  No atomics on global memory, no waiting between workgroups.
 * CLFA_PVOC_OPS_GRID_MAX caps its workgroups. */
enum { CLFA_PVOC_TRACE_RESIDUAL = 1 };
CLFA_API int clfa_pvoc_trace_dev(clfa_pvoc *pv, const void *frames_in, void *frames_out, const void *n, void *bins,
                                 int list_n, long F, int first_bin, int nbins, int flags, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_trace(clfa_pvoc *pv, const float *frames_in, float *frames_out, const float *n, int *bins,
                             int list_n, long F, int first_bin, int nbins, int flags);
/* "k_pvoc_trace" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_trace_kernel_name(const clfa_pvoc *pv);

/* ---- stereo demix by azimuth, with an azimuth profile ---- */
/* The two inputs are the left and the right channel of one recording: every bin is placed on an azimuth axis by the gain
 * that best cancels it between the channels, the bins inside a window of positions are kept, and the azimuth profile —
 * where the sources sit — can be had beside them.  Csound's pvsdemix, the ADRess method.
 * frames_l, frames_r, frames_out: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte aligned.  par: F x 2
 * float32, 4-byte aligned, required: row f is (pos, width), shared by the channels.  az: NULL, or channels x F x (2P + 1)
 * float32, 4-byte aligned.  P = points, 1 <= P <= 1024.  first_bin and nbins select the bins lo = first_bin .. hi =
 * first_bin + nbins - 1 as for clfa_pvoc_desc_dev (0 <= lo <= hi <= M).  Anything else is CLFA_INVALID_VALUE.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.
 *
 * Per channel, frame f and bin k, with L = l.amp and R = r.amp:
 *   SIDE       the bin is LEFT where L > R holds, otherwise RIGHT (a tie or a NaN is RIGHT).  loud is the larger amp,
 *              quiet the other.  The freq of the output is the freq bits of the loud side's input, in every bin: kept or
 *              not, in the range or not.
 *   SCAN       g[n] = fl((float)n / (float)P), n = 0..P, the correctly rounded division; d[n] = |fl(quiet - fl(g[n] loud))|.
 *              m is the smallest d, nmin the lowest n that has it, mx the largest d; mag = fl(mx - m).  The bin is PLACED
 *              where no d[n] is a NaN and mag > 0 holds.
 *   AZIMUTH    u = nmin - P for LEFT (-P..0, -P is hard left), u = P - nmin for RIGHT (0..P): one axis of 2P + 1 positions,
 *              on which the centred bins of both sides meet at u = 0.
 *   WINDOW     of frame f: pc = fminf(fmaxf(pos, -1), 1) (a NaN gives -1), c = (int)rintf(fl(pc (float)P));
 *              w = fminf(fmaxf(width, 1), (float)(2P + 1)) (a NaN gives 1), H = (int)w / 2, an integer division.  The bin
 *              is KEPT where it is placed, lies in lo..hi, and |u - c| <= H.
 *   FRAMES     the output amp is mag where the bin is kept, +0 elsewhere.
 *   PROFILE    (az != NULL) column j = 0..2P of a frame's row is T(t), THE TREE SUM of the descriptors above (the same W,
 *              the same pairing, the Nyquist bin last, a term outside lo..hi being +0), with t[k] = mag where bin k is
 *              placed and u == j - P, else +0.  The window does not enter the profile.  Every term is >= +0, so no column
 *              is a NaN.
 * The scan need not be executed literally: fl(quiet - fl(g[n] loud)) is monotone in n, so mx is at an end and m where the
 * sign changes.  What is defined is the scan's result, for every input — odd amps, negative ones, infinities and NaNs
 * included; the closed form round(P quiet / loud) alone is not the definition, ties and rounding go to the scan.
 *
 * How this differs from Csound's pvsdemix: there is one signed azimuth axis, not a plane per side, which keeps a source of
 * the other side from piling up at the centre; the side is chosen per bin, by the louder amp; the width is a count of
 * positions centred on pos; and the profile is an output of its own.
 *
 * Stateless: no state of the object is read or written, and a device call allocates nothing.  The rules of the frame
 * operations above hold: asynchronous on `stream`, capturable, one launch per call, one stream at a time, the current
 * device left as found; F == 0 succeeds and does nothing.  Argument checks that need no device come first: on an object
 * whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the object's error.  An output
 * (frames_out, az) that overlaps any input or the other output, even partly, is CLFA_INVALID_VALUE and nothing is
 * written; the two inputs may overlap or be one buffer.  The blocking form also refuses per-frame values outside their
 * meaning: pos must be finite and in [-1, 1], width finite and in [1, 2P + 1]; the device form clamps as above.  The
 * outputs are the same bits however a stream is cut into calls, for any grid cap, on any stream and under graph replay.
 * tests/pvoc_demix_model.py restates all of it in numpy, the scan done literally.
 *
 * Kernels: "k_pvoc_demix" without the profile (a lane per bin, 16 bytes in and 8 out, no LDS; two bisections over n in
 * place of the scan), "k_pvoc_demix_az" with it (a workgroup takes whole frames: the same per bin, leaving (u, mag) of
 * every bin in LDS, 8 bytes a bin; then the 2P + 1 tree sums from LDS, the columns dealt over the waves, four columns a
 * pass, the tree inside a wave with the descriptors' DPP and swizzle moves).  Each input frame is read once, each output
 * written once.  No atomics, no waiting between workgroups.  CLFA_PVOC_OPS_GRID_MAX caps the workgroups of both. */
CLFA_API int clfa_pvoc_demix_dev(clfa_pvoc *pv, const void *frames_l, const void *frames_r, void *frames_out, const void *par,
                                 void *az, long F, int points, int first_bin, int nbins, void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_demix(clfa_pvoc *pv, const float *frames_l, const float *frames_r, float *frames_out, const float *par,
                             float *az, long F, int points, int first_bin, int nbins);
/* "k_pvoc_demix", or "k_pvoc_demix_az" for a call with the profile ("" for a failed object) */
CLFA_API const char *clfa_pvoc_demix_kernel_name(const clfa_pvoc *pv, int with_az);

/* ---- the pitch of every frame from its spectral peaks, and the peak list ---- */
/* Csound's pvspitch (kfr, kamp pvspitch fsig, kthresh): the fundamental frequency of every frame, by subharmonic
 * summation on the frame's spectral peaks, and the list of those peaks (amp, true freq) as an output of its own.  The
 * descriptors' PEAK_FREQ is the loudest bin, which is not the pitch of a voice with a weak or missing fundamental; a
 * peak's freq column is the phase vocoder's estimate of the partial's true frequency, far finer than a bin.
 * frames_in: channels x F x (M + 1) x 2 float32 in the layout above, 8-byte aligned.  rows: channels x F x 4 float32,
 * dense, 4-byte aligned: the columns CLFA_PVOC_PITCH_F0, _SAL, _CONF, _NPEAKS.  peaks: NULL, or channels x F x npeaks x 2
 * float32 (amp, freq) pairs, dense, 8-byte aligned.  first_bin and nbins select the bins lo = first_bin .. hi =
 * first_bin + nbins - 1 with 1 <= first_bin, 1 <= nbins and first_bin + nbins <= M, so that every bin of the range has
 * both neighbours.  1 <= npeaks <= CLFA_PVOC_PITCH_PEAKS_MAX; thresh finite and >= 0; fmin a normal float32 > 0, fmax
 * finite, fmin <= fmax; 0 <= tol <= 0.5; 0 < decay <= 1.  Anything else, a NaN included, is CLFA_INVALID_VALUE.
 *
 * Every float32 operation is rounded on its own (no fused multiply-add); fl() marks a rounding.  Divisions are correctly
 * rounded, as in the descriptors' CENT.  Per channel and frame, with a[k] the amp and q[k] the freq of bin k:
 *   PEAK        bin k of lo..hi is a peak iff a[k] > a[k-1] and a[k] >= a[k+1] (the neighbours are read from the frame even
 *               when they lie outside lo..hi), a[k] >= thresh, and q[k] is finite and q[k] > 0.  A NaN makes its comparison
 *               false.  Of a plateau only the lowest bin is a peak.
 *   LIST        the first npeaks peaks in ascending bin order, L of them; (A[i], Q[i]) = (a, q) of list entry i, as bits.
 *               (A caller who wants the loudest peaks instead runs clfa_pvoc_trace_dev in front.)  peaks, where given,
 *               receives the pairs of the list and (+0, +0) in the entries from L on.
 *   CANDIDATES  for every list entry i and every m = 1..CLFA_PVOC_PITCH_DIV, c = fl(Q[i] / (float)m); it is a candidate
 *               iff fmin <= c <= fmax.
 *   SCORE       s(c) starts at +0 and takes the list entries j = 0..L-1 in that order.  With w[h-1] =
 *               (float)pow((double)decay, h - 1), computed on the host: r = fl(Q[j] / c), h = rintf(r); entry j counts iff
 *               1 <= h <= CLFA_PVOC_PITCH_HARM and fl(fl(|fl(r - h)|) / h) <= tol; if it counts, s = fl(s + fl(A[j] w[h-1])).
 *               A candidate whose score is a NaN is dropped.  (Subharmonic summation on the peaks; the decay lets the true
 *               fundamental beat c / 2, which matches the same peaks at higher harmonic numbers.)
 *   BEST        the candidate that no other candidate beats: d beats c iff s(d) > s(c), or s(d) == s(c) and d > c (of equal
 *               scores the higher pitch wins).  Two candidates equal in both give the same outputs.
 *   ROW         F0 = the bits of the best c; SAL = its score; CONF = fl(SAL / TOTAL) with TOTAL the serial sum of
 *               A[0..L-1] in list order from +0, and CONF = +0 where TOTAL == 0; NPEAKS = (float)L.  With no candidate
 *               F0, SAL and CONF are +0.
 * A row is a function of one frame: the outputs are the same bits however a stream is cut into calls, on any stream, for
 * any grid cap and under graph replay.  The bits are defined given the host's pow (two libms may differ in the last place
 * of a double power; decay = 1 and the first weight are exact everywhere).
 *
 * Stateless: no state of the object is read or written, and a device call allocates nothing.  The rules of the frame
 * operations above hold: asynchronous on `stream`, capturable, one launch per call, one stream at a time, the current
 * device left as found; F == 0 succeeds and does nothing.  Argument checks that need no device come first: on an object
 * whose creation found no device a bad argument is still CLFA_INVALID_VALUE, a good one the object's error.  rows or peaks
 * overlapping frames_in or each other, even partly, is CLFA_INVALID_VALUE and nothing is written.
 * tests/pvoc_pitch_model.py restates all of it in numpy.
 *
 * Kernel: "k_pvoc_pitch" (a group of W = min(M, 256) lanes owns a frame; the lanes test the bins of the range row by row,
 * a peak's place in the list is a prefix count in bin order — ballots inside a wave, the waves' counts through LDS — and
 * the walk stops once npeaks are found; the list goes to LDS; the at most 8 L candidates are dealt to the lanes, each
 * lane scoring its candidates serially over the list, which fixes the order of the sum; the best is reduced by shuffles
 * and through LDS).  No atomics, no waiting between workgroups.  CLFA_PVOC_OPS_GRID_MAX caps its workgroups. */
enum { CLFA_PVOC_PITCH_DIV = 8, CLFA_PVOC_PITCH_HARM = 32, CLFA_PVOC_PITCH_PEAKS_MAX = 32 };
enum { CLFA_PVOC_PITCH_F0 = 0, CLFA_PVOC_PITCH_SAL = 1, CLFA_PVOC_PITCH_CONF = 2, CLFA_PVOC_PITCH_NPEAKS = 3 };
CLFA_API int clfa_pvoc_pitch_dev(clfa_pvoc *pv, const void *frames_in, void *rows, void *peaks, long F, int first_bin,
                                 int nbins, int npeaks, float thresh, float fmin, float fmax, float tol, float decay,
                                 void *stream);
/* host arrays, copied in and out, blocking */
CLFA_API int clfa_pvoc_pitch(clfa_pvoc *pv, const float *frames_in, float *rows, float *peaks, long F, int first_bin,
                             int nbins, int npeaks, float thresh, float fmin, float fmax, float tol, float decay);
/* "k_pvoc_pitch" ("" for a failed object) */
CLFA_API const char *clfa_pvoc_pitch_kernel_name(const clfa_pvoc *pv);

/* ---- convolution matrix (extension: nothing of the reference's) ------------- */
/* Uniformly partitioned overlap-add convolution of `inputs` signals with an outputs x inputs matrix of static responses:
 * y_o = sum over i of x_i * h_{o,i}.
 *
 * Creation: pts a power of two, 32..4096 (other sizes: CLFA_INVALID_VALUE), nparts = cvs / pts (floor, as Clpconv) >= 1,
 * inputs >= 1, outputs >= 1.  A failed creation still returns a handle; get_error / get_log report the error.
 * Responses: push_ir takes outputs x inputs rows of nparts*pts floats, row (o, i) at (o*inputs + i) * nparts*pts;
 * push_ir_dev reads the rows at row_stride >= nparts*pts floats (4-byte aligned).  A push replaces the whole matrix and
 * applies from the next block; the input history and the overlap-add tails are kept (as Clpconv::push_ir keeps ring A).
 * A fresh object has zero responses and zero history.
 *
 * process_dev: `inputs` rows of nblocks*pts floats (row i at in + i*in_stride) -> `outputs` rows of the same length
 * (row o at out + o*out_stride).  Block j of output o equals the sum over i of what a Clpconv(cvs, pts) instance holding
 * h_{o,i} returns for block j of input i (in exact arithmetic).  A call of K blocks equals K calls of one block and leaves
 * the same state.
 *
 * Numerics: for every output bin the products x_i(block) h_{o,i}(partition) are summed in a fixed order: the sequence
 * r = i*nparts + p (inputs ascending, and within an input the partitions from the oldest input block to the newest) is cut
 * at creation into S segments [floor(s*inputs*nparts/S), floor((s+1)*inputs*nparts/S)); each segment is one float32
 * accumulator over its r ascending, and the segment sums are added as ((seg_0 + seg_1) + seg_2) + ...  S depends on the
 * geometry alone (inputs, outputs, pts, nparts, device), never on K, the sub-batch, the split of a signal into calls, the
 * stream or graph replay: all of these give the same bits.
 *
 * Arguments as clfa_pconv_process_blocks_dev: nblocks == 0 succeeds and does nothing; in_stride, out_stride >=
 * nblocks*pts; any 4-byte aligned address and stride.  out overlapping in even partly, or any other bad argument:
 * CLFA_INVALID_VALUE, and the state is untouched.  One object runs on one stream at a time (a change of stream waits for
 * the previous one); capturable into a hipGraph; the current device is left as found.  Workspace: allocated by the first
 * call that needs it (workspace_bytes() = what is held), released with the object; a call under capture that would have
 * to allocate it returns CLFA_INVALID_OPERATION.  Long calls run in sub-batches of an internal cap (at most 1024 blocks;
 * CLFA_PCONV_MATRIX_BLOCKS_MAX, read at creation, lowers it).
 *
 * Timed crossfade (push_ir_fade, push_ir_fade_dev): a change of responses without the step of a plain push.  ir,
 * row_stride and the row layout are those of push_ir / push_ir_dev.  Definition: let A be the responses in force at the
 * push and B the pushed ones; block 0 the next block processed after the push; N = fade_blocks * pts; n a sample's index
 * counted from the first sample of block 0; yA what this object would have produced without the push; yB what a second
 * matrix of the same geometry would produce if it had held B and received every input this object has received so far
 * (yB's overlap-add tail from the block before block 0 included).  Then
 *   for 0 <= n < N the output sample is  yA + g(n) * (yB - yA),  evaluated in float32 in that form (a subtraction, a
 *     multiplication, an addition, each rounded on its own), with  g(n) = (float)n / (float)N  (IEEE division, round to
 *     nearest): exactly 0 at n = 0, rising linearly to (N-1)/N;
 *   from sample N on the output is yB, B is the matrix in force and fade_remaining() is 0.
 * State: the input rings are shared by both paths and written once.  During a fade the object holds a second response
 * set and a second set of tails, primed at the push from the nparts frames the rings hold; when the last fade block has
 * been processed they are copied over the first set on the same stream.  No device address of the object (responses,
 * rings, tails, workspaces) ever changes: a graph captured outside a fade stays valid after one.  state_bytes() and
 * workspace_bytes() count the second set and its workspaces once they exist (from the first fade push on).
 * Refusals (the state is untouched in each): fade_blocks < 1, fade_blocks * pts > 2^31 - 1 or any argument error of
 * push_ir_dev: CLFA_INVALID_VALUE; a fade push, or a plain push_ir / push_ir_dev, while fade_remaining() > 0:
 * CLFA_INVALID_OPERATION; a fade push on a capturing stream (it allocates what the fade needs): CLFA_INVALID_OPERATION;
 * process_dev on a capturing stream while fade_remaining() > 0 (the fade's progress is host state that a replay would
 * not advance): CLFA_INVALID_OPERATION.  A process_dev call outside capture never allocates because of a fade.
 * Numerics: both paths sum every output bin over the object's segments in the object's order, and a sub-batch lies
 * wholly inside or wholly outside a fade: a fade's outputs are the same bits however its blocks are split into calls,
 * for every sub-batch cap and on any stream; from sample N on they are the bits of a plain push of B made at the same
 * point, and a fade from A to A gives the bits of no push at all. */
CLFA_API int clfa_pconv_matrix_create(clfa_pconv_matrix **m, int device, int cvs, int pts, int inputs, int outputs);
CLFA_API void clfa_pconv_matrix_destroy(clfa_pconv_matrix *m);
CLFA_API int clfa_pconv_matrix_get_error(const clfa_pconv_matrix *m);
CLFA_API const char *clfa_pconv_matrix_get_log(const clfa_pconv_matrix *m);
CLFA_API int clfa_pconv_matrix_push_ir(clfa_pconv_matrix *m, const float *ir);
CLFA_API int clfa_pconv_matrix_push_ir_dev(clfa_pconv_matrix *m, const void *ir, long row_stride, void *stream);
CLFA_API int clfa_pconv_matrix_push_ir_fade(clfa_pconv_matrix *m, const float *ir, long fade_blocks); /* host rows, blocking */
CLFA_API int clfa_pconv_matrix_push_ir_fade_dev(clfa_pconv_matrix *m, const void *ir, long row_stride, long fade_blocks,
                                                void *stream);
/* blocks of the fade not yet processed; 0 = none (and for a NULL handle) */
CLFA_API long clfa_pconv_matrix_fade_remaining(const clfa_pconv_matrix *m);
CLFA_API int clfa_pconv_matrix_process_dev(clfa_pconv_matrix *m, void *out, long out_stride, const void *in, long in_stride,
                                           long nblocks, void *stream);
/* host form: rows contiguous (stride nblocks*pts), blocking */
CLFA_API int clfa_pconv_matrix_convolution(clfa_pconv_matrix *m, float *out, const float *in, long nblocks);
/* 0 for a failed object */
CLFA_API int clfa_pconv_matrix_nparts(const clfa_pconv_matrix *m);
/* responses + input rings + tails (+ a fade's second responses and tails); the sub-batch workspaces */
CLFA_API size_t clfa_pconv_matrix_state_bytes(const clfa_pconv_matrix *m);
CLFA_API size_t clfa_pconv_matrix_workspace_bytes(const clfa_pconv_matrix *m);
/* "k_pconvm_mac" ("" for a failed object) */
CLFA_API const char *clfa_pconv_matrix_kernel_name(const clfa_pconv_matrix *m);

/* ---- non-uniformly partitioned convolution (extension): long responses at low latency ---------------------------------
 * Two levels, static responses, `channels` independent instances.  pts0 and pts1 are powers of two with
 * 32 <= pts0 < pts1 <= 4096, m = pts1 / pts0, and cvs >= 3 * pts1.  The head covers h[0 : 2*pts1) in 2m partitions of
 * pts0; the tail covers h[2*pts1 : 2*pts1 + n1*pts1), n1 = floor((cvs - 2*pts1) / pts1), in partitions of pts1; the
 * remainder of cvs is ignored (the reference's floor).  Anything else: CLFA_INVALID_VALUE from create, the offending
 * parameter named in the log; the arguments are checked before the device is looked for.
 *
 * Definition, bit for bit.  For a channel with input stream x, counted from creation or the last reset: let yh be what
 * Clpconv(2*pts1, pts0) holding h[:2*pts1] returns for x through clfa_pconv_process_blocks_dev, and yt what
 * Clpconv(cvs - 2*pts1, pts1) holding h[2*pts1:] returns for x the same way.  Then y[n] = yh[n] + yt[n - 2*pts1], one
 * float32 addition with the head as its first operand; yt[k] = +0 for k < 0, and the addition is performed there too.
 * Both levels take the blocks route's arithmetic whatever the call's length (forward transform, one accumulator per bin
 * over the partitions ascending, inverse transform and overlap-add): the output bits do not depend on how the stream is
 * cut into calls, and a call of K blocks equals K calls of one block, in output and in the state it leaves.  The packed
 * DC / Nyquist rule of the library (products at half gain) applies per level at that level's block size, so the result is
 * NEITHER bit-equal NOR rounding-equal to Clpconv(cvs, pts0): it differs from it in bins 0 and pts of every level's
 * products, as two Clpconv objects of different pts differ from each other.
 *
 * Schedule.  c = head blocks since reset (position()), s = c mod m its phase.  Tail block j (input x[j*pts1 : (j+1)*pts1))
 * is complete after head block (j+1)*m - 1; its spectrum is taken at c = (j+1)*m; head block c in [(j+1)*m, (j+2)*m)
 * computes slice s of its bins (16-byte items [s*pts0/2, (s+1)*pts0/2) of two bins) over all n1 partitions; after slice
 * m - 1 it is inverse-transformed and overlap-added; its pts1 samples are mixed into head blocks [(j+2)*m, (j+3)*m).  Per
 * head block that is 2m partitions of pts0 head bins plus n1 partitions of pts0 tail bins, one forward transform of pts1
 * at phase 0 and one inverse at phase m - 1: no phase carries a whole tail block.  In a call of many blocks the head runs
 * through the blocks route over the whole call and the tail's slices between two period boundaries are one launch: the
 * number of launches is a constant plus a constant per boundary crossed.
 *
 * process_dev: rows as clfa_pconv_process_blocks_dev (row c of `in` at in + c*in_stride floats, nblocks*pts0 floats; any
 * 4-byte aligned address, strides >= nblocks*pts0); nblocks == 0 succeeds and does nothing.  A bad argument, or an out
 * that overlaps in even partly: CLFA_INVALID_VALUE, the state untouched.  A call (or a reset) on a capturing stream:
 * CLFA_INVALID_OPERATION — the phase lives on the host.  One object runs on one stream at a time.  convolution: the same
 * on packed host rows, blocking.
 * push_ir / push_ir_dev: rows of at least 2*pts1 + n1*pts1 floats (e.g. cvs), both levels' responses written in stream
 * order.  At position() % m == 0 a push is exact: at c = P*m it equals pushing the head object of the definition before
 * its block c and the tail object before its block P - 1 (block 0 for P = 0), the tail block whose multiply-accumulate
 * begins at c — the new tail response is heard from sample (P + 1)*pts1 on, the new head at once.  At another phase the
 * tail block in progress sums the bins of its REMAINING slices with the new response and keeps the bins of the slices
 * already done: push at phase 0, or use the timed crossfade below, which is clean at any phase.
 * reset: the input history, the overlap-add tails and the blocks in progress are cleared, position() is 0, the responses
 * stay: the object then repeats what it returned after its creation and the same pushes.
 *
 * Timed crossfade (push_ir_fade, push_ir_fade_dev): a change of responses without the step of a plain push, at any phase.
 * ir, channel_stride and the row layout are those of push_ir / push_ir_dev.  Definition: let A be the response set in
 * force at the push and B the pushed set; c = position() at the push (any phase); block 0 the next head block processed;
 * N = fade_blocks * pts0; n a sample's index counted from the first sample of block 0; yA what this object would have
 * produced without the push; yB what a second object of the same geometry would produce if it had held B since its
 * creation or last reset and had received every input this object has received since then.  Both are complete outputs,
 * head + pending tail, one float32 addition with the head first.  Then
 *   for 0 <= n < N the output sample is  yA + g(n) * (yB - yA),  evaluated in float32 in that form (a subtraction, a
 *     multiplication, an addition, each rounded on its own, no contraction), with  g(n) = (float)n / (float)N  (IEEE
 *     division, round to nearest): exactly 0 at n = 0, rising linearly to (N-1)/N;
 *   from sample N on the output is yB, B is in force, fade_remaining() is 0, and the object is in every later bit the
 *     object that always held B.
 * The output does not depend on how the stream is cut into calls, during the fade or after it; a fade from A to A gives
 * the bits of no push at all.
 * State: the input-spectra rings do not depend on the response; both paths share them and they are written once.  The
 * second path has its own response spectra of both levels, overlap-add tails of both levels, pending row, tail-block
 * accumulators and a scratch row of channels x pts0 for its head output.  All of its history is recomputed at the push
 * from the rings alone with the plain path's kernels, hence with its bits: with P = c div m and s = c mod m, the head's
 * tail from head block c - 1 (c >= 1); the tail level's tail from tail block P - 3 (P >= 3); the pending row and the
 * tail level's tail from tail block P - 2 (P >= 2); slices 0 .. s-1 of tail block P - 1 (P >= 1, s > 0).  A block of
 * negative index is not computed: its contribution is the +0 of a cleared row.  For this the tail's ring keeps n1 + 2
 * frames (the multiply-accumulate walks the newest n1).  When the last fade block has been issued the second set becomes
 * the first by an exchange of pointers on the host, nothing is copied.  The second set is allocated by the first fade
 * push and kept for the next: A FADE DOUBLES THE RESPONSE MEMORY (the tail responses of 256 channels x 2^20 taps are
 * 2 GB), and state_bytes() and workspace_bytes() count the second set from then on.
 * Schedule: a head block of a fade runs one forward transform (and the tail's at phase 0), the stage kernel, ONE
 * k_nupc_mac launch of up to four jobs (head and tail slice under A and under B), the two head inverses, k_nupc_fade_mix
 * and, after phase m - 1, both tail inverses.  A call of K blocks that meets a fade runs the fade's blocks one at a time
 * and what follows the fade on the usual route.
 * Refusals (the state is untouched in each): fade_blocks < 1, fade_blocks * pts0 > 2^31 - 1 or any argument error of
 * push_ir_dev: CLFA_INVALID_VALUE; a fade push, a plain push_ir / push_ir_dev, or a reset while fade_remaining() > 0:
 * CLFA_INVALID_OPERATION; a fade push on a capturing stream: CLFA_INVALID_OPERATION.  The argument checks come before
 * the device is looked at; a failed object answers with its error.
 *
 * Time-varying second input (process_tv_dev, convolution_tv): the response as a live stream, the reference's
 * convolution(out, in1, in2) — "block t of in2 overwrites partition t mod nparts" — stated for two levels.  With
 * R1 = n1 + 2 (the tail blocks of one response period), R0 = R1 * m (its head blocks, tv_period()) and
 * L = R1 * pts1 (the response length push_ir reads), the second input w is a stream of head blocks beside x, and sample j
 * of w is response sample j mod L.  Let c = position() before the block.  A time-varying block carrying the pts0 samples
 * w_c does, in this order:
 *   1. phase 0 (c mod m == 0 and c >= m): with U = c/m - 1 and r = U mod R1, if r >= 2 and every one of the m head blocks
 *      of tail block U was a time-varying block, tail partition r - 2 becomes the pts1 samples those blocks carried.  The
 *      step belongs to the finished tail block: whichever block arrives at phase 0 performs it, plain or time-varying;
 *   2. head partition: with a = c mod R0, if a < 2m head partition a becomes w_c, before this block's
 *      multiply-accumulate;
 *   3. staging: w_c is kept as part c mod m of the second input's tail block c div m;
 *   4. the block is processed exactly as a plain block is.
 * A plain block (process_dev, or process_tv_dev with in2 == NULL) does step 4 and, at phase 0, step 1; it spoils the tail
 * block it falls into, whose partition keeps its old content (the opcode's "freeze").  So plain and time-varying calls
 * mix freely; a partition never written keeps what push_ir put there, or zeros; a plain push_ir between calls overwrites
 * everything as before; and tail partitions change at phase 0 only: no tail block mixes two responses across its slices.
 * Definition, bit for bit: take a second plain object of the same geometry that has received the same pushes and inputs,
 * and keep a response array hc beside it, starting as the pushed responses or zeros.  Before each head block rewrite hc
 * by steps 1 and 2; whenever it changed, push_ir(hc); then process the block with process_dev.  The time-varying call's
 * output and every later output are the bits of that object (the re-push of the unchanged partitions gives their old
 * bits, so a push off phase 0 is harmless there): a rewritten partition is push_ir's forward transform of those samples.
 * A call of K blocks equals K calls of one block, in output and in the state left, however the stream is cut and however
 * plain calls are interleaved.
 * Arguments: rows as process_dev; in2 has its own stride and alignment (any 4-byte aligned address) and may be `in`
 * itself; in2 == NULL is the plain call.  An out that overlaps in or in2, even partly, or any other bad argument:
 * CLFA_INVALID_VALUE.  A capturing stream, or a non-NULL in2 while fade_remaining() > 0: CLFA_INVALID_OPERATION (a fade
 * push AFTER time-varying calls is allowed; later writes go to the set then in force).  Every refusal leaves the state
 * untouched, and the argument checks come before the device is looked at.  reset clears the second input's staged block
 * and its completeness count; the responses stay.  The second stage row (channels x pts1 floats) is allocated by the first
 * time-varying call and counted by state_bytes() from then on; a plain object's figures do not change.
 * Schedule: a single time-varying block is one launch FEWER than a plain one — k_nupc_fwd transforms x and w_c in one
 * launch and files both in their stage rows as it loads them (at phase 0 a launch of it for the tail level goes first:
 * the finished block of x into the input ring and, where step 1 applies, the second input's into its response frame),
 * then k_nupc_mac, the head inverse, k_nupc_mix and, after phase m - 1, the tail inverse.  A call of several blocks is
 * cut at a = 2m and at the response period's end: for the blocks with a < 2m the head is clfa_pconv_process_blocks_dev's
 * time-varying route (the commit launch writes the new frames into the response ring; a second input whose rows lie
 * otherwise than x's takes a forward launch of its own), for the others its static route; either way one k_nupc_stage2
 * launch stages both inputs between period boundaries, and the tail keeps one launch of slices there.  The head's
 * second-input sub-batch workspace is allocated by the first time-varying call and counted by workspace_bytes(). */
CLFA_API int clfa_nupconv_create(clfa_nupconv **pc, int device, int cvs, int pts0, int pts1, int channels);
CLFA_API void clfa_nupconv_destroy(clfa_nupconv *pc);
CLFA_API int clfa_nupconv_get_error(const clfa_nupconv *pc);
CLFA_API const char *clfa_nupconv_get_log(const clfa_nupconv *pc);
/* partitions of level 0 (the head: 2m) or 1 (the tail: n1); 0 for another level or a failed object */
CLFA_API int clfa_nupconv_nparts(const clfa_nupconv *pc, int level);
/* head blocks since creation or the last reset */
CLFA_API long clfa_nupconv_position(const clfa_nupconv *pc);
/* both levels' rings, responses and tails, the stage row and the pending tail output (+ a fade's second responses, tails
 * and pending row); the tail block's accumulators and the head's sub-batch workspaces (grown by the call that needs more
 * blocks than any before it; + a fade's second accumulators and head row) */
CLFA_API size_t clfa_nupconv_state_bytes(const clfa_nupconv *pc);
CLFA_API size_t clfa_nupconv_workspace_bytes(const clfa_nupconv *pc);
/* "k_nupc_mac" ("" for a failed object) */
CLFA_API const char *clfa_nupconv_kernel_name(const clfa_nupconv *pc);
CLFA_API int clfa_nupconv_push_ir(clfa_nupconv *pc, const float *ir);
CLFA_API int clfa_nupconv_push_ir_dev(clfa_nupconv *pc, const void *ir, long channel_stride, void *stream);
CLFA_API int clfa_nupconv_push_ir_fade(clfa_nupconv *pc, const float *ir, long fade_blocks); /* host rows, blocking */
CLFA_API int clfa_nupconv_push_ir_fade_dev(clfa_nupconv *pc, const void *ir, long channel_stride, long fade_blocks,
                                           void *stream);
/* head blocks of the fade not yet processed; 0 = none (and for a NULL handle) */
CLFA_API long clfa_nupconv_fade_remaining(const clfa_nupconv *pc);
CLFA_API int clfa_nupconv_process_dev(clfa_nupconv *pc, void *out, long out_stride, const void *in, long in_stride,
                                      long nblocks, void *stream);
CLFA_API int clfa_nupconv_convolution(clfa_nupconv *pc, float *out, const float *in, long nblocks);
/* the time-varying second input (above); in2 == NULL: the plain call */
CLFA_API int clfa_nupconv_process_tv_dev(clfa_nupconv *pc, void *out, long out_stride, const void *in, long in_stride,
                                         const void *in2, long in2_stride, long nblocks, void *stream);
CLFA_API int clfa_nupconv_convolution_tv(clfa_nupconv *pc, float *out, const float *in, const float *in2,
                                         long nblocks); /* packed host rows, blocking */
/* R0 = (n1 + 2) * m, the head blocks of one response period; 0 for a NULL handle or a failed object */
CLFA_API long clfa_nupconv_tv_period(const clfa_nupconv *pc);
CLFA_API int clfa_nupconv_reset(clfa_nupconv *pc, void *stream);

/* ---- non-uniformly partitioned convolution matrix (extension): many inputs into many outputs at low latency ----------
 * `inputs` signals mixed into `outputs` signals, y_o = sum_i x_i * h_{o,i}, with long static responses at a latency of pts0
 * samples: clfa_nupconv's two levels and schedule around clfa_pconv_matrix's sum over inputs.  Geometry as clfa_nupconv:
 * powers of two with 32 <= pts0 < pts1 <= 4096, m = pts1 / pts0, cvs >= 3 * pts1; the head covers h[0 : 2*pts1) in 2m
 * partitions of pts0, the tail h[2*pts1 : 2*pts1 + n1*pts1), n1 = floor((cvs - 2*pts1) / pts1), in partitions of pts1, the
 * remainder of cvs is ignored; inputs >= 1, outputs >= 1.  Anything else: CLFA_INVALID_VALUE from create, the offending
 * parameter (pts0, pts1, cvs, inputs, outputs) named in the log; the arguments are checked before the device is looked for.
 * Responses: static; row (o, i) at (o * inputs + i) * row_stride floats, at least 2*pts1 + n1*pts1 floats each.
 *
 * Definition, bit for bit, for the input rows counted from creation or the last reset: let yh be what
 * clfa_pconv_matrix(2*pts1, pts0, inputs, outputs) holding h[:, :, :2*pts1] returns for them, and yt what
 * clfa_pconv_matrix(cvs - 2*pts1, pts1, inputs, outputs) holding h[:, :, 2*pts1:] returns, each of the two reducing in
 * S = segments(level) segments in the matrix's documented order: the sequence r = i * nparts + p (p = 0 the oldest input
 * frame) is cut at floor(s * inputs * nparts / S), every segment is one float32 accumulator per bin summed over its r
 * ascending, and the segments are added as ((seg_0 + seg_1) + seg_2) + ...  (a matrix object created with
 * CLFA_PCONV_MATRIX_SEGS = S reduces so).  Then y_o[n] = yh_o[n] + yt_o[n - 2*pts1], one float32 addition with the head
 * as its first operand; before sample 2*pts1 the delayed tail is +0, and the addition is performed there too.  The
 * output bits do not depend on how the stream is cut into calls: a call of K blocks equals K calls of one block, in
 * output and in the state it leaves.  The packed DC / Nyquist rule applies per level, as in clfa_nupconv.
 * segments(level): the head's count is what the matrix's plan gives for the head's geometry (pts0 bins, 2m partitions,
 * inputs, outputs) on the device; the tail's is what it gives for one SLICE of the tail (pts0 bins, n1 partitions): that
 * is what a single-block call offers the multiply-accumulate (a plan of this object's own, from measurement).
 * CLFA_PCONV_MATRIX_SEGS (1..4096, read at creation) overrides both levels.  The definition goes through this accessor,
 * not through a plan.
 *
 * Schedule: clfa_nupconv's, with the inputs in front of the multiply-accumulate and the outputs behind it.  The phase is
 * position() mod m; the tail's forward transform (inputs rows) runs at phase 0 into ring frame w; every phase computes one
 * slice of pts0/2 16-byte items of the tail block for every output; the tail's inverse (outputs rows) runs after phase
 * m - 1 into the pending row, which is mixed into the head's output.  A call of one block: the stage kernel, the head's
 * forward into its ring frame, ONE k_nupm_mac launch of two jobs (the head's block, the tail's slice), one k_nupm_reduce
 * launch where a level has more than one segment, the head's inverse and the mix.  A call of several blocks runs the head
 * through the matrix's sub-batch launches over the whole call and the tail's slices between two period boundaries in one
 * launch.
 *
 * process_dev: row i of `in` at in + i*in_stride floats, row o of `out` at out + o*out_stride, nblocks*pts0 floats each;
 * any 4-byte aligned address, strides >= nblocks*pts0; nblocks == 0 succeeds and does nothing.  A bad argument, or an out
 * that overlaps in even partly: CLFA_INVALID_VALUE, the state untouched.  A call (or a reset) on a capturing stream:
 * CLFA_INVALID_OPERATION — the phase lives on the host.  One object runs on one stream at a time.  convolution: the same
 * on packed host rows, blocking.
 * push_ir / push_ir_dev: both levels' response spectra written in stream order.  At position() % m == 0 a push is exact in
 * clfa_nupconv's sense: at c = P*m it equals pushing the head object of the definition before its block c and the tail
 * object before its block P - 1 (block 0 for P = 0).  At another phase the tail block in progress sums its REMAINING
 * slices with the new responses: push at phase 0, or use the timed crossfade below, which is clean at any phase.
 * reset: the input history, the overlap-add tails and the blocks in progress are cleared, position() is 0, the responses
 * stay.
 *
 * Timed crossfade (push_ir_fade, push_ir_fade_dev): a change of responses without the step of a plain push, at any phase.
 * ir, row_stride and the row layout are those of push_ir / push_ir_dev.  Definition (clfa_nupconv's, with rows in place of
 * channels): let A be the response set in force at the push and B the pushed set; c = position() at the push (any phase);
 * block 0 the next head block processed; N = fade_blocks * pts0; n a sample's index counted from the first sample of block
 * 0; yA what this object would have produced without the push; yB what a second clfa_nupconv_matrix of the same geometry
 * AND THE SAME segments(0), segments(1) would produce if it had held B since its creation or last reset and had received
 * every input this object has received since then.  Both are complete outputs, head + pending tail, one float32 addition
 * with the head first.  Then
 *   for 0 <= n < N the output sample is  yA + g(n) * (yB - yA),  evaluated in float32 in that form (a subtraction, a
 *     multiplication, an addition, each rounded on its own, no contraction), with  g(n) = (float)n / (float)N  (IEEE
 *     division, round to nearest): exactly 0 at n = 0, rising linearly to (N-1)/N;
 *   from sample N on the output is yB, B is in force, fade_remaining() is 0, and the object is in every later bit the
 *     object that always held B.
 * The output does not depend on how the stream is cut into calls, during the fade or after it; a fade from A to A gives
 * the bits of no push at all.
 * State: the inputs' spectra rings, the stage rows and the forward transforms do not depend on the responses; both paths
 * share them and they are written once.  What depends on the responses exists twice during a fade: both levels' response
 * spectra, both levels' overlap-add tail pairs, the pending rows, both levels' single-block accumulators and partial
 * sums; on top of that a scratch of outputs x pts0 floats for the second path's head output.  All of the second set's
 * history is recomputed at the push from the rings alone with the plain path's kernels (k_nupm_mac over all items of a
 * block, k_nupm_reduce, the inverse), hence with its bits — a whole block in one multiply-accumulate has the bits of the
 * block computed slice by slice, because the segments cut the term sequence, not the bins: with P = c div m and s = c mod
 * m, the head's tail from head block c - 1 (c >= 1); the tail level's tail from tail block P - 3 (P >= 3); the pending
 * rows and the tail level's tail from tail block P - 2 (P >= 2); slices 0 .. s-1 of tail block P - 1 (P >= 1, s > 0).  A
 * block of negative index is not computed: its contribution is the +0 of a cleared row.  For this the tail's ring keeps
 * n1 + 2 frames per input (the sums walk the newest n1); the head's keeps its 2m, which head block c - 1 finds intact.
 * When the last fade block has been issued the sets exchange roles on the host, nothing is copied.  The second set is
 * allocated by the first fade push and kept for the next: A FADE DOUBLES THE RESPONSE MEMORY (the responses of 64 x 64
 * rows of 2^18 taps are 8 GB), and state_bytes() and workspace_bytes() count the second set from then on; until then they
 * are those of an object without fades, the tail ring's two more frames apart.
 * Schedule: a head block of a fade runs the head's forward transform (and the tail's at phase 0), the stage kernel, ONE
 * k_nupm_mac launch of up to four jobs (head and tail slice under A and under B), ONE k_nupm_reduce launch over the same
 * jobs, the two head inverses (A's into the output rows, B's into the scratch), k_nupc_fade_mix over the outputs rows
 * and, after phase m - 1, both tail inverses.  A call of K blocks that meets a fade runs the fade's blocks one at a time
 * and what follows the fade on the usual route.
 * Refusals (the state is untouched in each): fade_blocks < 1, fade_blocks * pts0 > 2^31 - 1 or any argument error of
 * push_ir_dev: CLFA_INVALID_VALUE; a fade push, a plain push_ir / push_ir_dev, or a reset while fade_remaining() > 0:
 * CLFA_INVALID_OPERATION; a fade push on a capturing stream: CLFA_INVALID_OPERATION.  The argument checks come before
 * the device is looked at; a failed object answers with its error. */
CLFA_API int clfa_nupconv_matrix_create(clfa_nupconv_matrix **pc, int device, int cvs, int pts0, int pts1, int inputs,
                                        int outputs);
CLFA_API void clfa_nupconv_matrix_destroy(clfa_nupconv_matrix *pc);
CLFA_API int clfa_nupconv_matrix_get_error(const clfa_nupconv_matrix *pc);
CLFA_API const char *clfa_nupconv_matrix_get_log(const clfa_nupconv_matrix *pc);
/* partitions of level 0 (the head: 2m) or 1 (the tail: n1); 0 for another level or a failed object */
CLFA_API int clfa_nupconv_matrix_nparts(const clfa_nupconv_matrix *pc, int level);
/* segments of the reduction over (input, partition) of level 0 or 1; 0 for another level or a failed object */
CLFA_API int clfa_nupconv_matrix_segments(const clfa_nupconv_matrix *pc, int level);
/* head blocks since creation or the last reset */
CLFA_API long clfa_nupconv_matrix_position(const clfa_nupconv_matrix *pc);
/* the state: both levels' rings, responses and tails, the stage rows and the pending tail output (+ a fade's second
 * responses, tails and pending rows) */
CLFA_API size_t clfa_nupconv_matrix_state_bytes(const clfa_nupconv_matrix *pc);
/* the workspaces: both levels' single-block accumulators and partial sums (allocated at creation) and the head's sub-batch
 * workspaces (none until a call of several blocks; grown by the call that needs more blocks than any before it; + a
 * fade's second accumulators and partial sums and its head rows) */
CLFA_API size_t clfa_nupconv_matrix_workspace_bytes(const clfa_nupconv_matrix *pc);
/* "k_nupm_mac" ("" for a failed object) */
CLFA_API const char *clfa_nupconv_matrix_kernel_name(const clfa_nupconv_matrix *pc);
CLFA_API int clfa_nupconv_matrix_push_ir(clfa_nupconv_matrix *pc, const float *ir); /* packed host rows, blocking */
CLFA_API int clfa_nupconv_matrix_push_ir_dev(clfa_nupconv_matrix *pc, const void *ir, long row_stride, void *stream);
CLFA_API int clfa_nupconv_matrix_push_ir_fade(clfa_nupconv_matrix *pc, const float *ir, long fade_blocks); /* packed host rows, blocking */
CLFA_API int clfa_nupconv_matrix_push_ir_fade_dev(clfa_nupconv_matrix *pc, const void *ir, long row_stride, long fade_blocks,
                                                  void *stream);
/* head blocks of the fade not yet processed; 0 = none (and for a NULL handle) */
CLFA_API long clfa_nupconv_matrix_fade_remaining(const clfa_nupconv_matrix *pc);
CLFA_API int clfa_nupconv_matrix_process_dev(clfa_nupconv_matrix *pc, void *out, long out_stride, const void *in,
                                             long in_stride, long nblocks, void *stream);
CLFA_API int clfa_nupconv_matrix_convolution(clfa_nupconv_matrix *pc, float *out, const float *in, long nblocks);
CLFA_API int clfa_nupconv_matrix_reset(clfa_nupconv_matrix *pc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CLFFT_AMD_H */
