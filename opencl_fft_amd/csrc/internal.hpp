// internal.hpp — launcher prototypes shared by the kernel files and the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_device.hpp"
#include "fft_route.hpp"   // FftMode, kLdsMaxLog, kMaxLog and which kernels a plan runs for a batch

namespace clfa {

// n = 8192 uses lane-addressed twiddle tables instead of the half table (fft_device.hpp, LaneTab13):
// [W_256^(j t), j, t < 16 | W_4096^(2^k j mod 4096), k < 4, j < 256 | W_8192^t, t < 512]; the first
// kLane13Lds entries live in LDS
constexpr bool kLdsTwoLevel(int logn) { return logn >= 13; }
constexpr int kLane13Lds = 1280, kLane13Size = 1792;
// ... in LDS the rows of the 16 x 16 part are kRow16Stride entries apart: the sixteen lanes of a ds_read_b128 group read
// sixteen DIFFERENT rows (row = tid & 15); 16 entries = 32 dwords apart they would fall on two groups of four banks (an
// 8-way conflict, 32 LDS cycles per read — rocprofv3 round 4: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.41-0.46 for
// config 3's kernel); 18 entries = 36 dwords apart they cover the 64 banks exactly once (MI355X_MICROARCH.md, LDS table)
constexpr int kRow16Stride = kRow16StrideDev;   // (fft_device.hpp, which compiles on the host alone, has the value)
static_assert(kRow16Stride >= 16 && kRow16Stride % 2 == 0, "rows stay 16-byte aligned");
constexpr int kRow16Lds = 16 * kRow16Stride;            // the s256 part follows
constexpr int kLaneLds = kRow16Lds + (kLane13Lds - 256);   // entries of the LDS copy
// LDS index of entry i < kLane13Lds of the global table
__host__ __device__ constexpr int lane_lds_index(int i) { return i < 256 ? (i >> 4) * kRow16Stride + (i & 15) : i + (kRow16Lds - 256); }
// the 16384-point chains of k_rfft_2x<14> (packed real size 65536: 1024 lanes, passes 16 x 16 x 16 x 4, fft_device.hpp
// LaneTab14): the same LDS part, then [W_16384^t | W_16384^(2 t) | W_16384^(3 t)], t < 1024
constexpr int kLds14Log = 14, kLane14Size = kLane13Lds + 3 * 1024;

struct FftTables {      // all device pointers, owned by the plan
  const cpx *half = nullptr;   // W_n^k, k < n/2, forward sign (LDS path; n = complex length)
  const cpx *w2 = nullptr;     // r2c table (cl_fft.cpp:233-238), sign of the plan's direction, m entries
  const cpx *four = nullptr;   // four-step tables: [half N1 | half N2 | lo | hi]
  const cpx *res16 = nullptr;  // n = 65536 only: tables of the resident kernel (kRes16TabSize entries)
};

struct DeviceInfo {
  int device = 0;
  int num_cus = 256;
};

// single-workgroup LDS FFT, n = 2^logn <= 2^kLdsMaxLog.  mode selects the fused
// r2c epilogue / c2r prologue.  scale: multiply by 1/n (forward plans).
// out_off (here and below): the results go to data + out_off complex elements — 0 = in place, otherwise a destination
// that does not overlap the source (clfa_fft_exec_dev_oop); the source is only read
hipError_t launch_fft_lds(int logn, bool fwd, int mode, bool scale, cpx *data, const FftTables &t,
                          long batch, const DeviceInfo &di, hipStream_t s, long out_off = 0);
// packed real size 65536 (n = 32768): two runs of the 16384-point machinery per transform, radix-2 step and pair
// map in registers; t.half = the n = 16384 lane tables (kLane14Size), t.w2 = the plan's r2c table (n entries)
hipError_t launch_rfft_lds15(bool fwd, cpx *data, const FftTables &t, long batch, const DeviceInfo &di, hipStream_t s,
                             long out_off = 0);
// packed real size 32768 the same way on two 8192-point runs (two 512-lane workgroups per CU); t.half = the n = 8192
// lane tables (kLane13Size), t.w2 = the plan's r2c table
hipError_t launch_rfft_2x13(bool fwd, cpx *data, const FftTables &t, long batch, const DeviceInfo &di, hipStream_t s,
                            long out_off = 0);
// complex n = 16384 as two 8192-point runs + a radix-2 step in registers; t.half = the n = 8192 lane tables
// (kLane13Size) followed by W_16384^t, t < 512
hipError_t launch_cfft_2x13(bool fwd, bool scale, cpx *data, const FftTables &t, long batch, const DeviceInfo &di,
                            hipStream_t s, long out_off = 0);

// four-step FFT, n = 2^logn in (2^kLdsMaxLog, 2^kMaxLog]; scratch = fourstep_grid() * n complex.  Which of its kernels
// a batch runs (the cols + rows pair, k_fft_4step, or for n = 65536 the resident kernel below, whose slots are the first
// kRes16SlotBytes * grid bytes of the scratch) is fft_route.hpp's decision: fourstep_spread()
int fourstep_grid(const DeviceInfo &di);
hipError_t launch_fft_4step(int logn, bool fwd, bool scale, cpx *data, cpx *scratch, const FftTables &t, long batch,
                            const DeviceInfo &di, hipStream_t s, long out_off = 0);
int fourstep_split(int logn, int *logn1, int *logn2, int *loglo);
// n = 65536, the whole intermediate resident on the CU (fft_resident.hip): one HBM pass, no scratch.
// tabs: kRes16TabSize entries, forward sign: [W_256^(t j), t, j < 16 | W_n^k, k < 256 | W_256^k, k < 256 |
// W_4096^(m k mod 4096), m = 1, 2, 4, 8, k < 256]
constexpr int kRes16TabSize = 1792;
// slots: 32 KiB per workgroup, grid = min(batch, CUs) workgroups (kRes16SlotBytes each)
constexpr size_t kRes16SlotBytes = 32768;
// out == data: in place (what every plan does); out != data: out of place (tools/res16_probe.hip times both; profiles/oop_r04.txt)
// ctr (optional): the counters of the shared assignment (fft_resident.hip, k_fft_res16<..., DYN>), kRes16CtrBytes that
// were zero before the first launch; every launch leaves them zero.  Like the slots they serve one launch at a time.
// Without them, and for batches where xcd_shared_ok() (fft_device.hpp) says no, the static assignment runs.
// rec (optional, a measurement aid): one ResRecord per workgroup, written as the workgroup exits.
constexpr size_t kRes16CtrBytes = 9 * 128;
// a plan keeps one line of kRes16GuardWord in front of its counters and one behind them: a counter access that strays shows
// there (clfa_fft_balance_counters)
constexpr size_t kRes16GuardBytes = 128;
constexpr unsigned kRes16GuardWord = 0xA5A5A5A5u;
struct alignas(16) ResRecord {
  unsigned count;              // transforms the workgroup processed
  unsigned xcd;                // workgroup index % 8
  unsigned long long stamp;    // wall clock at its exit
};
hipError_t launch_fft_res16(bool fwd, bool scale, const cpx *data, cpx *out, cpx *slots, const cpx *tabs, long batch,
                            const DeviceInfo &di, hipStream_t s, unsigned *ctr = nullptr, ResRecord *rec = nullptr);
// packed real transforms of size 131072, forward: the same kernel with the reference's pair map inside its second
// phase (w2 = the plan's pair twiddles, 65536 entries) — one HBM pass instead of the transform + k_r2c_pack
hipError_t launch_rfft_res16(const cpx *data, cpx *out, cpx *slots, const cpx *tabs, const cpx *w2, long batch,
                             const DeviceInfo &di, hipStream_t s);
// ... and the inverse: the reference's iconv map inside the first phase (w2 = the inverse plan's pair twiddles)
hipError_t launch_crfft_res16(const cpx *data, cpx *out, cpx *slots, const cpx *tabs, const cpx *w2, long batch,
                              const DeviceInfo &di, hipStream_t s);
// n = 2^17 .. 2^kBigMaxLog (extension: the reference overflows above 65536): columns + rows + transpose
constexpr int kBigMaxLog = 24;
struct BigGeom {
  int logn, logn1, logn2;   // n = 2^logn1 x 2^logn2
  bool two_run;                    // two-pass sizes: 1024-point columns / rows as two 512-point runs (two workgroups per CU)
};
int big_split(int logn, BigGeom *g);
// bigtabs: [half N1 | W_n^k, k < 128 | W_n^(128 k), k < 128 | W_n^(16384 k), k < n / 16384]; sub: tables of the 2^logn2 row transform; scratch holds `batch`
// transforms (batch <= 65535), scratch2 the row transform's own workspace (logn2 > kLdsMaxLog)
// (out: where the last pass writes; data itself is only read)
hipError_t launch_fft_big(const BigGeom &g, bool fwd, bool scale, cpx *data, cpx *out, cpx *scratch, cpx *scratch2,
                          const cpx *bigtabs, const FftTables &sub, long batch, const DeviceInfo &di, hipStream_t s);

// stand-alone pack / unpack (reference kernels conv / iconv) for M above the LDS path
hipError_t launch_r2c_pack(cpx *data, const cpx *w2, int m, long batch, hipStream_t s, long out_off = 0);
hipError_t launch_c2r_unpack(cpx *data, const cpx *w2, int m, long batch, hipStream_t s, long out_off = 0);

// arbitrary (non power-of-two) complex lengths, an extension: Bluestein's algorithm around two m-point
// power-of-two transforms, m >= 2 n - 1 (fft_aux.inc); n up to kBlueMaxN
constexpr int kBlueMaxN = 1 << 22;
hipError_t launch_blue_lds(int m, const cpx *x, cpx *y, const cpx *w, const cpx *bt, const cpx *tab, int n, float scale,
                           long batch, const DeviceInfo &di, hipStream_t s);
hipError_t launch_blue_pre(const cpx *x, const cpx *w, cpx *a, int n, int m, long batch, hipStream_t s);
hipError_t launch_blue_mul(cpx *a, const cpx *bt, int m, long batch, hipStream_t s);
hipError_t launch_blue_post(const cpx *a, const cpx *w, cpx *x, int n, int m, float scale, long batch, hipStream_t s);

// reference `reorder` kernel as an op
hipError_t launch_reorder(cpx *out, const cpx *in, int logn, long batch, hipStream_t s);

// ---- partitioned convolution --------------------------------------------------
struct PconvGeom {
  int logb;      // log2(bins), bins = pts
  int bins;
  int nparts;
  int channels;
};
// input block (channels x pts floats) -> zero-padded 2*pts real FFT -> packed
// spectrum frame `frame` of ring (channels x nparts x bins complex).  Unscaled,
// reference pack (cl_conv_kernels.h:46-85).
// in_b / ring_b / frame_b: optional second input of a time-varying block, transformed by the same launch
hipError_t launch_pconv_forward(const PconvGeom &g, const float *in, long in_stride, cpx *ring, int frame,
                                const cpx *half, const cpx *w2f, hipStream_t s, const float *in_b = nullptr,
                                cpx *ring_b = nullptr, int frame_b = 0);
// acc = sum_p A[(wp+p)%nparts] (.) B[p]  (cl_conv_kernels.h:102-118), acc: channels x bins complex
int pconv_mac_split(const PconvGeom &g);   // partial accumulators the MAC writes (acc must hold that many)
// reduce = false leaves the pconv_mac_split() partial sums for launch_pconv_inverse(nsplit) to add up
hipError_t launch_pconv_mac(const PconvGeom &g, const cpx *ringA, const cpx *ringB, int wp, cpx *acc,
                            hipStream_t s, bool reduce = true);
// acc -> c2r -> inverse FFT -> overlap-add (cl_conv_kernels.h:87-100,120-124); out channels x pts,
// tail channels x pts (unscaled second half kept for the next block)
hipError_t launch_pconv_inverse(const PconvGeom &g, const cpx *acc, float *tail, float *out,
                                const cpx *half, const cpx *w2i, hipStream_t s, int nsplit = 1);
// one launch per block (forward + MAC + inverse in one workgroup per channel); used when
// one launch per block for a FEW channels (pconv_coop.hip, k_pconv_coop): 2^logs bin slices x sparts segments of
// the partition axis per channel (logs = -1: the kernel does not apply); xacc: channels x sparts x bins complex
// (hand-over of the accumulator slices), counters: one zero-initialised unsigned per channel (returned to zero by
// every launch)
struct PconvCoop {
  int logs, sparts;
};
PconvCoop pconv_coop_plan(const PconvGeom &g, const DeviceInfo &di);
hipError_t launch_pconv_coop(const PconvGeom &g, PconvCoop c, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                             float *tail, float *out, int frame1, int frame2, int wp, const cpx *half, const cpx *w2f,
                             const cpx *w2i, cpx *xacc, unsigned *counters, int num_cus, hipStream_t s);
// pconv_fused_ok(): bins 512..4096 and enough channels to fill the chip
bool pconv_fused_ok(const PconvGeom &g, const DeviceInfo &di);
hipError_t launch_pconv_fused(const PconvGeom &g, const float *in1, const float *in2, cpx *ringA, cpx *ringB,
                              float *tail, float *out, int frame1, int frame2, int wp, const cpx *half,
                              const cpx *w2f, const cpx *w2i, hipStream_t s, bool deep = false);   // deep: fewer channels than CUs
// K consecutive blocks of every channel in four launches (pconv_blocks.hip), bins 32..4096: in1 / in2 / out point at
// block 0 of the sub-batch (row c at c * stride floats); X, Y (and XB, time-varying) are channels x cap x bins complex
// workspaces, tail_ws channels x bins floats.  w / w2: the object's wp / wp2 before the sub-batch; K <= cap, and
// K <= nparts when in2 is set.  The rings and the tail are written only by the last launch, after every read.
struct PconvBlocks {
  PconvGeom g;
  int K = 0, cap = 0, w = 0, w2 = 0;
  int kt = 4;     // outputs per MAC tile: pconv_blocks_tile()
  int run = 8;    // blocks per inverse run
  const float *in1 = nullptr, *in2 = nullptr;
  long in_stride = 0, out_stride = 0;
  float *out = nullptr;
  int aligned_in = 1, aligned_out = 1;   // every row start 8-byte aligned
  cpx *ringA = nullptr, *ringB = nullptr;
  float *tail = nullptr;
  cpx *X = nullptr, *XB = nullptr, *Y = nullptr;
  float *tail_ws = nullptr;
  const cpx *half = nullptr, *w2f = nullptr, *w2i = nullptr;
};
int pconv_blocks_tile(const PconvGeom &g, const DeviceInfo &di);
hipError_t launch_pconv_blocks(const PconvBlocks &a, hipStream_t s);
constexpr int kPconvBlocksMinLog = 5, kPconvBlocksMaxLog = 12;
// the forward / inverse launches of a sub-batch on their own (pconv_blocks.hip), for the convolution matrix
hipError_t launch_pconvb_forward(int logb, const float *in, long in_stride, cpx *X, int K, int cap, int channels, int aligned,
                                 const cpx *half, const cpx *w2f, hipStream_t s);
hipError_t launch_pconvb_inverse(int logb, const cpx *Y, const float *tail, float *tail_out, float *out, long out_stride, int K,
                                 int cap, int R, int channels, int aligned, const cpx *half, const cpx *w2i, hipStream_t s);
// Convolution matrix (pconv_matrix.hip): y_o = sum_i x_i * h_{o,i}, K consecutive blocks of every input per sub-batch.
// Responses H: outputs x inputs x nparts x bins complex, partition q of row (o, i) at ((o * inputs + i) * nparts + q) * bins.
// The MAC walks the reduction sequence r = i * nparts + p (p = 0 pairs with partition nparts - 1, the oldest input frame)
// in `segs` fixed segments [r_s, r_{s+1}), r_s = floor(s * inputs * nparts / segs); segment 0 writes Y, segment s > 0 the
// partial P[s - 1]; with segs > 1 a reduce launch adds them to Y in ascending s.
struct PconvMatrixPlan {
  int kt = 4;     // outputs per MAC tile (4 or 16)
  int segs = 1;   // segments of the reduction over (input, partition)
};
struct PconvMatrixArgs {
  int logb = 0, bins = 0, nparts = 0, inputs = 0, outputs = 0;
  PconvMatrixPlan plan;
  int K = 0, cap = 0, w = 0;
  int run = 8;    // blocks per inverse run
  const float *in = nullptr;
  float *out = nullptr;
  long in_stride = 0, out_stride = 0;
  int aligned_in = 1, aligned_out = 1;   // every row start 8-byte aligned
  const cpx *H = nullptr;
  cpx *ringA = nullptr;                  // inputs x nparts x bins
  float *tail = nullptr;                 // outputs x bins
  cpx *X = nullptr, *Y = nullptr, *P = nullptr;   // inputs x cap, outputs x cap, (segs - 1) x outputs x cap frames
  float *tail_ws = nullptr;              // outputs x bins
  const cpx *half = nullptr, *w2f = nullptr, *w2i = nullptr;
  // a timed crossfade to a second response set (launch_pconv_matrix_fade / _prime): the set, its tails and workspaces
  const cpx *H2 = nullptr;
  float *tail2 = nullptr;                // outputs x bins
  cpx *Y2 = nullptr, *P2 = nullptr;      // as Y, P
  float *tail_ws2 = nullptr;             // outputs x bins
  float *mix = nullptr;                  // the second path's samples: outputs rows of cap * bins floats
  long fade_pos = 0, fade_len = 0;       // blocks of the fade before this sub-batch, blocks of the whole fade
  bool two_mac = false;                  // two launches of the plain MAC instead of the two-response one
};
PconvMatrixPlan pconv_matrix_plan(int bins, int nparts, int inputs, int outputs, const DeviceInfo &di);
hipError_t launch_pconv_matrix(const PconvMatrixArgs &a, hipStream_t s);
// A sub-batch inside a fade (K <= fade_len - fade_pos): both paths over the shared ring, the second one's samples mixed
// into `out` with g(n) = (float)n / (float)(fade_len * bins), n counted from the fade's first sample; ring, tail and tail2
// committed.  _prime: tail2 = the second half of the block before the next one under H2, from ring A alone.
hipError_t launch_pconv_matrix_fade(const PconvMatrixArgs &a, hipStream_t s);
hipError_t launch_pconv_matrix_prime(const PconvMatrixArgs &a, hipStream_t s);
constexpr int kPconvMaxLogBins = 15;   // pts up to 32768 (the reference harness' largest, csound/tests.py:13)
// ends of the composed chain used when bins exceed the LDS FFT sizes
hipError_t launch_pconv_pad(const float *in, long in_stride, cpx *work, int bins, int channels, hipStream_t s);
hipError_t launch_pconv_olap(const float *work, float *tail, float *out, int bins, int channels, hipStream_t s);

// ---- short-time transforms (stft_kernels.hip) --------------------------------------
// packed real size 2^(logn + 1), logn 5..kLdsMaxLog.  forward: channels rows of `signal` (row c at c * stride floats) ->
// spec_out, nframes = channels * F frames of n complex; inverse: spec_in (nframes frames) -> rows of `out`, L = (F - 1) hop
// + size floats each.  window: size floats; cum (inverse, normalize only): [lo | hi] running sums of window^2 along steps
// of hop (2 * size floats); half / w2: the Clrfft tables of the direction.  aligned8: every frame start is 8-byte aligned.
struct StftArgs {
  int logn = 0;
  bool forward = true;
  int hop = 1, F = 0;
  long channels = 0, nframes = 0, stride = 0;
  bool aligned8 = true;
  int normalize = 0;
  int grid_max = 0;                // cap on a launch's workgroups (CLFA_STFT_GRID_MAX, 0 = none)
  const float *signal = nullptr;
  float *out = nullptr;
  const cpx *spec_in = nullptr;
  cpx *spec_out = nullptr;
  const float *window = nullptr;
  const double *cum = nullptr;     // the envelope's running sums (stft_plan.hpp)
  const cpx *half = nullptr, *w2 = nullptr;
};
hipError_t launch_stft(const StftArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- phase vocoder on the Stft spectra (pvoc_kernels.hip) ---------------------------
// spectra: channels x F x M complex (the packed layout); frames: channels x F x (M + 1) x (amp, freq in Hz).
constexpr int kPvocChunk = 64;   // frames per chunk of the synthesis' phase scan (fixed: clfa_pvoc_scan_chunk)
struct PvocArgs {
  int M = 0, channels = 0;
  long F = 0;                      // frames per channel in the caller's buffers (the channels' rows are F frames apart)
  const cpx *spec_in = nullptr;    // analysis
  float *frames_out = nullptr;
  cpx *prev = nullptr;             // channels x (M + 1): z of the frame before the call's first
  const cpx *etab = nullptr;       // M + 1 expected advances e[k]
  float sh = 0.f, srs = 0.f;       // size / hop, sr / size
  const float *frames_in = nullptr;   // synthesis
  cpx *spec_out = nullptr;
  unsigned *theta = nullptr;       // channels x (M + 1) phases in 2^-32 turn
  unsigned *sums = nullptr;        // channels x nchunks x (M + 1): the chunks' sums, then their bases
  float kf = 0.f;                  // hop / sr
};
// one launch: frames of every channel, prev read by the lanes of frame 0 and replaced by the same lanes
hipError_t launch_pvoc_analyze(const PvocArgs &a, const DeviceInfo &di, hipStream_t s);
// frames [f0, f0 + nf) of every channel, nf <= the workspace's chunks x kPvocChunk: the chunks' sums of increments, then
// (one lane per channel and bin) their bases in place and the new theta, then the walk that writes the spectra
hipError_t launch_pvoc_synth(const PvocArgs &a, long f0, long nf, const DeviceInfo &di, hipStream_t s);

// ---- oscillator-bank resynthesis of (amp, freq) frames (pvoc_adsyn.hip) -------------
constexpr int kAdsynTile = 256;    // oscillators per LDS tile of k_adsyn_osc = its lanes (clfa_pvoc_adsyn_tile_bins)
struct PvocAdsynArgs {
  int M = 0, channels = 0, hop = 0;
  long F = 0;                          // frames per channel in the caller's buffers
  const float *frames = nullptr;       // channels x F x (M + 1) x (amp, freq)
  const float *fmod = nullptr;         // F, or NULL
  int first = 0, nbins = 0, step = 1;  // the oscillators are the bins first + i step, i < nbins
  float gain = 1.f, ks = 0.f;          // ks = 1 / sr
  unsigned long long *phase = nullptr; // the state, per channel and bin: P, W, A
  int *w = nullptr;
  float *amp = nullptr;
  unsigned long long *sums = nullptr;  // workspace: per channel, chunk and oscillator the chunk sums, then bases
  int *w0 = nullptr;                   // workspace: per channel and oscillator, the endpoint the sub-batch starts from
  float *a0 = nullptr;
  const float *ramp = nullptr;         // w_j = (float)((double)j / hop), j = 1..hop
  float *signal = nullptr;             // channels rows of F hop floats, sstride apart
  long sstride = 0;
  int grid_max = 0;                    // > 0: at most this many workgroups
};
// frames [f0, f0 + nf) of every channel, nf <= the workspace's chunks x kPvocChunk: k_adsyn_sums, k_adsyn_scan, k_adsyn_osc
hipError_t launch_pvoc_adsyn(const PvocAdsynArgs &a, long f0, long nf, const DeviceInfo &di, hipStream_t s);

// ---- what the launches of the frame operations below share (filled by pvoc_host.cpp's pvoc_frames_args) ----
struct PvocFramesArgs {
  int M = 0, channels = 0;
  long F = 0;                      // frames per channel of the output (and of every input but the read's)
  int logn = 0;                    // log2(M): the envelope kernels' transform length (complex)
  const cpx *half = nullptr, *w2 = nullptr;   // the envelope kernels: the Clrfft tables of size (forward sign)
  int grid_max = 0;                // > 0: at most this many workgroups
};

// ---- operations on (amp, freq) frames (pvoc_ops.hip): pitch scale, frequency shift, timed read ----
enum PvocOp { PVOC_SCALE = 0, PVOC_SHIFT = 1, PVOC_READ = 2 };
struct PvocOpsArgs : PvocFramesArgs {
  int op = PVOC_SCALE;
  long Fin = 0;                    // read: input frames per channel
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  cpx *out = nullptr;
  const float *par = nullptr;      // F values: scale, shift in Hz, or positions
  int lowest = 1, keepform = 0, coefs = 1;
  float gain = 1.f, cf = 0.f, bpf = 0.f;   // sr / size, size / sr
};
// one launch: k_pvoc_map, k_pvoc_formant<logn> (keepform) or k_pvoc_read
hipError_t launch_pvoc_ops(const PvocOpsArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- operations on two streams of (amp, freq) frames (pvoc_pair.hip) ------------------
enum PvocPairOp { PVOC_CROSS = 0, PVOC_MORPH = 1, PVOC_FILTER = 2, PVOC_MIX = 3, PVOC_VOCODE = 4 };   // CLFA_PVOC_*
struct PvocPairArgs : PvocFramesArgs {
  int op = PVOC_CROSS;
  const cpx *a = nullptr, *b = nullptr;   // frames as (amp, freq) pairs; they may overlap
  cpx *out = nullptr;
  const float *p = nullptr, *q = nullptr;   // F values each (mix: not read)
  int coefs = 1;                   // vocode
};
// one launch: k_pvoc_pair, or k_pvoc_vocode<logn> for PVOC_VOCODE
hipError_t launch_pvoc_pair(const PvocPairArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- operations that reshape one stream of (amp, freq) frames along the bins (pvoc_shape.hip) ----
enum PvocShapeOp { PVOC_BAND = 0, PVOC_MASK = 1, PVOC_STENCIL = 2, PVOC_ARP = 3, PVOC_LOCK = 4, PVOC_WARP = 5 };   // CLFA_PVOC_*
struct PvocShapeArgs : PvocFramesArgs {
  int op = PVOC_BAND;
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  cpx *out = nullptr;
  const float *par = nullptr;      // F rows of 4 values
  const float *table = nullptr;    // M + 1 values (mask, stencil; the others do not read it)
  int reject = 0;                  // band
  int lowest = 1, coefs = 1;       // warp
  float bpf = 0.f;                 // size / sr
};
// one launch: k_pvoc_shape (ops 0..3), k_pvoc_lock or k_pvoc_warp<logn>
hipError_t launch_pvoc_shape(const PvocShapeArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- operations along a stream of (amp, freq) frames, with carried state (pvoc_time.hip) ----
enum PvocTimeOp { PVOC_BLUR = 0, PVOC_SMOOTH = 1, PVOC_FREEZE = 2 };   // CLFA_PVOC_*
struct PvocTimeArgs : PvocFramesArgs {
  int op = PVOC_BLUR;
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  cpx *out = nullptr;
  const float *p = nullptr, *q = nullptr;   // F values each (blur: q is not read)
  cpx *state = nullptr;            // blur: the history, channels x L frames, oldest first; smooth: y; freeze: held
  cpx *spare = nullptr;            // blur: as the history
  int max_frames = 1;              // blur: L = max_frames - 1
};
// the main launch, then what commits the state on the same stream: blur k_pvoc_tail into the spare and a copy of the
// spare over the history, freeze k_pvoc_tail of the output's last frame into held; smooth commits in its own launch
hipError_t launch_pvoc_time(const PvocTimeArgs &a, const DeviceInfo &di, hipStream_t s);
// `frames` frames of EMPTY bins (cf = sr / size): what the three states start from
hipError_t launch_pvoc_time_fill(cpx *dst, long frames, int M, float cf, hipStream_t s);
// dst (channels x (M + 1) pairs) = frame F - 1 of src (channels x F frames), F >= 1: k_pvoc_tail, the freeze's commit
hipError_t launch_pvoc_time_last(const cpx *src, long F, cpx *dst, int channels, int M, int grid_max, const DeviceInfo &di,
                                 hipStream_t s);
// dst (channels x rows frames) = the last `rows` frames of the stream hist ++ src per channel (hist: channels x L frames,
// read only where rows > F, and then rows <= L; src: channels x F frames): k_pvoc_tail, a history's commit into its spare
hipError_t launch_pvoc_time_tail(const cpx *hist, int L, const cpx *src, long F, cpx *dst, int rows, int channels, int M,
                                 int grid_max, const DeviceInfo &di, hipStream_t s);

// ---- per-bin delay with feedback along a stream of (amp, freq) frames, with carried state (pvoc_delay.hip) ----
struct PvocDelayArgs : PvocFramesArgs {
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  cpx *out = nullptr;
  const int *delays = nullptr;     // M + 1 values, shared by the channels, clamped to 0 .. L
  const float *feedback = nullptr; // M + 1 values, or NULL: none
  cpx *xhist = nullptr, *yhist = nullptr;   // the last L input / output frames per channel, oldest first
  cpx *spare = nullptr;            // as one history
  int L = 0;
};
// k_pvoc_delay (feedback NULL) or k_pvoc_delay_fb, which only read the histories, then their commits on the same stream:
// for xhist and then for yhist, k_pvoc_tail into the spare and a copy of the spare over the history
hipError_t launch_pvoc_delay(const PvocDelayArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- per-frame descriptors of a stream of (amp, freq) frames, with carried state (pvoc_desc.hip) ----
struct PvocDescArgs : PvocFramesArgs {   // F: also the rows per channel of desc
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  float *desc = nullptr;           // channels x F x 8
  cpx *last = nullptr;             // the state: channels x (M + 1) pairs, the stream's previous frame (the amps are read)
  int lo = 0, hi = 0;              // the range of bins, 0 <= lo <= hi <= M
  int rectify = 0;
  float cf = 0.f;                  // sr / size
};
// k_pvoc_desc<min(M, 256)>, which only reads the state, then its commit on the same stream (k_pvoc_tail)
hipError_t launch_pvoc_desc(const PvocDescArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- the N loudest bins of every frame of a stream of (amp, freq) frames (pvoc_trace.hip) ----
struct PvocTraceArgs : PvocFramesArgs {
  const cpx *in = nullptr;         // frames as (amp, freq) pairs
  cpx *out = nullptr;
  const float *n = nullptr;        // F values, shared by the channels
  int *bins = nullptr;             // NULL, or channels x F x list_n: the bins kept, ascending, then -1
  int list_n = 0;
  int lo = 0, hi = 0;              // the range of bins, 0 <= lo <= hi <= M
  int residual = 0;                // the complement: the selected bins silenced, the others kept
};
// one launch: k_pvoc_trace<min(M, 256)>
hipError_t launch_pvoc_trace(const PvocTraceArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- stereo demix by azimuth of two streams of (amp, freq) frames, with the azimuth profile (pvoc_demix.hip) ----
struct PvocDemixArgs : PvocFramesArgs {
  const cpx *l = nullptr, *r = nullptr;   // the left and the right channel's frames as (amp, freq) pairs; they may overlap
  cpx *out = nullptr;
  const float *par = nullptr;      // F rows of (pos, width), shared by the channels
  float *az = nullptr;             // NULL, or channels x F x (2 points + 1): the azimuth profile
  int points = 1;                  // P, 1..1024: the gains 0, 1/P, ..., 1 of either side
  int lo = 0, hi = 0;              // the range of bins, 0 <= lo <= hi <= M
};
// one launch: k_pvoc_demix, or k_pvoc_demix_az<log2 M> where az is given
hipError_t launch_pvoc_demix(const PvocDemixArgs &a, const DeviceInfo &di, hipStream_t s);

// ---- direct convolution ----------------------------------------------------------
struct DconvPlan {
  int C;    // taps per workgroup
  int G;    // chunks of the tap axis (grid x)
  int VB;   // output blocks (grid y): block y takes the tiles of 64 outputs y, y + VB, ...
};
DconvPlan dconv_plan(int irsize, int vsize);
// one block: out[0..vsize) from the rings as they stand with in1 (and in2) written at wp; files the block in the rings.
// part: G x vsize floats, counters: VB zeroed words (both only touched when G > 1).  out must not overlap in1 / in2.
hipError_t launch_dconv_block(const DconvPlan &pl, float *out, const float *in1, const float *in2, float *del, float *coefs,
                              float *part, unsigned *counter, int irsize, int vsize, int wp, int num_cus, hipStream_t s);

// ---- direct convolution, many blocks and channels per call (dconv_blocks.hip) -------
constexpr int kDconvbChunk = 256;    // taps per staged window and per partial accumulator
constexpr int kDconvbSeg = 4096;     // taps per segment: longer responses are split (fixed at creation)
constexpr int kDconvbMaxSegs = 64;   // ... into at most this many segments
struct DconvBlocksPlan {
  int segs = 1;      // segments of the tap axis (grid z); > 1: partial sums in a workspace, summed by a second launch
  int seg_len = 0;   // taps per segment, a multiple of kDconvbChunk
  int force_r = 0;   // outputs per lane, 2 or 8; 0: the launcher picks by the size of the launch (the bits are the same)
};
DconvBlocksPlan dconv_blocks_plan(int irsize);
struct DconvBlocksArgs {
  DconvBlocksPlan plan;
  int irsize = 0, end = 0, channels = 1, wp = 0;
  long L = 0;                           // outputs per channel in this launch (whole blocks)
  long in_stride = 0, out_stride = 0;   // floats between the channels' rows
  const float *in1 = nullptr, *coefs = nullptr;
  float *out = nullptr, *del = nullptr;
  float *part = nullptr;                // segs x channels rows of part_stride >= L floats (segs > 1)
  long part_stride = 0;
};
// static form: out rows from the rings at wp and the input rows, then the rows' last `end` samples filed in the delay
// rings (the caller advances wp).  out must not overlap in1.
hipError_t launch_dconv_blocks(const DconvBlocksArgs &a, const DeviceInfo &di, hipStream_t s);

}  // namespace clfa
