// pconv_launch.hpp — the launchers of the partitioned convolution (pconv_chain.hip, pconv_coop.hip, pconv_blocks.hip,
// pconv_matrix.hip, pconv_nup.hip, pconv_nupm.hip) as the convolutions' hosts (pconv_host.cpp, pconv_matrix_host.cpp,
// nupconv_host.cpp) see them: PconvGeom and the per-block launches, the
// cooperative and the fused block, the many-block sub-batch (PconvBlocks), the convolution matrix (PconvMatrixArgs), the
// tail level of the non-uniform partitioning (launch_nupc_*), its matrix form (launch_nupm_*) and the ends of the composed
// chain.
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

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
  long in2_stride = 0;                   // rows of in2 that lie otherwise than in1's (0 / -1: as in1's): then in2 is
  int aligned_in2 = -1;                  // transformed by a forward launch of its own
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
// Non-uniformly partitioned convolution, the tail level (pconv_nup.hip).  stage / pend: channels x pts1 floats; off and n
// (multiples of 32, off + n <= pts1) are the stream's position in the tail block and the call's samples there; in / out
// point at the first of them (row c at c * stride floats, any 4-byte aligned address and stride).
hipError_t launch_nupc_stage(const float *in, long in_stride, float *stage, int pts1, int off, int n, int channels,
                             hipStream_t s);
// ... and two sets of rows (x and a time-varying second input) in one launch, each into its own stage row
hipError_t launch_nupc_stage2(const float *in, long in_stride, float *stage, const float *in_b, long in_b_stride, float *stage_b,
                              int pts1, int off, int n, int channels, hipStream_t s);
// The forward transforms of one level (bins = 1 << logb) for a time-varying block, one or two jobs in one launch: row ch of
// the job (bins floats at src + ch * stride, any 4-byte aligned address; aligned: every row start 8-byte aligned) ->
// the packed spectrum at frame + ch * frames * bins, with launch_pconvb_forward's bits.  copy (8-byte aligned, or NULL):
// the row's samples are stored at copy + ch * copy_stride as they are loaded.  frame == NULL: the job only copies.
struct NupcFwdJob {
  const float *src = nullptr;
  long stride = 0;
  int aligned = 0;
  cpx *frame = nullptr;
  int frames = 0;
  float *copy = nullptr;
  long copy_stride = 0;
};
hipError_t launch_nupc_fwd(int logb, const NupcFwdJob *jobs, int njobs, int channels, const cpx *half, const cpx *w2f, hipStream_t s);
// out = out + pend[off .. off + n): out holds the head's samples
hipError_t launch_nupc_mix(float *out, long out_stride, const float *pend, int pts1, int off, int n, int channels,
                           hipStream_t s);
// a fade's block: a = out + pendA[off .. off + n), b = headB + pendB[off .. off + n), out = a + g * (b - a), each operation
// rounded on its own, g = (float)(n0 + k) / N for sample k of the row; headB: channels x n floats, the second path's head
hipError_t launch_nupc_fade_mix(float *out, long out_stride, const float *headB, const float *pendA, const float *pendB, int pts1,
                                int off, int n, int channels, long n0, float N, hipStream_t s);
// Y (channels x bins complex) items [item0, item0 + nitems) of 16 bytes = the sum over the nparts partitions, ascending, of
// ring A frame (w - (nparts - 1) + p) mod ring times ring B frame p: w is the frame that holds the new block, ring >= nparts
// the frames ring A holds per channel (it may keep more history than the sum walks).  One or two jobs (the head's block,
// the tail's slice) side by side in one launch; up to four in a fade (each under both response sets)
struct NupcMacJob {
  const cpx *ringA = nullptr, *ringB = nullptr;   // channels x ring x bins, channels x nparts x bins
  cpx *Y = nullptr;
  int w = 0, bins = 0, nparts = 0, ring = 0, item0 = 0, nitems = 0;
};
constexpr int kNupcMacDepth = 16;   // partitions whose loads are in flight per lane
constexpr int kNupcMacJobs = 4;
hipError_t launch_nupc_mac(const NupcMacJob *jobs, int njobs, int channels, hipStream_t s);
// Non-uniformly partitioned convolution matrix (pconv_nupm.hip): ONE block of a level, items [item0, item0 + nitems) of
// every output.  ring A: inputs x nparts x bins, frame w holds the new block; H: outputs x inputs x nparts x bins, partition
// q of row (o, i) at ((o * inputs + i) * nparts + q) * bins — the layouts of PconvMatrixArgs, so that launch_pconv_matrix
// runs a head of many blocks over the same state (`ring` frames per input, ring >= nparts: the tail keeps more history
// than the sum walks, input i's frames at i * ring * bins).  Step p of input i pairs ring frame (w - (nparts - 1) + p) mod
// ring with partition nparts - 1 - p; the sequence r = i * nparts + p is cut into `segs` segments at floor(s * inputs * nparts /
// segs), one accumulator per segment and bin over its r ascending: segment 0 writes Y (outputs x bins), segment s > 0 the
// partial P[s - 1] ((segs - 1) x outputs x bins).  launch_nupm_mac runs one or two jobs (the head's block, the tail's
// slice) side by side in one launch, up to four in a fade (each under both response sets); launch_nupm_reduce then forms Y = ((Y + P[0]) + P[1]) + ... for the jobs with segs > 1
// (no launch when there is none).
struct NupmMacJob {
  const cpx *ringA = nullptr, *H = nullptr;
  cpx *Y = nullptr, *P = nullptr;
  int w = 0, bins = 0, nparts = 0, ring = 0, segs = 1, item0 = 0, nitems = 0;
};
constexpr int kNupmMacDepth = 16;   // terms whose loads are in flight per lane
constexpr int kNupmMacJobs = 4;
hipError_t launch_nupm_mac(const NupmMacJob *jobs, int njobs, int inputs, int outputs, hipStream_t s);
hipError_t launch_nupm_reduce(const NupmMacJob *jobs, int njobs, int outputs, hipStream_t s);
constexpr int kPconvMaxLogBins = 15;  // pts up to 32768 (the reference harness' largest, csound/tests.py:13)
// ends of the composed chain used when bins exceed the LDS FFT sizes
hipError_t launch_pconv_pad(const float *in, long in_stride, cpx *work, int bins, int channels, hipStream_t s);
hipError_t launch_pconv_olap(const float *work, float *tail, float *out, int bins, int channels, hipStream_t s);

}  // namespace clfa
