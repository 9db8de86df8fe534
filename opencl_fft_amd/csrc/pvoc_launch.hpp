// pvoc_launch.hpp — the launchers of the phase vocoder (the ten pvoc_*.hip files) as the Pvoc host sources see them: analysis and
// synthesis (PvocArgs), the oscillator bank (PvocAdsynArgs), and the operations on (amp, freq) frames, each with its *Args
// struct over PvocFramesArgs: ops, pair, shape, time, delay, desc, trace, demix.  (The analysis of a stored signal,
// tanal_kernels.hip, has tanal_launch.hpp: it shares the FFT engine with the Stft kernels, not these launchers; the filter
// bank, bank_kernels.hip, has bank_launch.hpp, and the pitch, pitch_kernels.hip, pitch_launch.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include "cpx.hpp"
#include "device_info.hpp"

namespace clfa {

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

// ---- what the launches of the frame operations below share (filled by pvoc_host.hpp's pvoc_frames_args) ----
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

}  // namespace clfa
