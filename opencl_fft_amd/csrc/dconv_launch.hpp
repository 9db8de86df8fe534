// dconv_launch.hpp — the launchers of the direct convolution as dconv_host.cpp sees them: the one-block form
// (dconv_block.hip: DconvPlan, launch_dconv_block) and the many-block, many-channel form (dconv_blocks.hip:
// DconvBlocksPlan, DconvBlocksArgs, launch_dconv_blocks).
#pragma once
#include <hip/hip_runtime.h>

#include "device_info.hpp"

namespace clfa {

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
