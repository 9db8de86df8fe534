// pconv_args.hpp — the sub-batch launchers' view of an object (pconv_launch.hpp: PconvBlocks, PconvMatrixArgs), filled
// from a geometry, tables, rings and workspaces: everything but the call's rows, K and ring positions.  For the hosts whose
// objects run those launchers — Clpconv and the convolution matrix over their own state, the two non-uniform objects over
// their heads.
#pragma once
#include "conv_host.hpp"
#include "pconv_launch.hpp"

namespace clfa {

inline PconvBlocks pconv_blocks_args(const PconvGeom &g, int cap, int kt, const DevBuf &half, const DevBuf &w2f, const DevBuf &w2i,
                                     const DevBuf &ringA, const DevBuf &ringB, const DevBuf &tail, const DevBuf &X, const DevBuf &XB,
                                     const DevBuf &Y, const DevBuf &tail_ws) {
  PconvBlocks a;
  a.g = g;
  a.cap = cap;
  a.kt = kt;
  a.half = (const cpx *)half.p;
  a.w2f = (const cpx *)w2f.p;
  a.w2i = (const cpx *)w2i.p;
  a.ringA = (cpx *)ringA.p;
  a.ringB = (cpx *)ringB.p;
  a.tail = (float *)tail.p;
  a.X = (cpx *)X.p;
  a.XB = (cpx *)XB.p;
  a.Y = (cpx *)Y.p;
  a.tail_ws = (float *)tail_ws.p;
  return a;
}

// (the second set of a fade, H2 .. mix, is the convolution matrix's own)
inline PconvMatrixArgs pconv_matrix_args(int logb, int nparts, int inputs, int outputs, PconvMatrixPlan plan, int cap,
                                         const DevBuf &half, const DevBuf &w2f, const DevBuf &w2i, const DevBuf &H,
                                         const DevBuf &ringA, const DevBuf &tail, const DevBuf &X, const DevBuf &Y, const DevBuf &P,
                                         const DevBuf &tail_ws) {
  PconvMatrixArgs a;
  a.logb = logb;
  a.bins = 1 << logb;
  a.nparts = nparts;
  a.inputs = inputs;
  a.outputs = outputs;
  a.plan = plan;
  a.cap = cap;
  a.half = (const cpx *)half.p;
  a.w2f = (const cpx *)w2f.p;
  a.w2i = (const cpx *)w2i.p;
  a.H = (const cpx *)H.p;
  a.ringA = (cpx *)ringA.p;
  a.tail = (float *)tail.p;
  a.X = (cpx *)X.p;
  a.Y = (cpx *)Y.p;
  a.P = (cpx *)P.p;
  a.tail_ws = (float *)tail_ws.p;
  return a;
}

}  // namespace clfa
