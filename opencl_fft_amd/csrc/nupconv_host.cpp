// nupconv_host.cpp — C ABI of the two non-uniformly partitioned objects (see include/clfft_amd.h): Nupconv (kernels:
// pconv_nup.hip; its head of many blocks is the blocks route of pconv_blocks.hip) and NupconvMatrix (pconv_nupm.hip; its
// head of many blocks is launch_pconv_matrix).  Both run ONE schedule, written once below as templates over the object:
// plain blocks, a fade's block, the second set's history, the head's workspaces, and the bodies of the ABI calls.  What
// differs — the rows, the multiply-accumulate, how a response push lays out its spectra, the head's sub-batch launcher
// and Nupconv's time-varying second input — each object supplies as overloaded functions (the hooks, per object below).
// Shared plumbing: conv_host.hpp and, below it, host.hpp.
#include "pconv_args.hpp"

using namespace clfa;

// one level: its geometry, tables, segments of the multiply-accumulate (Nupconv: 1), the input-spectra ring (`ring`
// frames per row: the head's nparts, which the sub-batch launchers run over; the tail keeps two more than its sum walks,
// the history from which a fade push recomputes the second path), ring position
struct NupLevel {
  int logb = 0, bins = 0, nparts = 0, ring = 0, segs = 1;
  DevBuf half, w2f, w2i;
  DevBuf ringA;
  int w = 0;
};

// what depends on the responses, per level [0] / [1]: the response spectra, the overlap-add tails (a single block's
// inverse reads one and writes the other; cur: the one in force), a single block's accumulators and the segments'
// partial sums (none for Nupconv); and the finished tail block's samples, being mixed in.  A fade runs two of these over
// the shared rings
struct NupSet {
  DevBuf resp[2];
  DevBuf tails[2][2];
  int cur[2] = {0, 0};
  DevBuf pend;
  DevBuf Y[2], P[2];
  size_t state_bytes() const {
    return resp[0].bytes + resp[1].bytes + tails[0][0].bytes + tails[0][1].bytes + tails[1][0].bytes + tails[1][1].bytes + pend.bytes;
  }
  size_t workspace_bytes() const { return Y[0].bytes + Y[1].bytes + P[0].bytes + P[1].bytes; }
  hipError_t clear_history(hipStream_t s) {   // (the responses stay)
    for (DevBuf *b : {&tails[0][0], &tails[0][1], &tails[1][0], &tails[1][1], &pend})
      if (hipError_t e = hipMemsetAsync(b->p, 0, b->bytes, s)) return e;
    cur[0] = cur[1] = 0;
    return hipSuccess;
  }
};

// what both objects are: block_shape(p) gives the rows in and out
struct NupObject {
  DeviceInfo di;
  int cvs = 0, pts0 = 0, pts1 = 0, m = 0;
  int err = 0;
  char log[256];
  hipStream_t stream = nullptr;
  NupLevel lv[2];                // the head (2m partitions of pts0) and the tail (n1 partitions of pts1)
  NupSet sets[2];                // sets[cur]: the responses in force and their path.  sets[cur ^ 1]: the second path of a
  int cur = 0;                   // timed crossfade (push_ir_fade), allocated by the first fade push and kept; it becomes
                                 // the first, on the host, when the fade's last block is issued
  NupSet &first() { return sets[cur]; }
  NupSet &second() { return sets[cur ^ 1]; }
  DevBuf stage;                  // the tail block being collected (rows in x pts1)
  DevBuf headb;                  // a fade: the second path's head samples (rows out x pts0)
  long fade_len = 0, fade_done = 0;   // head blocks of the pending fade (0: none) and how many of them have been processed
  DevBuf bX, bY, bP, btail;      // the head's sub-batch workspaces, for hcap blocks (grown by the call that needs more)
  int hcap = 0, bcap = 1, bkt = 4;
  DevBuf in1, in2, out;          // staging of the blocking forms (conv_arrays; in2: Nupconv's time-varying second input)
  DevBuf ir;                     // ... and of push_ir
  StreamOrder order;
  long c = 0;                    // head blocks since creation / reset
};

// a multiply-accumulate of the schedule: items [item0, item0 + nitems) of the level's block in ring frame w under the
// set's responses, into the set's accumulators.  One or two side by side in one launch (the head's block, the tail's
// slice), up to four in a fade (each under both sets)
struct NupJob {
  int level;
  const NupSet *set;
  int w, item0, nitems;
};
static_assert(kNupcMacJobs == 4 && kNupmMacJobs == 4, "a fade's four jobs");

// ---------------------------------------------------------------------------------
// the hooks of Nupconv: channels rows in and out, one response per channel
// ---------------------------------------------------------------------------------

struct clfa_nupconv : NupObject {
  int channels = 0;
  DevBuf stage2;                 // the second input's tail block being collected (allocated by the first time-varying call)
  int tv_count = 0;              // time-varying blocks among the head blocks of the tail block being collected
  DevBuf bXB;                    // the second input's sub-batch spectra, for hcap2 blocks (time-varying calls of several blocks)
  int hcap2 = 0;
};

static BlockShape block_shape(const clfa_nupconv *p) { return {p->pts0, p->channels, p->channels}; }
static long nup_resp_rows(const clfa_nupconv *p) { return p->channels; }

static PconvGeom nup_head_geom(const clfa_nupconv *p) { return {p->lv[0].logb, p->lv[0].bins, p->lv[0].nparts, p->channels}; }
static void nup_plan(clfa_nupconv *p) {
  p->bcap = subbatch_cap(3L * p->channels * p->pts0 * (long)sizeof(cpx), "CLFA_PCONV_BLOCKS_MAX");   // as Clpconv's blocks route
  p->bkt = pconv_blocks_tile(nup_head_geom(p), p->di);
}

// h[0 : 2*pts1) in the head's partitions, h[2*pts1 : 2*pts1 + n1*pts1) in the tail's, in stream order: partition i of
// every row -> response frame nparts - 1 - i of the level (the frame the MAC pairs with the i-th newest input block), with
// the blocks route's forward transform: the bits Clpconv's push gives
static int nup_push_levels(const clfa_nupconv *p, const NupSet &set, const float *ir, long stride, hipStream_t s) {
  for (int k = 0; k < 2; k++) {
    const NupLevel &l = p->lv[k];
    const float *src = ir + (k ? 2L * p->pts1 : 0);
    const int aligned = rows_aligned8(src, stride);
    for (int i = 0; i < l.nparts; i++)
      HIP_TRY(launch_pconvb_forward(l.logb, src + (long)i * l.bins, stride, (cpx *)set.resp[k].p + (long)(l.nparts - 1 - i) * l.bins, 1,
                                    l.nparts, p->channels, aligned, (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  }
  return CLFA_SUCCESS;
}

static int nup_mac(const clfa_nupconv *p, const NupJob *jobs, int njobs, hipStream_t s) {
  NupcMacJob j[kNupcMacJobs];
  for (int i = 0; i < njobs; i++) {
    const NupLevel &l = p->lv[jobs[i].level];
    const NupSet &b = *jobs[i].set;
    j[i] = {(const cpx *)l.ringA.p, (const cpx *)b.resp[jobs[i].level].p, (cpx *)b.Y[jobs[i].level].p, jobs[i].w, l.bins, l.nparts, l.ring,
            jobs[i].item0, jobs[i].nitems};
  }
  HIP_TRY(launch_nupc_mac(j, njobs, p->channels, s));
  return CLFA_SUCCESS;
}

// the head's K blocks through the blocks route, sub-batch by sub-batch, as clfa_pconv_process_blocks_dev.  in2, before
// a = n0 in the response period: the blocks are time-varying ones at positions pos, pos + 1, ... < n0, the time-varying
// blocks route: block j's second input becomes response frame n0 - 1 - (pos + j) for itself and the blocks after it
static int nup_head(clfa_nupconv *p, float *out, long out_stride, const float *in, long in_stride, long nblocks, hipStream_t s,
                    const float *in2, long in2_stride) {
  NupLevel &l = p->lv[0];
  NupSet &set = p->first();
  const long pos = p->c % ((long)(p->lv[1].nparts + 2) * p->m);
  if (pos >= l.nparts) in2 = nullptr;
  PconvBlocks a = pconv_blocks_args(nup_head_geom(p), p->hcap, p->bkt, l.half, l.w2f, l.w2i, l.ringA, set.resp[0],
                                    set.tails[0][set.cur[0]], p->bX, p->bXB, p->bY, p->btail);
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = rows_aligned8(in, in_stride);
  a.aligned_out = rows_aligned8(out, out_stride);
  a.in2_stride = in2_stride;
  a.aligned_in2 = rows_aligned8(in2, in2_stride);
  for (long j0 = 0; j0 < nblocks; j0 += a.K) {
    a.K = (int)(nblocks - j0 < p->hcap ? nblocks - j0 : p->hcap);
    a.w = l.w;
    a.in1 = in + j0 * p->pts0;
    a.in2 = in2 ? in2 + j0 * p->pts0 : nullptr;
    a.w2 = (int)(l.nparts - 1 - (pos + j0));
    a.out = out + j0 * p->pts0;
    HIP_TRY(launch_pconv_blocks(a, s));
    l.w = (int)((l.w + a.K) % l.nparts);
  }
  return CLFA_SUCCESS;
}

// The time-varying second input (clfft_amd.h), step 1, asked at phase 0 of period P >= 1: the response frame of the tail
// level that the second input's finished tail block U = P - 1 rewrites, or -1 where it rewrites none — one of its m head
// blocks was a plain block, or it lies in the two head-covered tail blocks of its response period
static int nup_tv_frame(const clfa_nupconv *p) {
  const int n1 = p->lv[1].nparts;
  const long r = (p->c / p->m - 1) % (n1 + 2);
  return p->tv_count == p->m && r >= 2 ? n1 - 1 - (int)(r - 2) : -1;
}
// phase 0 of period P, after the tail level's forward transform: step 1 carried out by a plain block (or a fade's, for
// time-varying blocks before the fade push) — the second stage row -> that frame of the set in force, push_ir's
// transform; and the count of the block now beginning
static int nup_phase0(clfa_nupconv *p, long P, hipStream_t s) {
  const NupLevel &t = p->lv[1];
  const int fr = P >= 1 ? nup_tv_frame(p) : -1;
  if (fr >= 0)
    HIP_TRY(launch_pconvb_forward(t.logb, (const float *)p->stage2.p, p->pts1, (cpx *)p->first().resp[1].p + (long)fr * t.bins, 1,
                                  t.nparts, p->channels, 1, (const cpx *)t.half.p, (const cpx *)t.w2f.p, s));
  p->tv_count = 0;
  return CLFA_SUCCESS;
}
// n samples of every row into the stage rows at off; with a second input (time-varying blocks) both in one launch
static int nup_stage(clfa_nupconv *p, const float *x, long in_stride, const float *x2, long in2_stride, int off, int n, hipStream_t s) {
  if (!x2) {
    HIP_TRY(launch_nupc_stage(x, in_stride, (float *)p->stage.p, p->pts1, off, n, p->channels, s));
    return CLFA_SUCCESS;
  }
  HIP_TRY(launch_nupc_stage2(x, in_stride, (float *)p->stage.p, x2, in2_stride, (float *)p->stage2.p, p->pts1, off, n, p->channels, s));
  p->tv_count += n / p->pts0;
  return CLFA_SUCCESS;
}
// reset: the second input's block in progress and how much of it is there
static int nup_reset_tv(clfa_nupconv *p, hipStream_t s) {
  if (p->stage2.p) HIP_TRY(hipMemsetAsync(p->stage2.p, 0, p->stage2.bytes, s));
  p->tv_count = 0;
  return CLFA_SUCCESS;
}

// ---------------------------------------------------------------------------------
// the hooks of NupconvMatrix: inputs rows in, outputs rows out, outputs x inputs responses in the matrix's layout
// ---------------------------------------------------------------------------------

struct clfa_nupconv_matrix : NupObject {
  int inputs = 0, outputs = 0;
};

static BlockShape block_shape(const clfa_nupconv_matrix *p) { return {p->pts0, p->inputs, p->outputs}; }
static long nup_resp_rows(const clfa_nupconv_matrix *p) { return (long)p->outputs * p->inputs; }

// each level's segments: the matrix's plan and its tuning switch, as mconv_setup — for the head at its geometry, for the
// tail at the geometry of a SLICE (pts0 bins of n1 partitions): a single-block call offers the multiply-accumulate
// pts0 / 2 items per output, not pts1 / 2, and with the whole block's count 64 x 64 at 64 / 4096 ran one segment of 3968
// terms on 32 waves (896 us per block against 160 for Nupconv on expanded inputs; profiles/HISTORY.md)
static void nup_plan(clfa_nupconv_matrix *p) {
  for (NupLevel &l : p->lv) {
    const PconvMatrixPlan pl = pconv_matrix_plan(p->pts0, l.nparts, p->inputs, p->outputs, p->di);
    l.segs = pl.segs;
    if (&l == &p->lv[0]) p->bkt = pl.kt;
    if (const char *env = getenv("CLFA_PCONV_MATRIX_SEGS")) {
      if (atoi(env) >= 1 && atoi(env) <= 4096) l.segs = atoi(env);
    }
  }
  p->bcap = subbatch_cap(((long)p->inputs + (long)p->outputs * p->lv[0].segs) * p->pts0 * (long)sizeof(cpx),
                         "CLFA_PCONV_MATRIX_BLOCKS_MAX");
}

// every partition of every row into a set's response spectra, one forward launch per level, as
// clfa_pconv_matrix_push_ir_dev: row (o, i) partition q -> frame ((o * inputs + i) * nparts + q); h[0 : 2*pts1) in the
// head's partitions, what follows in the tail's
static int nup_push_levels(const clfa_nupconv_matrix *p, const NupSet &set, const float *rows, long row_stride, hipStream_t s) {
  for (int k = 0; k < 2; k++) {
    const NupLevel &l = p->lv[k];
    const float *src = rows + (k ? 2L * p->pts1 : 0);
    HIP_TRY(launch_pconvb_forward(l.logb, src, row_stride, (cpx *)set.resp[k].p, l.nparts, l.nparts, p->outputs * p->inputs,
                                  rows_aligned8(src, row_stride), (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  }
  return CLFA_SUCCESS;
}

// ... the multiply-accumulates and then the segments' sums
static int nup_mac(const clfa_nupconv_matrix *p, const NupJob *jobs, int njobs, hipStream_t s) {
  NupmMacJob j[kNupmMacJobs];
  for (int i = 0; i < njobs; i++) {
    const NupLevel &l = p->lv[jobs[i].level];
    const NupSet &b = *jobs[i].set;
    j[i] = {(const cpx *)l.ringA.p, (const cpx *)b.resp[jobs[i].level].p, (cpx *)b.Y[jobs[i].level].p, (cpx *)b.P[jobs[i].level].p,
            jobs[i].w, l.bins, l.nparts, l.ring, l.segs, jobs[i].item0, jobs[i].nitems};
  }
  HIP_TRY(launch_nupm_mac(j, njobs, p->inputs, p->outputs, s));
  HIP_TRY(launch_nupm_reduce(j, njobs, p->outputs, s));
  return CLFA_SUCCESS;
}

// the head's K blocks through the matrix's sub-batch launches, sub-batch by sub-batch, as clfa_pconv_matrix_process_dev
static int nup_head(clfa_nupconv_matrix *p, float *out, long out_stride, const float *in, long in_stride, long nblocks, hipStream_t s,
                    const float *, long) {
  NupLevel &l = p->lv[0];
  NupSet &set = p->first();
  PconvMatrixArgs a = pconv_matrix_args(l.logb, l.nparts, p->inputs, p->outputs, {p->bkt, l.segs}, p->hcap, l.half, l.w2f, l.w2i,
                                        set.resp[0], l.ringA, set.tails[0][set.cur[0]], p->bX, p->bY, p->bP, p->btail);
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.aligned_in = rows_aligned8(in, in_stride);
  a.aligned_out = rows_aligned8(out, out_stride);
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

// (no second input: phase 0 is the tail level's forward transform alone, staging the plain launch, reset the shared part)
static int nup_phase0(clfa_nupconv_matrix *, long, hipStream_t) { return CLFA_SUCCESS; }
static int nup_stage(clfa_nupconv_matrix *p, const float *x, long in_stride, const float *, long, int off, int n, hipStream_t s) {
  HIP_TRY(launch_nupc_stage(x, in_stride, (float *)p->stage.p, p->pts1, off, n, p->inputs, s));
  return CLFA_SUCCESS;
}
static int nup_reset_tv(clfa_nupconv_matrix *, hipStream_t) { return CLFA_SUCCESS; }

// ---------------------------------------------------------------------------------
// creation
// ---------------------------------------------------------------------------------

// the two partition sizes and the response length, and the levels they give
static int nup_geometry(NupObject *p, int cvs, int pts0, int pts1) {
  p->log[0] = 0;
  p->cvs = cvs;
  p->pts0 = pts0;
  p->pts1 = pts1;
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
  p->m = pts1 / pts0;
  NupLevel &h = p->lv[0], &t = p->lv[1];
  h.logb = ilog2(pts0), h.bins = pts0, h.nparts = 2 * p->m;
  t.logb = ilog2(pts1), t.bins = pts1, t.nparts = (cvs - 2 * pts1) / pts1;   // floor: remainder samples are dropped
  h.ring = h.nparts;
  t.ring = t.nparts + 2;
  return CLFA_SUCCESS;
}

// a set's buffers (kept once they exist)
template <class T>
static int nup_alloc_set(const T *p, NupSet &b) {
  const size_t outs = (size_t)block_shape(p).out_rows;
  int e;
  for (int k = 0; k < 2; k++) {
    const NupLevel &l = p->lv[k];
    const size_t frame = sizeof(cpx) * (size_t)l.bins, tail = sizeof(float) * outs * l.bins;
    if ((e = b.resp[k].ensure(frame * (size_t)nup_resp_rows(p) * l.nparts)) || (e = b.Y[k].ensure(frame * outs)) ||
        (l.segs > 1 && (e = b.P[k].ensure(frame * outs * (size_t)(l.segs - 1)))) || (e = b.tails[k][0].ensure(tail)) ||
        (e = b.tails[k][1].ensure(tail)))
      return e;
  }
  return b.pend.ensure(sizeof(float) * outs * p->pts1);
}

// after the geometry and the object's rows: the device, the object's plan, tables, rings and the first set, all zero
template <class T>
static int nup_setup(T *p, int device) {
  int e = device_info(device, p->di);
  if (e) return e;
  nup_plan(p);
  ENTER_DEVICE(device);
  HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  const size_t ins = (size_t)block_shape(p).in_rows;
  for (NupLevel &l : p->lv) {
    if ((e = upload_conv_tables(l.bins, l.half, l.w2f, l.w2i))) return e;
    if ((e = l.ringA.ensure(sizeof(cpx) * (size_t)l.bins * ins * l.ring))) return e;
    HIP_TRY(hipMemsetAsync(l.ringA.p, 0, l.ringA.bytes, p->stream));
  }
  NupSet &a = p->first();
  if ((e = nup_alloc_set(p, a)) || (e = p->stage.ensure(sizeof(float) * ins * p->pts1))) return e;
  for (DevBuf *b : {&a.resp[0], &a.resp[1], &p->stage}) HIP_TRY(hipMemsetAsync(b->p, 0, b->bytes, p->stream));
  HIP_TRY(a.clear_history(p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return CLFA_SUCCESS;
}

static int nupc_setup(clfa_nupconv *p, int device, int cvs, int pts0, int pts1, int channels) {
  p->channels = channels;
  if (int e = nup_geometry(p, cvs, pts0, pts1)) return e;
  if (channels < 1) {
    snprintf(p->log, sizeof(p->log), "channels must be at least 1 (got %d)", channels);
    return CLFA_INVALID_VALUE;
  }
  return nup_setup(p, device);
}

static int nupm_setup(clfa_nupconv_matrix *p, int device, int cvs, int pts0, int pts1, int inputs, int outputs) {
  p->inputs = inputs;
  p->outputs = outputs;
  if (int e = nup_geometry(p, cvs, pts0, pts1)) return e;
  if (inputs < 1) {
    snprintf(p->log, sizeof(p->log), "inputs must be at least 1 (got %d)", inputs);
    return CLFA_INVALID_VALUE;
  }
  if (outputs < 1) {
    snprintf(p->log, sizeof(p->log), "outputs must be at least 1 (got %d)", outputs);
    return CLFA_INVALID_VALUE;
  }
  return nup_setup(p, device);
}

// ---------------------------------------------------------------------------------
// the schedule
// ---------------------------------------------------------------------------------

// one block of a level, single-block route.  forward: the rows' samples -> ring frame w (committing it is the caller's
// w + 1)
template <class T>
static int nup_forward(const T *p, const NupLevel &l, const float *in, long in_stride, hipStream_t s) {
  HIP_TRY(launch_pconvb_forward(l.logb, in, in_stride, (cpx *)l.ringA.p + (long)l.w * l.bins, 1, l.ring, (int)block_shape(p).in_rows,
                                rows_aligned8(in, in_stride), (const cpx *)l.half.p, (const cpx *)l.w2f.p, s));
  return CLFA_SUCCESS;
}
// ... inverse transform and overlap-add of level k: the set's Y and the tail in force -> out, the other tail, which comes
// into force
template <class T>
static int nup_inverse(const T *p, int k, NupSet &set, float *out, long out_stride, hipStream_t s) {
  const NupLevel &l = p->lv[k];
  int &cur = set.cur[k];
  HIP_TRY(launch_pconvb_inverse(l.logb, (const cpx *)set.Y[k].p, (const float *)set.tails[k][cur].p, (float *)set.tails[k][cur ^ 1].p, out,
                                out_stride, 1, 1, 1, (int)block_shape(p).out_rows, rows_aligned8(out, out_stride), (const cpx *)l.half.p,
                                (const cpx *)l.w2i.p, s));
  cur ^= 1;
  return CLFA_SUCCESS;
}

// nblocks >= 1 blocks outside a fade.  One block: the head's forward transform straight into its ring frame, its
// multiply-accumulate beside the tail's slice in one launch (nup_mac), its inverse.  Several blocks: the head through its
// sub-batch launcher over the whole call (nup_head), the tail's slices between two period boundaries in one launch.  The
// arithmetic of a bin is the same on both ways, and both leave the same rings, tails and positions.  x2 (Nupconv; or
// NULL): the blocks are time-varying ones, a stretch that lies on one side of a = n0 in its response period — their
// second input is staged beside x, and before a = n0 the head takes the time-varying blocks route.
template <class T>
static int nup_blocks(T *p, float *o, long out_stride, const float *x, long in_stride, long nblocks, hipStream_t s,
                      const float *x2 = nullptr, long in2_stride = 0) {
  const long pts0 = p->pts0, m = p->m;
  const int outs = (int)block_shape(p).out_rows;
  const bool single = nblocks == 1;
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &a = p->first();
  if (!single)
    if (int e = nup_head(p, o, out_stride, x, in_stride, nblocks, s, x2, in2_stride)) return e;
  // the tail, period by period: head blocks [j0, j0 + k) of the call are phases [sa, sb) of period P, in which tail block
  // P - 1 is multiplied and tail block P - 2 is heard
  const int hb0 = (int)(pts0 / 2);
  for (long j0 = 0; j0 < nblocks;) {
    const long P = p->c / m;
    const int sa = (int)(p->c % m);
    const long k = nblocks - j0 < m - sa ? nblocks - j0 : m - sa;
    const int sb = sa + (int)k, off = sa * (int)pts0, n = (int)(k * pts0);
    if (single)
      if (int e = nup_forward(p, h, x, in_stride, s)) return e;
    // phase 0: the spectra of the finished block, before this period's samples overwrite the rows
    if (sa == 0) {
      if (P >= 1)
        if (int e = nup_forward(p, t, (const float *)p->stage.p, p->pts1, s)) return e;
      if (int e = nup_phase0(p, P, s)) return e;
    }
    if (int e = nup_stage(p, x + j0 * pts0, in_stride, x2 ? x2 + j0 * pts0 : nullptr, in2_stride, off, n, s)) return e;
    NupJob jobs[2];
    int njobs = 0;
    if (single) jobs[njobs++] = {0, &a, h.w, 0, hb0};
    if (P >= 1) jobs[njobs++] = {1, &a, t.w, sa * hb0, (sb - sa) * hb0};
    if (njobs)
      if (int e = nup_mac(p, jobs, njobs, s)) return e;
    if (single) {
      if (int e = nup_inverse(p, 0, a, o, out_stride, s)) return e;
      h.w = (h.w + 1) % h.ring;
    }
    HIP_TRY(launch_nupc_mix(o + j0 * pts0, out_stride, (const float *)a.pend.p, p->pts1, off, n, outs, s));
    // after slice m - 1: the block's samples replace the ones just heard, its spectra stay in the ring
    if (P >= 1 && sb == m) {
      if (int e = nup_inverse(p, 1, a, (float *)a.pend.p, p->pts1, s)) return e;
      t.w = (t.w + 1) % t.ring;
    }
    p->c += k;
    j0 += k;
  }
  return CLFA_SUCCESS;
}

// One head block of a fade, on the single-block route with every response-dependent step run for both sets over the
// shared rings: the four multiply-accumulates are one nup_mac, the first path's head goes to the output rows and the
// second's to headb, and k_nupc_fade_mix forms both paths' head + pending sums and a + g * (b - a) over the output rows.
// After the fade's last block the second set becomes the first (nothing is copied; the objects are not capturable, so no
// address has to stay fixed).
template <class T>
static int nup_fade_block(T *p, float *o, long out_stride, const float *x, long in_stride, hipStream_t s) {
  NupLevel &h = p->lv[0], &t = p->lv[1];
  NupSet &a = p->first(), &b = p->second();
  const int pts0 = p->pts0, m = p->m, hb0 = pts0 / 2, outs = (int)block_shape(p).out_rows;
  const long P = p->c / m;
  const int sa = (int)(p->c % m), off = sa * pts0;
  if (int e = nup_forward(p, h, x, in_stride, s)) return e;
  if (sa == 0) {
    if (P >= 1)
      if (int e = nup_forward(p, t, (const float *)p->stage.p, p->pts1, s)) return e;
    if (int e = nup_phase0(p, P, s)) return e;
  }
  if (int e = nup_stage(p, x, in_stride, nullptr, 0, off, pts0, s)) return e;
  NupJob jobs[4];
  int njobs = 0;
  jobs[njobs++] = {0, &a, h.w, 0, hb0};
  jobs[njobs++] = {0, &b, h.w, 0, hb0};
  if (P >= 1) {
    jobs[njobs++] = {1, &a, t.w, sa * hb0, hb0};
    jobs[njobs++] = {1, &b, t.w, sa * hb0, hb0};
  }
  int e;
  if ((e = nup_mac(p, jobs, njobs, s)) || (e = nup_inverse(p, 0, a, o, out_stride, s)) ||
      (e = nup_inverse(p, 0, b, (float *)p->headb.p, pts0, s)))
    return e;
  h.w = (h.w + 1) % h.ring;
  HIP_TRY(launch_nupc_fade_mix(o, out_stride, (const float *)p->headb.p, (const float *)a.pend.p, (const float *)b.pend.p, p->pts1,
                               off, pts0, outs, p->fade_done * pts0, (float)(p->fade_len * pts0), s));
  if (P >= 1 && sa == m - 1) {
    if ((e = nup_inverse(p, 1, a, (float *)a.pend.p, p->pts1, s)) || (e = nup_inverse(p, 1, b, (float *)b.pend.p, p->pts1, s)))
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
// again from tail blocks P - 3 and P - 2 (whole blocks in one multiply-accumulate: the matrix's segments cut the term
// sequence, not the bins, so a bin's sums do not depend on how the bins are cut into slices); slices [0, sa) of tail block
// P - 1, in progress.  A block of negative index is not computed: what it would have left is the +0 the rows are cleared
// to.  Tail block P - 3 reads back to input block P - 2 - n1, which is why the tail's ring keeps n1 + 2 frames; head block
// c - 1 reads frames w - 2m .. w - 1, all intact in a ring of 2m.
template <class T>
static int nup_prime(T *p, hipStream_t s) {
  NupSet &b = p->second();
  const long P = p->c / p->m;
  const int sa = (int)(p->c % p->m);
  HIP_TRY(b.clear_history(s));
  // items [0, nitems) of level k's block `back` blocks before frame w: multiply-accumulate
  const auto mac = [&](int k, int back, int nitems) {
    const NupLevel &l = p->lv[k];
    const NupJob job = {k, &b, (l.w - back + l.ring) % l.ring, 0, nitems};
    return nup_mac(p, &job, 1, s);
  };
  // a whole block: then its inverse (the samples: to `out`, rows of the level's block length)
  const auto block = [&](int k, int back, float *out) {
    if (int e = mac(k, back, p->lv[k].bins / 2)) return e;
    return nup_inverse(p, k, b, out, p->lv[k].bins, s);
  };
  int e;
  if (p->c >= 1 && (e = block(0, 1, (float *)p->headb.p))) return e;
  if (P >= 3 && (e = block(1, 2, (float *)b.pend.p))) return e;
  if (P >= 2 && (e = block(1, 1, (float *)b.pend.p))) return e;
  if (P >= 1 && sa > 0 && (e = mac(1, 0, sa * (p->pts0 / 2)))) return e;
  return CLFA_SUCCESS;
}

// the head's sub-batch workspaces for a call of `rest` blocks through its launcher
template <class T>
static int nup_ensure_head(T *p, long rest, hipStream_t s) {
  if (rest <= 1 || rest <= p->hcap) return CLFA_SUCCESS;
  const int cap = (int)(rest < p->bcap ? rest : p->bcap);
  if (cap <= p->hcap) return CLFA_SUCCESS;
  const BlockShape sh = block_shape(p);
  const size_t frames = sizeof(cpx) * (size_t)cap * (size_t)p->pts0;
  if (int e = ensure_workspaces({{&p->bX, frames * sh.in_rows},
                                 {&p->bY, frames * sh.out_rows},
                                 {&p->bP, frames * sh.out_rows * (size_t)(p->lv[0].segs - 1)},
                                 {&p->btail, sizeof(float) * (size_t)sh.out_rows * (size_t)p->pts0}},
                                s))
    return e;
  p->hcap = cap;
  return CLFA_SUCCESS;
}

// ---------------------------------------------------------------------------------
// the bodies of the ABI calls
// ---------------------------------------------------------------------------------

template <class T>
static long nup_ir_len(const T *p) {
  return 2L * p->pts1 + (long)p->lv[1].nparts * p->pts1;
}
template <class T>
static size_t nup_state_bytes(const T *p) {
  return p->lv[0].ringA.bytes + p->lv[1].ringA.bytes + p->stage.bytes + p->sets[0].state_bytes() + p->sets[1].state_bytes();
}
template <class T>
static size_t nup_workspace_bytes(const T *p) {
  return p->sets[0].workspace_bytes() + p->sets[1].workspace_bytes() + p->headb.bytes + p->bX.bytes + p->bY.bytes + p->bP.bytes +
         p->btail.bytes;
}

template <class T>
static int nup_push_ir_dev(T *p, const void *ir, long stride, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || stride < nup_ir_len(p)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // a fade is pending: the responses are one end of it
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(p->order.use(s));
  return nup_push_levels(p, p->first(), (const float *)ir, stride, s);
}

template <class T>
static int nup_push_ir_fade_dev(T *p, const void *ir, long stride, long fade_blocks, void *stream) {
  if (int e = obj_error(p)) return e;
  if (!device_rows_ok(ir) || stride < nup_ir_len(p) || !fade_blocks_ok(fade_blocks, p->pts0)) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;   // one fade at a time
  ENTER_DEVICE(p->di.device);
  hipStream_t s = (hipStream_t)stream;
  // everything the fade needs is allocated here, so that no process call allocates because of it: refused under capture
  if (StreamOrder::capturing(s)) return CLFA_INVALID_OPERATION;
  NupSet &b = p->second();
  int e;
  if ((e = nup_alloc_set(p, b)) || (e = p->headb.ensure(sizeof(float) * (size_t)block_shape(p).out_rows * p->pts0))) return e;
  HIP_TRY(p->order.use(s));
  // the rows' spectra into the second set (as push_ir_dev into the first), then that set's history from the rings
  if ((e = nup_push_levels(p, b, (const float *)ir, stride, s)) || (e = nup_prime(p, s))) return e;
  p->fade_len = fade_blocks;
  p->fade_done = 0;
  return CLFA_SUCCESS;
}

// the blocking pushes; fade_blocks: of push_ir_fade, NULL for push_ir
template <class T>
static int nup_push_ir_host(T *p, const float *ir, const long *fade_blocks) {
  if (int e = obj_error(p)) return e;
  if (!ir || (fade_blocks && !fade_blocks_ok(*fade_blocks, p->pts0))) return CLFA_INVALID_VALUE;
  if (p->fade_len) return CLFA_INVALID_OPERATION;
  ENTER_DEVICE(p->di.device);
  const long len = nup_ir_len(p);
  return push_host(p, ir, sizeof(float) * (size_t)nup_resp_rows(p) * len, [&](const void *rows) {
    return fade_blocks ? nup_push_ir_fade_dev(p, rows, len, *fade_blocks, p->stream) : nup_push_ir_dev(p, rows, len, p->stream);
  });
}

template <class T>
static int nup_process_dev(T *p, void *out, long out_stride, const void *in, long in_stride, long nblocks, void *stream) {
  if (int e = obj_error(p)) return e;
  const BlockShape sh = block_shape(p);
  const long pts0 = sh.pts;
  long len;
  if (int e = check_blocks_dev(nblocks, pts0, out, out_stride, sh.out_rows, in, nullptr, in_stride, sh.in_rows, &len)) return e;
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

template <class T>
static int nup_convolution(T *p, float *out, const float *in, long nblocks) {
  return blocks_host(p, out, in, nullptr, nblocks, [&](void *o, long len, const void *i1, const void *) {
    return nup_process_dev(p, o, len, i1, len, nblocks, p->stream);
  });
}

template <class T>
static int nup_reset(T *p, void *stream) {
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
  if (int e = nup_reset_tv(p, s)) return e;
  HIP_TRY(p->first().clear_history(s));
  p->c = 0;
  return CLFA_SUCCESS;
}

// ---------------------------------------------------------------------------------
// Nupconv's own: the time-varying second input
// ---------------------------------------------------------------------------------

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
  const int ch = p->channels, pts0 = p->pts0, m = p->m, hb0 = pts0 / 2, n0 = h.nparts;
  const long P = p->c / m, R0 = (long)(t.nparts + 2) * m, pos = p->c % R0;
  const int sa = (int)(p->c % m), off = sa * pts0;
  if (P >= 1 && sa == 0) {
    NupcFwdJob jobs[2];
    int njobs = 0;
    jobs[njobs++] = {(const float *)p->stage.p, p->pts1, 1, (cpx *)t.ringA.p + (long)t.w * t.bins, t.ring, nullptr, 0};
    const int fr = nup_tv_frame(p);
    if (fr >= 0) jobs[njobs++] = {(const float *)p->stage2.p, p->pts1, 1, (cpx *)a.resp[1].p + (long)fr * t.bins, t.nparts, nullptr, 0};
    HIP_TRY(launch_nupc_fwd(t.logb, jobs, njobs, ch, (const cpx *)t.half.p, (const cpx *)t.w2f.p, s));
  }
  if (sa == 0) p->tv_count = 0;
  const NupcFwdJob jobs0[2] = {
      {x, in_stride, rows_aligned8(x, in_stride), (cpx *)h.ringA.p + (long)h.w * pts0, h.ring, (float *)p->stage.p + off, p->pts1},
      {x2, in2_stride, rows_aligned8(x2, in2_stride), pos < n0 ? (cpx *)a.resp[0].p + (long)(n0 - 1 - pos) * pts0 : nullptr, n0,
       (float *)p->stage2.p + off, p->pts1}};
  HIP_TRY(launch_nupc_fwd(h.logb, jobs0, 2, ch, (const cpx *)h.half.p, (const cpx *)h.w2f.p, s));
  p->tv_count++;
  NupJob jobs[2];
  int njobs = 0;
  jobs[njobs++] = {0, &a, h.w, 0, hb0};
  if (P >= 1) jobs[njobs++] = {1, &a, t.w, sa * hb0, hb0};
  if (int e = nup_mac(p, jobs, njobs, s)) return e;
  if (int e = nup_inverse(p, 0, a, o, out_stride, s)) return e;
  h.w = (h.w + 1) % h.ring;
  HIP_TRY(launch_nupc_mix(o, out_stride, (const float *)a.pend.p, p->pts1, off, pts0, ch, s));
  if (P >= 1 && sa == m - 1) {
    if (int e = nup_inverse(p, 1, a, (float *)a.pend.p, p->pts1, s)) return e;
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
  const long pts0 = p->pts0, n0 = p->lv[0].nparts, R0 = (long)(p->lv[1].nparts + 2) * p->m;
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

extern "C" {

int clfa_nupconv_create(clfa_nupconv **pc, int device, int cvs, int pts0, int pts1, int channels) {
  return create_object(pc, [&](clfa_nupconv *p) { return nupc_setup(p, device, cvs, pts0, pts1, channels); });
}

void clfa_nupconv_destroy(clfa_nupconv *p) { destroy_object(p); }

int clfa_nupconv_get_error(const clfa_nupconv *p) { return p ? p->err : CLFA_INVALID_VALUE; }
const char *clfa_nupconv_get_log(const clfa_nupconv *p) { return p ? p->log : ""; }
int clfa_nupconv_nparts(const clfa_nupconv *p, int level) {
  return p && !p->err && (level == 0 || level == 1) ? p->lv[level].nparts : 0;
}
long clfa_nupconv_position(const clfa_nupconv *p) { return p ? p->c : 0; }
size_t clfa_nupconv_state_bytes(const clfa_nupconv *p) { return p ? nup_state_bytes(p) + p->stage2.bytes : 0; }
size_t clfa_nupconv_workspace_bytes(const clfa_nupconv *p) { return p ? nup_workspace_bytes(p) + p->bXB.bytes : 0; }
long clfa_nupconv_fade_remaining(const clfa_nupconv *p) { return p ? p->fade_len - p->fade_done : 0; }
const char *clfa_nupconv_kernel_name(const clfa_nupconv *p) { return !p || p->err ? "" : "k_nupc_mac"; }

int clfa_nupconv_push_ir_dev(clfa_nupconv *p, const void *ir, long channel_stride, void *stream) {
  return nup_push_ir_dev(p, ir, channel_stride, stream);
}
int clfa_nupconv_push_ir(clfa_nupconv *p, const float *ir) { return nup_push_ir_host(p, ir, nullptr); }
int clfa_nupconv_push_ir_fade_dev(clfa_nupconv *p, const void *ir, long channel_stride, long fade_blocks, void *stream) {
  return nup_push_ir_fade_dev(p, ir, channel_stride, fade_blocks, stream);
}
int clfa_nupconv_push_ir_fade(clfa_nupconv *p, const float *ir, long fade_blocks) { return nup_push_ir_host(p, ir, &fade_blocks); }
int clfa_nupconv_process_dev(clfa_nupconv *p, void *out, long out_stride, const void *in, long in_stride, long nblocks,
                             void *stream) {
  return nup_process_dev(p, out, out_stride, in, in_stride, nblocks, stream);
}
int clfa_nupconv_convolution(clfa_nupconv *p, float *out, const float *in, long nblocks) { return nup_convolution(p, out, in, nblocks); }
int clfa_nupconv_reset(clfa_nupconv *p, void *stream) { return nup_reset(p, stream); }

long clfa_nupconv_tv_period(const clfa_nupconv *p) { return p && !p->err ? (long)(p->lv[1].nparts + 2) * p->m : 0; }

int clfa_nupconv_process_tv_dev(clfa_nupconv *p, void *out, long out_stride, const void *in, long in_stride, const void *in2,
                                long in2_stride, long nblocks, void *stream) {
  if (!in2) return nup_process_dev(p, out, out_stride, in, in_stride, nblocks, stream);
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
  const long n0 = p->lv[0].nparts, stat = clfa_nupconv_tv_period(p) - n0, longest = stat > n0 ? stat : n0;
  if (int e = nup_ensure_head(p, nblocks < longest ? nblocks : longest, s)) return e;
  // ... and the second input's spectra (the frames of a channel lie hcap frames apart in every workspace of the sub-batch)
  if (p->hcap2 < p->hcap) {
    if (int e = ensure_workspaces({{&p->bXB, sizeof(cpx) * (size_t)ch * (size_t)p->hcap * (size_t)pts0}}, s)) return e;
    p->hcap2 = p->hcap;
  }
  HIP_TRY(p->order.use(s));
  if (first) HIP_TRY(hipMemsetAsync(p->stage2.p, 0, p->stage2.bytes, s));
  return nup_tv_blocks(p, (float *)out, out_stride, (const float *)in, in_stride, (const float *)in2, in2_stride, nblocks, s);
}

int clfa_nupconv_convolution_tv(clfa_nupconv *p, float *out, const float *in, const float *in2, long nblocks) {
  return blocks_host(p, out, in, in2, nblocks, [&](void *o, long len, const void *i1, const void *i2) {
    return clfa_nupconv_process_tv_dev(p, o, len, i1, len, i2, len, nblocks, p->stream);
  });
}

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
size_t clfa_nupconv_matrix_state_bytes(const clfa_nupconv_matrix *p) { return p ? nup_state_bytes(p) : 0; }
size_t clfa_nupconv_matrix_workspace_bytes(const clfa_nupconv_matrix *p) { return p ? nup_workspace_bytes(p) : 0; }
long clfa_nupconv_matrix_fade_remaining(const clfa_nupconv_matrix *p) { return p ? p->fade_len - p->fade_done : 0; }
const char *clfa_nupconv_matrix_kernel_name(const clfa_nupconv_matrix *p) { return !p || p->err ? "" : "k_nupm_mac"; }

int clfa_nupconv_matrix_push_ir_dev(clfa_nupconv_matrix *p, const void *ir, long row_stride, void *stream) {
  return nup_push_ir_dev(p, ir, row_stride, stream);
}
int clfa_nupconv_matrix_push_ir(clfa_nupconv_matrix *p, const float *ir) { return nup_push_ir_host(p, ir, nullptr); }
int clfa_nupconv_matrix_push_ir_fade_dev(clfa_nupconv_matrix *p, const void *ir, long row_stride, long fade_blocks, void *stream) {
  return nup_push_ir_fade_dev(p, ir, row_stride, fade_blocks, stream);
}
int clfa_nupconv_matrix_push_ir_fade(clfa_nupconv_matrix *p, const float *ir, long fade_blocks) {
  return nup_push_ir_host(p, ir, &fade_blocks);
}
int clfa_nupconv_matrix_process_dev(clfa_nupconv_matrix *p, void *out, long out_stride, const void *in, long in_stride,
                                    long nblocks, void *stream) {
  return nup_process_dev(p, out, out_stride, in, in_stride, nblocks, stream);
}
int clfa_nupconv_matrix_convolution(clfa_nupconv_matrix *p, float *out, const float *in, long nblocks) {
  return nup_convolution(p, out, in, nblocks);
}
int clfa_nupconv_matrix_reset(clfa_nupconv_matrix *p, void *stream) { return nup_reset(p, stream); }

}  // extern "C"
