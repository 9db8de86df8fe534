// pconv_nupm.hip — the multiply-accumulate of the non-uniformly partitioned convolution matrix (clfa_nupconv_matrix,
// nupconv_host.cpp): `inputs` signals into `outputs` signals through outputs x inputs responses held on two levels, a head of
// small partitions (pts0) and a tail of large ones (pts1 = m * pts0) whose blocks are multiplied in m slices of their bins.
//   k_nupm_mac     one segment's sum over r = i * nparts + p, ascending, of  A_i[(w - (nparts - 1) + p) mod ring] (.)
//                  H_{o,i}[nparts - 1 - p]  for ONE block of a level over a range of its 16-byte items: the terms, their
//                  order and the segments of k_pconvm_mac, hence its bits, however the bins are cut into slices.  A
//                  single-block call runs the head's block and the tail's slice in one launch of it; a fade's block runs
//                  both under both response sets (four jobs)
//   k_nupm_reduce  Y = ((Y + P[0]) + P[1]) + ... of the jobs with more than one segment, the order of k_pconvm_reduce
// Everything around them exists: the transforms are launch_pconvb_forward / launch_pconvb_inverse with K = 1, the stage row
// and the mix are k_nupc_stage / k_nupc_mix (pconv_nup.hip) over inputs / outputs rows, and calls of several blocks run the
// head through launch_pconv_matrix over the same ring, responses and tails.  No atomics and no hand-overs between
// workgroups: stream order alone.
#include "pconv_device.hpp"
#include "pconv_launch.hpp"

namespace clfa {

namespace {

__device__ __forceinline__ cpx2 ld_plain(const cpx2 *p) { return *p; }

}  // namespace

template <int NJ> struct NupmMacJobs { NupmMacJob j[NJ]; };

// blockIdx.y picks the job (selects, not an index into the kernel's arguments)
template <int NJ>
__device__ __forceinline__ const NupmMacJob &nupm_pick(const NupmMacJobs<NJ> &jobs) {
  static_assert(NJ == 2 || NJ == kNupmMacJobs, "two jobs, or a fade's four");
  return NJ > 2 && blockIdx.y >= 2 ? (blockIdx.y == 3 ? jobs.j[NJ - 1] : jobs.j[NJ - 2]) : (blockIdx.y ? jobs.j[1] : jobs.j[0]);
}

// ---------------------------------------------------------------------------------
// One lane = (segment, output, item), the lanes laid over all three together, so that a slice of 16 items and a handful of
// outputs still fill their waves.  A segment is one serial chain per lane (the order is the result's bits), so what hides
// the memory latency is depth: the loads of D terms are in flight together.  The queue's head walks (i, p) by counting,
// without a division per term, and stays on the last term of the whole sequence once it is there; terms past the end of
// the segment are loaded (they are the next segment's, valid memory) and dropped by a select.  Response frames are read
// once per block: non-temporal loads.  Input frames are read by every output: plain loads, which may hit the CU's L1
// (measured against non-temporal ones: profiles/HISTORY.md).  An input's frames are `ring` apart: the tail's ring keeps
// more frames than the sum walks.
// ---------------------------------------------------------------------------------
template <int D, int NJ>
__global__ __launch_bounds__(64) void k_nupm_mac(NupmMacJobs<NJ> jobs, int inputs, int outputs) {
  const NupmMacJob &job = nupm_pick(jobs);
  const cpx *__restrict__ ringA = job.ringA;
  const cpx *__restrict__ H = job.H;
  const int w = job.w, bins = job.bins, nparts = job.nparts, ring = job.ring, segs = job.segs, item0 = job.item0, nitems = job.nitems;
  const long lanes = (long)segs * outputs * nitems;
  if (blockIdx.x * 64L >= lanes) return;   // (the grid is the larger job's)
  const int hb = bins >> 1;
  const long gid = blockIdx.x * 64L + threadIdx.x;
  const long g = gid < lanes ? gid : lanes - 1;   // (clamped: straight-line loads; the store is guarded)
  const int item = item0 + (int)(g % nitems);
  const long rest = g / nitems;
  const int o = (int)(rest % outputs), s = (int)(rest / outputs);
  const long total = (long)inputs * nparts;
  const long r0 = total * s / segs, r1 = total * (s + 1) / segs;   // r0 <= total - 1
  const cpx2 *xa = reinterpret_cast<const cpx2 *>(ringA) + item;
  const cpx2 *ha = reinterpret_cast<const cpx2 *>(H + (long)o * inputs * nparts * bins) + item;
  // the queue's head: term r = hi * nparts + hp
  long hr = r0;
  int hi = (int)(r0 / nparts), hp = (int)(r0 - (long)hi * nparts);
  auto fetch = [&](cpx2 &x, cpx2 &h) {
    int f = w - (nparts - 1) + hp;
    f = f < 0 ? f + ring : f;
    x = ld_plain(xa + ((long)hi * ring + f) * hb);
    h = ld_nt(ha + ((long)hi * nparts + (nparts - 1 - hp)) * hb);
    const int more = hr + 1 < total ? 1 : 0;
    hr += more;
    hp += more;
    const bool wrap = hp == nparts;
    hp = wrap ? 0 : hp;
    hi += wrap ? 1 : 0;
  };
  const bool dc = item == 0;   // packed DC / Nyquist bin: (re*re, im*im)
  cpx s0 = mk(0.f, 0.f), s1 = mk(0.f, 0.f);
  cpx2 xq[D], hq[D];
#pragma unroll
  for (int d = 0; d < D; d++) fetch(xq[d], hq[d]);
  for (long q = r0; q < r1; q += D) {
#pragma unroll
    for (int d = 0; d < D; d++) {
      const cpx2 x = xq[d], h = hq[d];
      fetch(xq[d], hq[d]);
      // past the end of the segment the term is dropped by a select on the sums, not by a branch: a branch in the body ends
      // the overlap of the loads with the arithmetic
      cpx t0 = s0, t1 = s1;
      mac_term(t0, t1, x, h, dc);
      const bool live = q + d < r1;
      s0 = mk(live ? t0.x : s0.x, live ? t0.y : s0.y);
      s1 = mk(live ? t1.x : s1.x, live ? t1.y : s1.y);
    }
  }
  if (gid < lanes) {
    cpx2 v;
    v.a = s0;
    v.b = s1;
    cpx *dst = s == 0 ? job.Y + (long)o * bins : job.P + ((long)(s - 1) * outputs + o) * bins;
    reinterpret_cast<cpx2 *>(dst)[item] = v;
  }
}

// ---------------------------------------------------------------------------------
// the segments' partial sums, added in ascending segment order: Y = ((Y + P[0]) + P[1]) + ..., one lane = (output, item)
// ---------------------------------------------------------------------------------
template <int NJ>
__global__ __launch_bounds__(64) void k_nupm_reduce(NupmMacJobs<NJ> jobs, int outputs) {
  const NupmMacJob &job = nupm_pick(jobs);
  const int segs = job.segs, nitems = job.nitems, hb = job.bins >> 1;
  const long lanes = (long)outputs * nitems;
  const long gid = blockIdx.x * 64L + threadIdx.x;
  if (segs < 2 || gid >= lanes) return;
  const int item = job.item0 + (int)(gid % nitems), o = (int)(gid / nitems);
  cpx2 *y = reinterpret_cast<cpx2 *>(job.Y) + (long)o * hb + item;
  const cpx2 *q = reinterpret_cast<const cpx2 *>(job.P) + (long)o * hb + item;
  const long pstride = (long)outputs * hb;   // one segment's partials, in cpx2
  cpx2 v = *y;
  // the additions are one chain, the loads are not: eight partials in flight (past the last one: clamped, dropped)
  for (int s0 = 1; s0 < segs; s0 += 8) {
    cpx2 u[8];
#pragma unroll
    for (int k = 0; k < 8; k++) u[k] = q[(long)((s0 + k < segs ? s0 + k : segs - 1) - 1) * pstride];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool live = s0 + k < segs;
      const cpx a = cadd(v.a, u[k].a), b = cadd(v.b, u[k].b);
      v.a = mk(live ? a.x : v.a.x, live ? a.y : v.a.y);
      v.b = mk(live ? b.x : v.b.x, live ? b.y : v.b.y);
    }
  }
  *y = v;
}

// ---------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------
static bool nupm_job_ok(const NupmMacJob &j) {
  return j.ringA && j.H && j.Y && j.bins >= 2 && j.item0 >= 0 && j.nitems >= 1 && j.item0 + j.nitems <= j.bins / 2 && j.nparts >= 1 &&
         j.ring >= j.nparts && j.w >= 0 && j.w < j.ring && j.segs >= 1 && (j.segs == 1 || j.P);
}

hipError_t launch_nupm_mac(const NupmMacJob *jobs, int njobs, int inputs, int outputs, hipStream_t s) {
  if (njobs < 1 || njobs > kNupmMacJobs || inputs < 1 || outputs < 1) return hipErrorInvalidValue;
  long blocks = 0;
  for (int i = 0; i < njobs; i++) {
    if (!nupm_job_ok(jobs[i])) return hipErrorInvalidValue;
    const long b = ((long)jobs[i].segs * outputs * jobs[i].nitems + 63) / 64;
    blocks = b > blocks ? b : blocks;
  }
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  // (jobs past njobs repeat the last one: blockIdx.y never picks them)
  if (njobs > 2) {
    NupmMacJobs<kNupmMacJobs> a;
    for (int i = 0; i < kNupmMacJobs; i++) a.j[i] = jobs[i < njobs ? i : njobs - 1];
    hipLaunchKernelGGL((k_nupm_mac<kNupmMacDepth, kNupmMacJobs>), dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, inputs, outputs);
  } else {
    const NupmMacJobs<2> a = {{jobs[0], jobs[njobs - 1]}};
    hipLaunchKernelGGL((k_nupm_mac<kNupmMacDepth, 2>), dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, inputs, outputs);
  }
  return hipGetLastError();
}

hipError_t launch_nupm_reduce(const NupmMacJob *jobs, int njobs, int outputs, hipStream_t s) {
  if (njobs < 1 || njobs > kNupmMacJobs || outputs < 1) return hipErrorInvalidValue;
  long blocks = 0;
  for (int i = 0; i < njobs; i++) {
    if (!nupm_job_ok(jobs[i])) return hipErrorInvalidValue;
    if (jobs[i].segs < 2) continue;
    const long b = ((long)outputs * jobs[i].nitems + 63) / 64;
    blocks = b > blocks ? b : blocks;
  }
  if (!blocks) return hipSuccess;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  if (njobs > 2) {
    NupmMacJobs<kNupmMacJobs> a;
    for (int i = 0; i < kNupmMacJobs; i++) a.j[i] = jobs[i < njobs ? i : njobs - 1];
    hipLaunchKernelGGL(k_nupm_reduce<kNupmMacJobs>, dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, outputs);
  } else {
    const NupmMacJobs<2> a = {{jobs[0], jobs[njobs - 1]}};
    hipLaunchKernelGGL(k_nupm_reduce<2>, dim3((unsigned)blocks, njobs), dim3(64), 0, s, a, outputs);
  }
  return hipGetLastError();
}

}  // namespace clfa
