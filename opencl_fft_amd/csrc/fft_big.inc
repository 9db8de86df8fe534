// fft_big.inc (part of the translation unit fft_kernels.hip) — batched 1-D FFTs of n = 2^17 .. 2^24 for gfx950
// (MI355X), composed with the launchers of fft_lds.inc and fft_4step.inc:
//   k_big2_cols / k_big2_rows (and their two-run forms `_2x`)  n <= 2^22 in two passes;
//   k_big_cols / k_big_transpose  above that, around the batched row transforms.
#include "fft_xfer.hpp"

namespace clfa {

// ---------------------------------------------------------------------------------
// n = 2^17 .. 2^24: beyond the reference's reach (its stage kernel overflows int32 above 65536,
// cl_fft.cpp:32) — an extension, composed from the kernels above
// ---------------------------------------------------------------------------------
// Above 2^22 (two passes up to there, see k_big2_*): n = N1 x N2, N1 = 128, 256 (columns), N2 = 65536 (rows):
//   1. k_big_cols: N1-point FFT down 16..128 adjacent columns of data[n1][n2], times W_n^(n2 k1),
//      to scratch[k1][n2]                                                       (16 B/sample)
//   2. the batched row kernel of this file over the n-contiguous rows of scratch, N1 * batch of them,
//      in place: k_fft_lds (N2 <= 8192, 16 B/sample) or the four-step kernel (32 B/sample)
//   3. k_big_transpose: scratch[k1][k2] -> data[k2 * N1 + k1] (natural order), times 1/n for forward
//      plans                                                                     (16 B/sample)
// Twiddles W_n^e: big_tw() below.

int big_split(int logn, BigGeom *g) {
  if (logn <= kMaxLog || logn > kBigMaxLog) return -1;
  g->logn = logn;
  if (logn <= kBig2MaxLog) {   // two passes, N1 x N2 with both <= 2048 (k_big2_cols / k_big2_rows)
    g->logn1 = (logn + (logn == 21 ? 1 : 0)) / 2;   // n = 2^21: the 2048-point factor in the columns, not the rows (2.04 -> 2.30 TB/s)
    g->logn2 = logn - g->logn1;
  } else {            // three passes
    g->logn2 = logn - 8;
    g->logn1 = logn - g->logn2;
  }
  g->two_run = true;   // (the one-run form of the 1024-point blocks lost its A/B by 1.4-6 % and left the library in round 4)
  return 0;
}

// the column / row block a workgroup takes: XCD-compact (fft_device.hpp, xcd_first; profiles/ab_big_xcd_r04.txt)
__device__ __forceinline__ int big_block() { return (int)xcd_first(blockIdx.x, gridDim.x); }
// W_n^e between the passes: e = e0 + 128 e1 + 16384 e2 from three tables of 128, 128 and n / 16384 entries (each rounded from
// double) in LDS, two multiplies: rms error of the factor 3.9e-8 where the two-table form it replaces had 3.4e-8 (a first table
// of W_n^e0 - 1, applied as a + a d, is no better: 4.0e-8), against 2.5-4e-7 of a whole transform.
// (Rounds 2-4 read two tables of 4096 and n / 4096 entries from global memory, one multiply: 64 more vector-memory instructions
// per lane and block than the 64 that move the data — without them the column passes run 12-34 % faster,
// profiles/big_two_pass_r05.txt.)
constexpr int kBigTwFixed = 256;   // entries of the first two tables
__device__ __forceinline__ void big_tw_fill(cpx *s_tw, const cpx *tw_g, int ntw, int tid, int lanes) {
  for (int i = tid; i < ntw; i += lanes) s_tw[i] = tw_g[i];
}
__device__ __forceinline__ cpx big_tw(const cpx *s_tw, int ex) {
  return cmul(cmul(s_tw[ex & 127], s_tw[128 + ((ex >> 7) & 127)]), s_tw[kBigTwFixed + (ex >> 14)]);
}
template <int LOGN1, bool FWD>
__global__ __launch_bounds__(256) void k_big_cols(const cpx *__restrict__ data, cpx *__restrict__ scratch,
                                                  const cpx *__restrict__ tabs_g, int logn2, int ntw) {
  constexpr int N1 = 1 << LOGN1, T1 = N1 / 16, C1 = 256 / T1;
  __shared__ cpx s_tab1[N1 / 2];
  __shared__ cpx s_tw[kBigTwFixed + (1 << (kBigMaxLog - 14))];
  __shared__ cpx s_x[N1 * C1];
  const int tid = threadIdx.x;
  for (int i = tid; i < N1 / 2; i += 256) s_tab1[i] = tabs_g[i];
  big_tw_fill(s_tw, tabs_g + N1 / 2, ntw, tid, 256);
  const int col = tid % C1, tf = tid / C1;
  const int n2 = big_block() * C1 + col;
  const long base = ((long)blockIdx.y << (LOGN1 + logn2)) + n2;
  cpx v[16];
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = ld_nt(data + base + ((long)(tf + T1 * e) << logn2));
  __syncthreads();
  pass_compute<LOGN1, 4, 0, FWD>(v, tf, s_tab1);
  pass_scatter<LOGN1, 4, 0>(v, tf, [&](int p, cpx val) { s_x[p * C1 + col] = val; });
  __syncthreads();
  pass_gather<LOGN1, 4>(v, tf, [&](int p) { return s_x[p * C1 + col]; });
  pass_compute<LOGN1, 4, 4, FWD>(v, tf, s_tab1);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k1 = tf + T1 * e;
    const int ex = n2 * k1;  // < n <= 2^24
    scratch[base + ((long)k1 << logn2)] = cmulc<!FWD>(v[e], big_tw(s_tw, ex));
  }
}

template <int LOGN1, bool SCALE>
__global__ __launch_bounds__(256) void k_big_transpose(const cpx *__restrict__ scratch, cpx *__restrict__ data,
                                                       int logn2, float inv_n) {
  constexpr int N1 = 1 << LOGN1, TK1 = N1 < 64 ? N1 : 64, TK2 = 4096 / TK1;
  __shared__ cpx tile[TK1 * (TK2 + 1)];
  const int tid = threadIdx.x;
  const int k2_0 = big_block() * TK2, k1_0 = blockIdx.y * TK1;
  const long tbase = (long)blockIdx.z << (LOGN1 + logn2);
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int i = tid + 256 * r, k1 = i / TK2, k2 = i % TK2;
    tile[k1 * (TK2 + 1) + k2] = scratch[tbase + ((long)(k1_0 + k1) << logn2) + k2_0 + k2];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int i = tid + 256 * r, k2 = i / TK1, k1 = i % TK1;
    cpx o = tile[k1 * (TK2 + 1) + k2];
    if constexpr (SCALE) o = cscale(o, inv_n);
    st_nt(data + tbase + ((long)(k2_0 + k2) << LOGN1) + k1_0 + k1, o);
  }
}

template <int LOGN1>
static hipError_t launch_big_n1(const BigGeom &g, bool fwd, bool scale, cpx *data, cpx *out, cpx *scratch, cpx *scratch2,
                                const cpx *bigtabs, const FftTables &sub, long batch, const DeviceInfo &di,
                                hipStream_t s) {
  constexpr int N1 = 1 << LOGN1, T1 = N1 / 16, C1 = 256 / T1, TK1 = N1 < 64 ? N1 : 64, TK2 = 4096 / TK1;
  const int n2 = 1 << g.logn2;
  const dim3 gc(n2 / C1, (unsigned)batch), gt(n2 / TK2, N1 / TK1, (unsigned)batch);
  if (fwd) hipLaunchKernelGGL((k_big_cols<LOGN1, true>), gc, dim3(256), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  else hipLaunchKernelGGL((k_big_cols<LOGN1, false>), gc, dim3(256), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (g.logn2 <= kLdsMaxLog) e = launch_fft_lds(g.logn2, fwd, MODE_C2C, false, scratch, sub, batch * N1, di, s, 0);
  else e = launch_fft_4step(g.logn2, fwd, false, scratch, scratch2, sub, batch * N1, di, s, 0);
  if (e != hipSuccess) return e;
  const float inv_n = 1.0f / (float)(1L << g.logn);
  if (scale) hipLaunchKernelGGL((k_big_transpose<LOGN1, true>), gt, dim3(256), 0, s, scratch, out, g.logn2, inv_n);
  else hipLaunchKernelGGL((k_big_transpose<LOGN1, false>), gt, dim3(256), 0, s, scratch, out, g.logn2, inv_n);
  return hipGetLastError();
}

// ---- n = 2^17 .. 2^22 in TWO passes (32 B/sample): both factors <= 2048, so a block of 16 columns
// (pass 1) or 16 rows (pass 2) of one transform fits the LDS of a CU (128-139 KiB, one workgroup of
// N1 resp. N2 lanes per CU) and both passes move 128-byte segments:
//   k_big2_cols: data[n1][16 columns] -> N1-point FFTs, times W_n^(n2 k1) -> scratch[k1][n2]
//   k_big2_rows: scratch[16 rows k1][n2] -> N2-point FFTs -> data[k2 * N1 + k1] (natural order)
template <int LOGN1, int LOGNS, bool FWD>
__device__ __forceinline__ void col_passes(cpx (&v)[16], int tf, const cpx *tab, cpx *sx, int col) {
  pass_compute<LOGN1, 4, LOGNS, FWD>(v, tf, tab);
  constexpr int LOGR = pass_logr(LOGN1, 4, LOGNS);
  if constexpr (LOGNS + LOGR < LOGN1) {
    __syncthreads();
    pass_scatter<LOGN1, 4, LOGNS>(v, tf, [&](int p, cpx val) { sx[p * 16 + col] = val; });
    __syncthreads();
    pass_gather<LOGN1, 4>(v, tf, [&](int p) { return sx[p * 16 + col]; });
    col_passes<LOGN1, LOGNS + LOGR, FWD>(v, tf, tab, sx, col);
  }
}
template <int LOGN1, bool FWD>
__global__ __launch_bounds__(1 << LOGN1) void k_big2_cols(const cpx *__restrict__ data, cpx *__restrict__ scratch,
                                                          const cpx *__restrict__ tabs_g, int logn2, int ntw) {
  constexpr int N1 = 1 << LOGN1, T1 = N1 / 16;
  __shared__ cpx s_tab1[N1 / 2];
  __shared__ cpx s_tw[kBigTwFixed + (1 << (2 * LOGN1 + 1 - 14))];   // n <= 2^(2 LOGN1 + 1)
  __shared__ cpx s_x[N1 * 16];
  const int tid = threadIdx.x;
  for (int i = tid; i < N1 / 2; i += N1) s_tab1[i] = tabs_g[i];
  big_tw_fill(s_tw, tabs_g + N1 / 2, ntw, tid, N1);
  const int col = tid % 16, tf = tid / 16;
  const int n2 = big_block() * 16 + col;
  const long base = ((long)blockIdx.y << (LOGN1 + logn2)) + n2;
  cpx v[16];
#pragma unroll
  for (int e = 0; e < 16; e++) v[e] = ld_nt(data + base + ((long)(tf + T1 * e) << logn2));
  __syncthreads();
  col_passes<LOGN1, 0, FWD>(v, tf, s_tab1, s_x, col);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k1 = tf + T1 * e;
    const int ex = n2 * k1;  // < n <= 2^19
    scratch[base + ((long)k1 << logn2)] = cmulc<!FWD>(v[e], big_tw(s_tw, ex));
  }
}

// N1 = 1024 in the two-run form of k_cfft_2x (DESIGN.md section 4.1b): the block's 16 columns x 1024 rows as two
// 512-point runs per column (even / odd rows) through ONE 64 KiB exchange buffer and a radix-2 step in registers —
// 512 lanes and half the LDS, so two workgroups share a CU where the one-run form (128 KiB) leaves one
// (LOGC = 10, round 5: N1 = 2048 as two 1024-point runs, 1024 lanes and 140 KiB of LDS, one workgroup per CU — what puts
// n = 2^21 and 2^22 on two passes of 128-byte segments: 1.70 -> 2.30 / 2.12 TB/s algorithmic.  Blocks of 8 columns, the other
// way to fit 2048 rows into LDS, copy at 3.8-4.1 TB/s against 5.3 for 16; a persistent form of both kernels that loads the
// next block under the stores of this one measured slower (profiles/big_two_pass_r05.txt).)
template <int LOGC, bool FWD>
__global__ __launch_bounds__(1 << LOGC, LOGC == 9 ? 4 : 1) void k_big2_cols_2x(const cpx *__restrict__ data, cpx *__restrict__ scratch,
                                                         const cpx *__restrict__ tabs_g, int logn2, int ntw) {
  constexpr int M = 1 << LOGC, TC = M / 16;   // M-point runs, TC lanes per column
  __shared__ cpx s_tabh[M / 2];   // W_M^k
  __shared__ cpx s_tabj[M];       // W_2M^k, k < M (the radix-2 step)
  __shared__ cpx s_tw[kBigTwFixed + (1 << (2 * (LOGC + 1) - 14))];   // n <= 2^(2 (LOGC + 1))
  __shared__ cpx s_x[M * 16];
  const int tid = threadIdx.x;
  s_tabj[tid] = tabs_g[tid];
  if (tid < M / 2) s_tabh[tid] = tabs_g[2 * tid];
  big_tw_fill(s_tw, tabs_g + M, ntw, tid, M);
  const int col = tid % 16, tf = tid / 16;
  const int n2 = big_block() * 16 + col;
  const long base = ((long)blockIdx.y << (LOGC + 1 + logn2)) + n2;
  cpx va[16], vb[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    va[e] = ld_nt(data + base + ((long)(2 * (tf + TC * e)) << logn2));
    vb[e] = ld_nt(data + base + ((long)(2 * (tf + TC * e) + 1) << logn2));
  }
  __syncthreads();
  col_passes<LOGC, 0, FWD>(va, tf, s_tabh, s_x, col);
  __syncthreads();
  col_passes<LOGC, 0, FWD>(vb, tf, s_tabh, s_x, col);
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k = tf + TC * e;
    const cpx p = cmulc<!FWD>(vb[e], s_tabj[k]);
    const cpx o0 = cadd(va[e], p), o1 = csub(va[e], p);
    const int ex0 = n2 * k, ex1 = n2 * (k + M);  // < n <= 2^22
    scratch[base + ((long)k << logn2)] = cmulc<!FWD>(o0, big_tw(s_tw, ex0));
    scratch[base + ((long)(k + M) << logn2)] = cmulc<!FWD>(o1, big_tw(s_tw, ex1));
  }
}

// all passes but the last with the lanes of a row adjacent (tf fast); the last one with the 16 rows on
// the fast lane index, so that the transposed store is 128-byte segments
template <int LOGN2, int LOGNS, bool FWD>
__device__ __forceinline__ void row_passes(cpx (&v)[16], int l, const cpx *tab, cpx *sx) {
  constexpr int T2 = (1 << LOGN2) / 16, S2 = lds_padded_size(1 << LOGN2) | 1;
  constexpr int LOGR = pass_logr(LOGN2, 4, LOGNS), NEXT = LOGNS + LOGR;
  const int tf = l % T2, row = l / T2;
  pass_compute<LOGN2, 4, LOGNS, FWD>(v, tf, tab);
  __syncthreads();
  pass_scatter_padded<LOGN2, 4, LOGNS>(v, tf, sx + row * S2);
  __syncthreads();
  if constexpr (NEXT + pass_logr(LOGN2, 4, NEXT) < LOGN2) {
    pass_gather_padded<LOGN2, 4>(v, tf, sx + row * S2);
    row_passes<LOGN2, NEXT, FWD>(v, l, tab, sx);
  } else {
    const int row2 = l % 16, tf2 = l / 16;
    pass_gather_padded<LOGN2, 4>(v, tf2, sx + row2 * S2);
    pass_compute<LOGN2, 4, NEXT, FWD>(v, tf2, tab);
  }
}
template <int LOGN2, bool FWD, bool SCALE>
__global__ __launch_bounds__(1 << LOGN2) void k_big2_rows(const cpx *__restrict__ scratch, cpx *__restrict__ data,
                                                          const cpx *__restrict__ tab_g, int logn1, float inv_n) {
  constexpr int N2 = 1 << LOGN2, T2 = N2 / 16, S2 = lds_padded_size(N2) | 1;
  __shared__ cpx s_tab2[N2 / 2];
  __shared__ cpx s_x[16 * S2];
  const int l = threadIdx.x;
  for (int i = l; i < N2 / 2; i += N2) s_tab2[i] = tab_g[i];
  const long tbase = (long)blockIdx.y << (LOGN2 + logn1);
  cpx v[16];
  {
    const int tf = l % T2, row = l / T2;
    const cpx *p = scratch + tbase + ((long)(big_block() * 16 + row) << LOGN2) + tf;
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = p[T2 * e];
  }
  __syncthreads();
  row_passes<LOGN2, 0, FWD>(v, l, s_tab2, s_x);
  const int row2 = l % 16, tf2 = l / 16;
  cpx *dst = data + tbase + big_block() * 16 + row2;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    cpx o = v[e];
    if constexpr (SCALE) o = cscale(o, inv_n);
    st_nt(dst + ((long)(tf2 + T2 * e) << logn1), o);
  }
}

// N2 = 1024 in the two-run form: 16 rows x 1024 points as two 512-point runs per row (one 16-byte load per lane brings
// an even and an odd sample), the last pass with the rows on the fast lane index as above, radix-2 step in registers
template <int LOGC, bool FWD, bool SCALE>
__global__ __launch_bounds__(1 << LOGC, LOGC == 9 ? 4 : 1) void k_big2_rows_2x(const cpx *__restrict__ scratch, cpx *__restrict__ data,
                                                         const cpx *__restrict__ tab_g, int logn1, float inv_n) {
  constexpr int M = 1 << LOGC, TC = M / 16, S2 = lds_padded_size(M) | 1;
  __shared__ cpx s_tabh[M / 2];   // W_M^k
  __shared__ cpx s_tabj[M];       // W_2M^k, k < M
  __shared__ cpx s_x[16 * S2];
  const int l = threadIdx.x;
  s_tabj[l] = tab_g[l];
  if (l < M / 2) s_tabh[l] = tab_g[2 * l];
  const long tbase = (long)blockIdx.y << (LOGC + 1 + logn1);
  cpx va[16], vb[16];
  {
    const int tf = l % TC, row = l / TC;
    const cpx *p = scratch + tbase + ((long)(big_block() * 16 + row) << (LOGC + 1)) + 2 * tf;
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const f4v q = *reinterpret_cast<const f4v *>(p + 2 * TC * e);
      va[e] = mk(q.x, q.y);
      vb[e] = mk(q.z, q.w);
    }
  }
  __syncthreads();
  row_passes<LOGC, 0, FWD>(va, l, s_tabh, s_x);
  __syncthreads();
  row_passes<LOGC, 0, FWD>(vb, l, s_tabh, s_x);
  const int row2 = l % 16, tf2 = l / 16;
  cpx *dst = data + tbase + big_block() * 16 + row2;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int k = tf2 + TC * e;
    const cpx p = cmulc<!FWD>(vb[e], s_tabj[k]);
    cpx o0 = cadd(va[e], p), o1 = csub(va[e], p);
    if constexpr (SCALE) {
      o0 = cscale(o0, inv_n);
      o1 = cscale(o1, inv_n);
    }
    st_nt(dst + ((long)k << logn1), o0);
    st_nt(dst + ((long)(k + M) << logn1), o1);
  }
}

template <int LOGN1>
static hipError_t launch_big2_cols(const BigGeom &g, bool fwd, const cpx *data, cpx *scratch, const cpx *bigtabs,
                                   long batch, hipStream_t s) {
  const dim3 grid((1 << g.logn2) / 16, (unsigned)batch);
  if (fwd) hipLaunchKernelGGL((k_big2_cols<LOGN1, true>), grid, dim3(1 << LOGN1), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  else hipLaunchKernelGGL((k_big2_cols<LOGN1, false>), grid, dim3(1 << LOGN1), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  return hipGetLastError();
}
template <int LOGN2>
static hipError_t launch_big2_rows(const BigGeom &g, bool fwd, bool scale, const cpx *scratch, cpx *data,
                                   const cpx *half2, long batch, hipStream_t s) {
  const dim3 grid((1 << g.logn1) / 16, (unsigned)batch);
  const float inv_n = 1.0f / (float)(1L << g.logn);
  if (fwd && scale) hipLaunchKernelGGL((k_big2_rows<LOGN2, true, true>), grid, dim3(1 << LOGN2), 0, s, scratch, data, half2, g.logn1, inv_n);
  else if (fwd) hipLaunchKernelGGL((k_big2_rows<LOGN2, true, false>), grid, dim3(1 << LOGN2), 0, s, scratch, data, half2, g.logn1, inv_n);
  else hipLaunchKernelGGL((k_big2_rows<LOGN2, false, false>), grid, dim3(1 << LOGN2), 0, s, scratch, data, half2, g.logn1, inv_n);
  return hipGetLastError();
}
template <int LOGC>
static hipError_t launch_big2_cols_2x(const BigGeom &g, bool fwd, const cpx *data, cpx *scratch, const cpx *bigtabs, long batch, hipStream_t s) {
  const dim3 grid((1 << g.logn2) / 16, (unsigned)batch);
  if (fwd) hipLaunchKernelGGL((k_big2_cols_2x<LOGC, true>), grid, dim3(1 << LOGC), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  else hipLaunchKernelGGL((k_big2_cols_2x<LOGC, false>), grid, dim3(1 << LOGC), 0, s, data, scratch, bigtabs, g.logn2, kBigTwFixed + (1 << (g.logn > 14 ? g.logn - 14 : 0)));
  return hipGetLastError();
}
template <int LOGC>
static hipError_t launch_big2_rows_2x(const BigGeom &g, bool fwd, bool scale, const cpx *scratch, cpx *out, const cpx *half2, long batch, hipStream_t s) {
  const dim3 grid((1 << g.logn1) / 16, (unsigned)batch);
  const float inv_n = 1.0f / (float)(1L << g.logn);
  if (fwd && scale) hipLaunchKernelGGL((k_big2_rows_2x<LOGC, true, true>), grid, dim3(1 << LOGC), 0, s, scratch, out, half2, g.logn1, inv_n);
  else if (fwd) hipLaunchKernelGGL((k_big2_rows_2x<LOGC, true, false>), grid, dim3(1 << LOGC), 0, s, scratch, out, half2, g.logn1, inv_n);
  else hipLaunchKernelGGL((k_big2_rows_2x<LOGC, false, false>), grid, dim3(1 << LOGC), 0, s, scratch, out, half2, g.logn1, inv_n);
  return hipGetLastError();
}
static hipError_t launch_fft_big2(const BigGeom &g, bool fwd, bool scale, cpx *data, cpx *out, cpx *scratch, const cpx *bigtabs,
                                  const FftTables &sub, long batch, hipStream_t s) {
  hipError_t e;
  switch (g.logn1) {
    case 8: e = launch_big2_cols<8>(g, fwd, data, scratch, bigtabs, batch, s); break;
    case 9: e = launch_big2_cols<9>(g, fwd, data, scratch, bigtabs, batch, s); break;
    case 10: e = launch_big2_cols_2x<9>(g, fwd, data, scratch, bigtabs, batch, s); break;    // 1024-point columns as two 512-point runs (two workgroups per CU)
    case 11: e = launch_big2_cols_2x<10>(g, fwd, data, scratch, bigtabs, batch, s); break;   // 2048-point columns as two 1024-point runs
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  switch (g.logn2) {
    case 9: return launch_big2_rows<9>(g, fwd, scale, scratch, out, sub.half, batch, s);
    case 10: return launch_big2_rows_2x<9>(g, fwd, scale, scratch, out, sub.half, batch, s);
    case 11: return launch_big2_rows_2x<10>(g, fwd, scale, scratch, out, sub.half, batch, s);
    default: return hipErrorInvalidValue;
  }
}

// scratch: `batch` transforms (the caller chunks); scratch2: the four-step workspace when N2 > 8192
hipError_t launch_fft_big(const BigGeom &g, bool fwd, bool scale, cpx *data, cpx *out, cpx *scratch, cpx *scratch2,
                          const cpx *bigtabs, const FftTables &sub, long batch, const DeviceInfo &di, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  if (batch > 65535) return hipErrorInvalidValue;
  if (g.logn <= kBig2MaxLog) return launch_fft_big2(g, fwd, scale, data, out, scratch, bigtabs, sub, batch, s);
  switch (g.logn1) {
    case 5: return launch_big_n1<5>(g, fwd, scale, data, out, scratch, scratch2, bigtabs, sub, batch, di, s);
    case 6: return launch_big_n1<6>(g, fwd, scale, data, out, scratch, scratch2, bigtabs, sub, batch, di, s);
    case 7: return launch_big_n1<7>(g, fwd, scale, data, out, scratch, scratch2, bigtabs, sub, batch, di, s);
    case 8: return launch_big_n1<8>(g, fwd, scale, data, out, scratch, scratch2, bigtabs, sub, batch, di, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace clfa
