// dev tool (not product): the resident n = 65536 kernel of the library, timed unchanged under other launch conditions.
//   hipcc -std=c++17 -O3 --offload-arch=gfx950 -fno-slp-vectorize -I opencl_fft_amd/csrc tools/res16_probe.hip -o /tmp/res16_probe
// 4096 transforms of zeros (timing only):
//   PROBE_GRID=1   fewer workgroups than CUs: does the chip need all of them to move these bytes?
//   PROBE_DELTA=1  dst = src + delta inside ONE allocation: which address relation of the two streams matters?
//   PROBE_OOP=1    in place against out of place, then ping-pong A -> B, B -> A (PROBE_PP=1: the ping-pong part only)
//   (none)         forward, then forward / inverse alternating on random data with real tables, per launch after an idle period
//   PROBE_STATIC=1 with any of them: the static transform assignment instead of the library's choice (the shared one
//                  wherever xcd_shared_ok() allows it, as launch_fft_res16 decides)
// The experiments that needed code INSIDE the kernel (parts left out, phase stamps, grid barrier, time slots, assignment
// sweeps) ended with the commit named in profiles/HISTORY.md, "The resident kernel's probe"; their results are on record there.
#include "../opencl_fft_amd/csrc/fft_resident.hip"

#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace clfa;

#define CK(x)                                                         \
  do {                                                                \
    hipError_t e = (x);                                               \
    if (e != hipSuccess) {                                            \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// ms per launch of `launch(i)`, i = 0 .. warm + reps - 1
template <class F> static float time_launches(int warm, int reps, F launch) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int i = 0; i < warm; i++) launch(i);
  CK(hipEventRecord(e0));
  for (int i = 0; i < reps; i++) launch(warm + i);
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  CK(hipGetLastError());
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return ms / reps;
}

// the shared assignment's counters (kRes16CtrBytes, zeroed once: every launch leaves them zero); null = PROBE_STATIC
static unsigned *g_ctr = nullptr;

// the complex instantiations carry the counters and the record pointer (null here) as arguments
template <bool FWD, bool SCALE> static void fft(int grid, const cpx *src, cpx *dst, cpx *slots, const cpx *tabs, long batch) {
  if (g_ctr && xcd_shared_ok(batch, (unsigned)grid))
    hipLaunchKernelGGL((k_fft_res16<FWD, SCALE, false, false, true, unsigned *, ResRecord *>), dim3(grid), dim3(256), 0, 0, src, dst, slots,
                       tabs, batch, (const cpx *)nullptr, g_ctr, (ResRecord *)nullptr);
  else
    hipLaunchKernelGGL((k_fft_res16<FWD, SCALE, false, false, false, unsigned *, ResRecord *>), dim3(grid), dim3(256), 0, 0, src, dst, slots,
                       tabs, batch, (const cpx *)nullptr, (unsigned *)nullptr, (ResRecord *)nullptr);
}

static void report(const char *name, float ms, long batch) {
  printf("%-34s %8.3f ms  %6.2f TB/s alg\n", name, ms, batch * 65536.0 * 16 / ms * 1e-9);
}

int main() {
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const long batch = 4096;
  cpx *data, *slots, *tabs;
  CK(hipMalloc(&data, batch * 65536 * 8));
  CK(hipMalloc(&slots, (size_t)cus * 32768));
  CK(hipMalloc(&tabs, 1792 * 8));
  CK(hipMemset(data, 0, batch * 65536 * 8));
  if (!getenv("PROBE_STATIC")) {
    CK(hipMalloc(&g_ctr, kRes16CtrBytes));
    CK(hipMemset(g_ctr, 0, kRes16CtrBytes));
    CK(hipDeviceSynchronize());
  }
  std::vector<cpx> t(1792);
  for (int i = 0; i < 1792; i++) t[i] = mk((float)cos(i * 0.001), (float)sin(i * 0.001));   // unit-modulus stand-ins: timing only
  CK(hipMemcpy(tabs, t.data(), 1792 * 8, hipMemcpyHostToDevice));
  printf("k_fft_res16 probe: %ld transforms, %d workgroups, %s assignment\n", batch, cus, g_ctr ? "shared" : "static");
  if (getenv("PROBE_GRID")) {
    for (int round = 0; round < 3; round++)
      for (int g : {256, 248, 240, 224, 208, 192, 160, 128}) {
        if (g > cus) continue;             // one slot per CU is all there is
        const long b2 = (batch / g) * g;   // whole rounds only
        char nm[64];
        snprintf(nm, sizeof nm, "grid %3d, %4ld transforms", g, b2);
        report(nm, time_launches(6, 30, [&](int) { fft<true, false>(g, data, data, slots, tabs, b2); }), b2);
      }
    return 0;
  }
  if (getenv("PROBE_DELTA")) {
    char *big;
    const size_t two_g = (size_t)batch * 65536 * 8;
    CK(hipMalloc(&big, 2 * two_g + (256u << 20)));
    CK(hipMemset(big, 0, 2 * two_g + (256u << 20)));
    const long deltas[] = {0, 256, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1 << 20, 2 << 20, 4 << 20, 8 << 20,
                           16 << 20, 32 << 20, 64 << 20, 128 << 20, (128 << 20) + 524288, (128 << 20) + 4096};
    for (int round = 0; round < 3; round++)
      for (int far = 0; far < 2; far++)
        for (long d : deltas) {
          const cpx *src = (const cpx *)big;
          cpx *dst = (cpx *)(big + (far ? two_g : 0) + d);
          const float ms = time_launches(6, 20, [&](int) { fft<true, false>(cus, src, dst, slots, tabs, batch); });
          printf("dst = src + %s%10ld   %8.3f ms\n", far ? "2 GiB + " : "        ", d, ms);
        }
    return 0;
  }
  if (getenv("PROBE_OOP")) {
    cpx *out2;
    CK(hipMalloc(&out2, batch * 65536 * 8));
    CK(hipMemset(out2, 0, batch * 65536 * 8));
    for (int round = 0; round < (getenv("PROBE_PP") ? 0 : 4); round++) {
      report("full, in place", time_launches(10, 40, [&](int) { fft<true, false>(cus, data, data, slots, tabs, batch); }), batch);
      report("full, OUT OF PLACE", time_launches(10, 40, [&](int) { fft<true, false>(cus, data, out2, slots, tabs, batch); }), batch);
    }
    // ping-pong: A -> B, B -> A (every buffer is read and written in turn, as a caller alternating directions would)
    for (int round = 0; round < 4; round++) {
      report("in place", time_launches(10, 40, [&](int) { fft<true, false>(cus, data, data, slots, tabs, batch); }), batch);
      report("ping-pong A -> B, B -> A",
             time_launches(10, 40, [&](int i) { fft<true, false>(cus, (i & 1) ? out2 : data, (i & 1) ? data : out2, slots, tabs, batch); }), batch);
    }
    return 0;
  }
#ifndef PROBE_OOP_ONLY   // -DPROBE_OOP_ONLY: compile the forward instantiation above only
  report("full", time_launches(10, 40, [&](int) { fft<true, false>(cus, data, data, slots, tabs, batch); }), batch);
  {
    // random data of O(1) magnitude (as bench.py), forward (scaled 1/N) / inverse alternating, per launch after an idle period
    std::vector<cpx> h(1 << 20);
    unsigned sd = 1;
    for (auto &c : h) {
      sd = sd * 1664525u + 1013904223u;
      float re = (sd >> 8) / 8388608.f - 1.f;
      sd = sd * 1664525u + 1013904223u;
      c = mk(re, (sd >> 8) / 8388608.f - 1.f);
    }
    for (long off = 0; off < batch * 65536; off += (1 << 20)) CK(hipMemcpy(data + off, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    std::vector<cpx> tt(1792);
    // real tables this time (unit-modulus stand-ins would let the values drift)
    for (int t = 0; t < 16; t++) for (int j = 0; j < 16; j++) tt[16 * t + j] = mk((float)cos(t * j * 2 * M_PI / 256), -(float)sin(t * j * 2 * M_PI / 256));
    for (int k = 0; k < 256; k++) tt[256 + k] = mk((float)cos(k * 2 * M_PI / 65536), -(float)sin(k * 2 * M_PI / 65536));
    for (int k = 0; k < 256; k++) tt[512 + k] = mk((float)cos(k * 2 * M_PI / 256), -(float)sin(k * 2 * M_PI / 256));
    for (int m = 0; m < 4; m++) for (int k = 0; k < 256; k++) { int idx = ((1 << m) * k) & 4095; tt[768 + 256 * m + k] = mk((float)cos(idx * 2 * M_PI / 4096), -(float)sin(idx * 2 * M_PI / 4096)); }
    CK(hipMemcpy(tabs, tt.data(), 1792 * 8, hipMemcpyHostToDevice));
    usleep(300000);
    const int n = 30;
    std::vector<hipEvent_t> ev(n + 1);
    for (auto &evt : ev) CK(hipEventCreate(&evt));
    CK(hipEventRecord(ev[0]));
    for (int i = 0; i < n; i++) {
      if (i & 1) fft<false, false>(cus, data, data, slots, tabs, batch);
      else fft<true, true>(cus, data, data, slots, tabs, batch);
      CK(hipEventRecord(ev[i + 1]));
    }
    CK(hipEventSynchronize(ev[n]));
    printf("%-44s", "random data, fwd/inv alternating, after idle");
    for (int i = 0; i < n; i++) {
      float ms;
      CK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      printf(" %.3f", ms);
    }
    printf("\n");
  }
#endif
  return 0;
}
