// overlap.hpp — the aliasing checks of the C ABI's entry points (plain C++: tests/test_overlap_cpu.py builds it with g++).
//
// They decide which caller buffers an entry point refuses.  On the one-launch routes that refusal is what keeps the
// kernels' __restrict__ reads correct, so every entry point uses these two and no copy of its own.
#pragma once
#include <cstddef>

namespace clfa {

// [a, a + abytes) and [b, b + bbytes) share a byte (both spans non-empty)
inline bool spans_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const char *x = (const char *)a, *y = (const char *)b;
  return x < y + bbytes && y < x + abytes;
}

// ra rows of a at a + i * sa and rb rows of b at b + k * sb bytes, len > 0 bytes each, strides >= len: does any row of a
// share a byte with any row of b?  (A single row's stride is not used: rb <= 1 takes sb = len, and ra <= 1 never reads
// sa.)  For row i of a, the rows k of b that could touch it form one interval of k.
inline bool rows_overlap(const void *a, long sa, long ra, const void *b, long sb, long rb, long len) {
  auto fdiv = [](long x, long y) { return x >= 0 ? x / y : -((-x + y - 1) / y); };   // floor, y > 0
  const long base = (long)((const char *)a - (const char *)b);   // (pointer difference as a plain offset)
  if (rb <= 1) sb = len;
  for (long i = 0; i < ra; i++) {
    const long d = base + i * sa;                  // row i of a starts d bytes after row 0 of b
    long kmin = fdiv(d - len, sb) + 1;             // k sb > d - len
    long kmax = -fdiv(-(d + len), sb) - 1;         // k sb < d + len
    kmin = kmin < 0 ? 0 : kmin;
    kmax = kmax > rb - 1 ? rb - 1 : kmax;
    if (kmin <= kmax) return true;
  }
  return false;
}

}  // namespace clfa
