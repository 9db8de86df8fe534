// overlap.hpp — the argument rules of the C ABI's arrays (plain C++: tests/test_overlap_cpu.py builds it with g++): the
// two aliasing predicates, the description of one array of a call, and the check every entry point runs over its arrays.
// They decide which caller buffers an entry point refuses.  On the one-launch routes that refusal is what keeps the
// kernels' __restrict__ reads correct, so every entry point uses these and no copy of its own.
#pragma once
#include <cstddef>
#include <cstdint>

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

// One array of a call, as the caller passed it: device memory in a device form, host memory in a blocking form.  It is
// `rows` rows of `bytes` each, `pitch` bytes apart (0: packed).  An array the call does not look at (`used` false) is not
// examined, not staged, and reaches the launch as NULL.  `stage`: where a blocking form stages it (host.hpp).
template <class Stage>
struct CallArray {
  const void *ptr;
  size_t bytes;
  int align;     // what a device form asks of ptr: 8 (frames, spectra, pairs) or 4 (floats)
  bool out;      // an output of the call; else an input
  Stage stage;
  bool used = true;
  size_t rows = 1, pitch = 0;
  size_t span() const { return pitch ? (rows - 1) * pitch + bytes : rows * bytes; }   // first byte to last, gaps included
};

// The arrays' rules: a NULL is refused, so is with device_ptrs a misaligned one, so is an output whose span (a strided
// array's gaps included) shares a byte with any other array of the call; the inputs may overlap each other.
template <class A, size_t N>
inline bool arrays_ok(const A (&arrays)[N], bool device_ptrs) {
  for (const A &a : arrays)
    if (a.used && (!a.ptr || (device_ptrs && ((uintptr_t)a.ptr & (uintptr_t)(a.align - 1))))) return false;
  for (const A &out : arrays)
    for (const A &a : arrays)
      if (out.used && out.out && a.used && &a != &out && spans_overlap(a.ptr, a.span(), out.ptr, out.span())) return false;
  return true;
}

}  // namespace clfa
