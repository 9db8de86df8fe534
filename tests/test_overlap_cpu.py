"""The aliasing checks of the C ABI and the check of a call's arrays (opencl_fft_amd/csrc/overlap.hpp) against a brute-force
byte-set comparison, on the CPU: they decide which caller buffers the entry points refuse, and on the GPU only a handful
of contract tests reach them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "overlap.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

alignas(16) static char arena[1 << 16];
static char *const b = arena + sizeof(arena) / 2;
static std::mt19937 rng(20261016);
static long uni(long lo, long hi) { return std::uniform_int_distribution<long>(lo, hi)(rng); }
static int verdict(long bad, bool covered) {
  printf(bad == 0 && covered ? "OK\n" : "FAIL (%ld mismatches)\n", bad);
  return bad == 0 && covered ? 0 : 1;
}

static int predicates() {
  std::vector<unsigned char> mark(sizeof(arena));
  long bad = 0, hit[2] = {0, 0}, neg = 0, pos = 0, tight = 0, one_row = 0, uneven = 0, len1 = 0;
  for (int t = 0; t < 4000; t++) {
    // rows: ra rows of a at stride sa, rb rows of b at stride sb, len bytes each (strides >= len; a single row's stride
    // is not used, so it is drawn from 0 up)
    const long len = t % 8 == 0 ? 1 : uni(1, 24);
    const long ra = uni(1, 5), rb = t % 3 == 0 ? ra : uni(1, 5);
    const long sa = t % 5 == 0 ? len : uni(ra > 1 ? len : 0, 3 * len + 7);
    const long sb = t % 7 == 0 ? len : uni(rb > 1 ? len : 0, 3 * len + 7);
    const long off = uni(-(ra * sa + 8), rb * sb + 8);   // a's first byte relative to b's
    char *const a = b + off;
    std::fill(mark.begin(), mark.end(), 0);
    for (long k = 0; k < rb; k++)
      for (long x = 0; x < len; x++) mark[b - arena + k * sb + x] = 1;
    bool want = false;
    for (long i = 0; i < ra; i++)
      for (long x = 0; x < len; x++) want = want || mark[a - arena + i * sa + x];
    if (clfa::rows_overlap(a, sa, ra, b, sb, rb, len) != want) {
      if (bad++ < 10) printf("rows: off %ld sa %ld ra %ld sb %ld rb %ld len %ld: want %d\n", off, sa, ra, sb, rb, len, want);
    }
    hit[want]++;
    neg += off < 0;
    pos += off > 0;
    tight += sa == len || sb == len;
    one_row += ra == 1 || rb == 1;
    uneven += ra != rb;
    len1 += len == 1;

    // spans: [a, a + abytes) and [b, b + bbytes), both non-empty
    const long abytes = t % 8 == 1 ? 1 : uni(1, 64), bbytes = t % 8 == 2 ? 1 : uni(1, 64);
    const long off2 = uni(-abytes - 8, bbytes + 8);
    std::fill(mark.begin(), mark.end(), 0);
    for (long x = 0; x < bbytes; x++) mark[b - arena + x] = 1;
    bool want2 = false;
    for (long x = 0; x < abytes; x++) want2 = want2 || mark[b - arena + off2 + x];
    if (clfa::spans_overlap(b + off2, (size_t)abytes, b, (size_t)bbytes) != want2) {
      if (bad++ < 10) printf("spans: off %ld abytes %ld bbytes %ld: want %d\n", off2, abytes, bbytes, want2);
    }
    hit[want2]++;
  }
  printf("overlap %ld, apart %ld, negative %ld, positive %ld, stride == len %ld, one row %ld, ra != rb %ld, len 1 %ld\n",
         hit[1], hit[0], neg, pos, tight, one_row, uneven, len1);
  return verdict(bad, hit[0] > 500 && hit[1] > 500 && neg > 0 && pos > 0 && tight > 0 && one_row > 0 && uneven > 0 && len1 > 0);
}

static int arrays() {
  long bad = 0;
  // the check of a call's arrays, arrays_ok: five slots of which 2..5 are arrays of the call, against the byte map.  Call
  // t is of kind t % 8: 0 random (now and then a NULL); then two arrays alone — an output sharing exactly the last byte of
  // an input (1), its first (2), none but the boundary (3), two outputs overlapping (4) — two overlapping inputs and an
  // output apart (5), an input wholly inside the gap between two rows of a strided output (6), and two arrays apart of
  // which one lies 0..7 bytes past an 8-byte boundary, align 4 and 8, with and without device_ptrs (7)
  typedef clfa::CallArray<int> Arr;
  enum { RANDOM, LAST_BYTE, FIRST_BYTE, ADJACENT, OUT_OUT, IN_IN, GAP, MISALIGNED, KINDS };
  const int expect[KINDS] = {-1, 1, 1, 0, 1, 0, 1, -1};   // refused, accepted, or as the map says
  long seen[KINDS][2] = {}, mis[2][8][2] = {}, unused = 0, null = 0;
  std::vector<unsigned char> all(sizeof(arena)), outs(sizeof(arena));
  for (int t = 0; t < 6000; t++) {
    const int kind = t % KINDS, s = t / KINDS;
    int n = kind == RANDOM ? (int)uni(2, 5) : (kind == IN_IN ? 3 : 2);
    bool device_ptrs = kind == RANDOM && uni(0, 1);
    Arr a[5];
    for (int i = 0; i < 5; i++) {
      const long rows = uni(1, 3), bytes = 8 * uni(1, 6);
      a[i] = Arr{b + 8 * uni(-60, 60), (size_t)bytes, uni(0, 1) ? 8 : 4, uni(0, 2) == 0, 0, i < n && (kind != RANDOM || uni(0, 5) > 0),
                 (size_t)rows, (size_t)(rows > 1 && uni(0, 1) ? bytes + 8 * uni(0, 4) : 0)};
    }
    if (kind == RANDOM && uni(0, 9) == 0) a[uni(0, n - 1)].ptr = nullptr;
    if (kind != RANDOM) a[0].out = false, a[1].out = true;
    if (kind == LAST_BYTE) a[1].ptr = (const char *)a[0].ptr + a[0].span() - 1;
    if (kind == FIRST_BYTE) a[1].ptr = (const char *)a[0].ptr - a[1].span() + 1;
    if (kind == ADJACENT) a[1].ptr = (const char *)a[0].ptr + (s % 2 ? (long)a[0].span() : -(long)a[1].span());
    if (kind == OUT_OUT) a[0].out = true, a[1].ptr = (const char *)a[0].ptr + uni(0, (long)a[0].span() - 1);
    if (kind == IN_IN) {
      a[1].out = false, a[1].ptr = (const char *)a[0].ptr + uni(0, (long)a[0].span() - 1);
      a[2].out = true, a[2].ptr = b + 8000;
    }
    if (kind == GAP) {   // out: rows of `bytes`, the gaps hold at least the input; in: one row somewhere inside the first gap
      a[1].rows = 2 + s % 2, a[1].pitch = a[1].bytes + a[0].bytes + 8 * uni(0, 3);
      a[0].rows = 1, a[0].pitch = 0;
      a[0].ptr = (const char *)a[1].ptr + a[1].bytes + uni(0, (long)(a[1].pitch - a[1].bytes - a[0].bytes));
    }
    if (kind == MISALIGNED) {
      const int eight = s % 2, m = (s / 2) % 8;
      device_ptrs = (s / 16) % 2;
      a[0].ptr = b + m, a[0].align = eight ? 8 : 4, a[1].ptr = b + 4000, a[1].align = 8;
      mis[eight][m][device_ptrs]++;
    }
    bool refuse = false;
    for (const Arr &x : a) {
      unused += !x.used;
      null += x.used && !x.ptr;
      refuse = refuse || (x.used && (!x.ptr || (device_ptrs && ((const char *)x.ptr - arena) % x.align != 0)));
    }
    std::fill(all.begin(), all.end(), 0);
    std::fill(outs.begin(), outs.end(), 0);
    for (const Arr &x : a) {
      if (!x.used || !x.ptr) continue;
      const long first = (const char *)x.ptr - arena, step = x.pitch ? (long)x.pitch : (long)x.bytes;
      for (long y = first; y < first + ((long)x.rows - 1) * step + (long)x.bytes; y++) all[y]++, outs[y] += x.out;
    }
    for (size_t y = 0; y < all.size(); y++) refuse = refuse || (outs[y] && all[y] >= 2);
    if (kind == GAP)   // ... and no byte of a ROW of the output is the input's: the span rule alone refuses
      for (size_t r = 0; r < a[1].rows; r++)
        if (clfa::spans_overlap((const char *)a[1].ptr + r * a[1].pitch, a[1].bytes, a[0].ptr, a[0].bytes)) bad++;
    if (clfa::arrays_ok(a, device_ptrs) == refuse || (expect[kind] >= 0 && expect[kind] != refuse)) {
      if (bad++ < 10) printf("arrays: call %d of kind %d: the map says %s\n", t, kind, refuse ? "refused" : "accepted");
    }
    seen[kind][refuse]++;
  }
  printf("arrays: random refused %ld accepted %ld, unused %ld, NULL %ld\n", seen[RANDOM][1], seen[RANDOM][0], unused, null);
  bool covered = seen[RANDOM][0] > 100 && seen[RANDOM][1] > 100 && unused > 0 && null > 0;
  for (int k = 1; k < KINDS - 1; k++) covered = covered && seen[k][expect[k]] > 0;
  for (int e = 0; e < 2; e++)
    for (int m = 0; m < 8; m++)
      for (int d = 0; d < 2; d++) covered = covered && mis[e][m][d] > 0;
  return verdict(bad, covered);
}

int main(int argc, char **argv) { return argc > 1 && !strcmp(argv[1], "arrays") ? arrays() : predicates(); }
"""


def _run(tmp_path, *args):
    src, exe = tmp_path / "overlap_check.cpp", str(tmp_path / "overlap_check")
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(src),
                           "-o", exe])
    p = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.strip().endswith("OK"), out


def test_overlap_predicates_match_brute_force(tmp_path):
    """spans_overlap / rows_overlap over a few thousand seeded geometries: negative and positive offsets, stride == len,
    one row, ra != rb, len 1"""
    _run(tmp_path)


def test_array_check_matches_brute_force(tmp_path):
    """arrays_ok over a few thousand seeded calls: unused arrays, NULL, every misalignment of 1..7 bytes for align 4 and 8
    with and without device_ptrs, an output touching an input by one byte at either end, two outputs overlapping, inputs
    overlapping each other, a strided output whose gap holds an input"""
    _run(tmp_path, "arrays")
