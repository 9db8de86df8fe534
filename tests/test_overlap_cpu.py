"""The aliasing checks of the C ABI (opencl_fft_amd/csrc/overlap.hpp) against a brute-force byte-set comparison, on the
CPU: they decide which caller buffers the entry points refuse, and on the GPU only a handful of contract tests reach them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "overlap.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

static char arena[1 << 16];

int main() {
  std::mt19937 rng(20261016);
  auto uni = [&](long lo, long hi) { return std::uniform_int_distribution<long>(lo, hi)(rng); };
  std::vector<unsigned char> mark(sizeof(arena));
  char *const b = arena + sizeof(arena) / 2;
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
  const bool covered = hit[0] > 500 && hit[1] > 500 && neg > 0 && pos > 0 && tight > 0 && one_row > 0 && uneven > 0 && len1 > 0;
  printf(bad == 0 && covered ? "OK\n" : "FAIL (%ld mismatches)\n", bad);
  return bad == 0 && covered ? 0 : 1;
}
"""


def test_overlap_predicates_match_brute_force(tmp_path):
    """spans_overlap / rows_overlap over a few thousand seeded geometries: negative and positive offsets, stride == len,
    one row, ra != rb, len 1"""
    src, exe = tmp_path / "overlap_check.cpp", str(tmp_path / "overlap_check")
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(src),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0 and out.strip().endswith("OK"), out
