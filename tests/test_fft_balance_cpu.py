"""The resident n = 65536 kernel's shared assignment on the CPU (opencl_fft_amd/csrc/fft_device.hpp, beside xcd_first()):
a g++-built program prints, for every batch of tests/test_gpu_fft_balance.py and every grid that is a multiple of 8 up
to 256, each XCD's share and the transforms its positions map to; this file checks them against the static assignment
written out on its own: per XCD the same transforms in the same order, all XCDs together every transform exactly once,
and every position beyond a share beyond the batch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = [255, 256, 257, 300, 511, 513, 777, 1029]

PROGRAM = r"""
#include "fft_device.hpp"

#include <cstdio>
#include <cstdlib>

using namespace clfa;

int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    const unsigned batch = (unsigned)atoi(argv[a]);
    for (unsigned grid = 8; grid <= 256; grid += 8) {
      printf("B %u %u %d\n", batch, grid, (int)xcd_shared_ok((long)batch, grid));
      for (unsigned x = 0; x < 8; x++) {
        const unsigned share = xcd_share(x, grid, batch);
        printf("X %u %u", x, share);
        // the share, and a window's worth of positions beyond it
        for (unsigned p = 0; p < share + grid / 8 + 1; p++) printf(" %u", xcd_transform(x, grid, p));
        printf("\n");
      }
    }
  }
  // where it does not apply: grids that are no multiple of 8, one transform per workgroup or fewer, indices beyond 32 bits
  printf("N %d %d %d %d %d %d\n", (int)xcd_shared_ok(1000, 255), (int)xcd_shared_ok(256, 256), (int)xcd_shared_ok(100, 256),
         (int)xcd_shared_ok(1L << 31, 256), (int)xcd_shared_ok(9, 8), (int)xcd_shared_ok(1000, 4));
  return 0;
}
"""


def static_order(x, grid, batch):
    """the transforms the workgroups of XCD x take under the static assignment, iteration by iteration: workgroup
    i = x + 8 c starts at x (grid / 8) + c and steps by the grid"""
    w = grid // 8
    out, it = [], 0
    while it * grid < batch:
        out += [it * grid + x * w + c for c in range(w) if it * grid + x * w + c < batch]
        it += 1
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("fft_balance")
    src = d / "fft_balance_check.cpp"
    src.write_text(PROGRAM)

    def build(name, *flags):
        exe = str(d / name)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"),
                               str(src), "-o", exe])
        return exe
    return build


def _lines(exe):
    p = subprocess.run([exe] + [str(b) for b in BATCHES], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    return out.strip().split("\n")


def test_positions_cover_every_transform_once_in_the_static_order(program):
    lines = _lines(program("fft_balance_check"))
    cases, batch, grid, seen = 0, None, None, None
    for ln in lines:
        f = ln.split()
        if f[0] == "B":
            if seen is not None:
                assert sorted(seen) == list(range(batch)), (batch, grid)
                cases += 1
            batch, grid, seen = int(f[1]), int(f[2]), []
            assert int(f[3]) == (batch > grid), ln
        elif f[0] == "X":
            x, share, t = int(f[1]), int(f[2]), [int(v) for v in f[3:]]
            assert t[:share] == static_order(x, grid, batch), (batch, grid, x)
            assert len(t) > share and all(v >= batch for v in t[share:]), (batch, grid, x)   # beyond the share: beyond the batch
            assert t == sorted(t)
            seen += t[:share]
        else:
            assert ln == "N 0 0 0 0 1 0"
    assert sorted(seen) == list(range(batch))
    assert cases + 1 == len(BATCHES) * 32


def test_balance_program_under_sanitizers(program):
    """the same program with AddressSanitizer and UBSan, stand-alone: the same output as the plain build"""
    plain = program("fft_balance_check")
    san = program("fft_balance_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _lines(san) == _lines(plain)
