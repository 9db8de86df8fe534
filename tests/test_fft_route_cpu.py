"""Which kernels an FFT plan runs for a batch (opencl_fft_amd/csrc/fft_route.hpp) on the CPU: a g++-built program prints
fft_route() for every shape and batch of a grid around the thresholds, and this file holds the table it has to match,
written out on its own.  The kernel names are the strings tests/test_gpu_fft_impulses.py asserts on the device."""
import os
import subprocess

import pytest

from tests import test_gpu_fft_impulses as impulses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "fft_route.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace clfa;

static const char *kNames[] = {"Lds", "Cfft2x13", "Rfft2x13", "Rfft2x14", "FourStepSpread", "FourStep", "Res16", "RealRes16",
                               "Big", "BlueLds", "Bluestein"};

static void line(const FftShape &s, long batch) {
  const FftRoute r = fft_route(s, batch);
  printf("%d %d %d %d %d %ld %s %s %d %d %u\n", s.num_cus, s.n, (int)s.real, (int)s.fwd, s.blue_m, batch, kNames[(int)r],
         route_kernel_name(r, s), (int)route_one_touch(r, s.real), (int)(s.real && route_pack_apart(r)), fft_routes(s) >> (int)r & 1);
}

int main(int argc, char **argv) {
  if (argc > 1) {   // real n pairs: the name a plan reports (a batch above every threshold)
    for (int i = 1; i + 1 < argc; i += 2) {
      const FftShape s = fft_shape(atoi(argv[i]) != 0, true, atoi(argv[i + 1]), 256);
      printf("%s\n", route_kernel_name(fft_route_many(s), s));
    }
    return 0;
  }
  for (int cus : {1, 7, 8, 64, 256, 304})
    for (int real = 0; real < 2; real++)
      for (int fwd = 0; fwd < 2; fwd++) {
        const long batches[] = {1, 2, 3, cus / 8, cus / 8 + 1, cus / 4, cus / 4 + 1, 70, 65535, 65536, 1000000};
        for (long batch : batches) {
          if (batch < 1) continue;
          for (int logn = 1; logn <= 24; logn++) line(fft_shape(real, fwd, 1 << logn, cus), batch);
          for (int n : {3, 100, 127, 129, 4095, 4097, 44100}) line(fft_shape(real, fwd, n, cus), batch);
        }
      }
  return 0;
}
"""


def expected(cus, n, real, blue_m, batch):
    """(route, real pack / unpack as a pass of its own) by the table of the plans' rules, first match"""
    if blue_m:
        return ("BlueLds" if 256 <= blue_m <= 8192 else "Bluestein"), real
    logn = n.bit_length() - 1
    if logn <= 13:
        return "Lds", False
    if logn > 16:
        return "Big", real
    if not real and logn == 14 and batch * 4 > cus:
        return "Cfft2x13", False
    if real and logn in (14, 15) and batch > cus // 8:
        return ("Rfft2x13" if logn == 14 else "Rfft2x14"), False
    if real and logn == 16 and batch * 4 > cus:
        return "RealRes16", False
    # complex 2^14..2^16 left over, and the packed real sizes below their thresholds: unpack / pack around it
    if batch * 4 <= cus and batch <= 65535:
        return "FourStepSpread", real
    return ("Res16" if logn == 16 else "FourStep"), real


NAMES = {"Cfft2x13": "k_cfft_2x", "Rfft2x13": "k_rfft_2x", "Rfft2x14": "k_rfft_2x", "FourStepSpread": "k_fft_4step_cols",
         "FourStep": "k_fft_4step", "Res16": "k_fft_res16", "RealRes16": "k_fft_res16", "BlueLds": "k_blue_lds",
         "Bluestein": "bluestein"}


def expected_name(route, n, real):
    if route == "Lds":
        logn = n.bit_length() - 1
        if not real and logn <= 2:
            return "k_fft_tiny"
        return "k_fft_small" if 2 <= logn <= (8 if real else 6) else "k_fft_lds"
    if route == "Big":
        return "k_big2_cols" if n <= 1 << 22 else "k_big_cols"
    return NAMES[route]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("fft_route")
    src = d / "fft_route_check.cpp"
    src.write_text(PROGRAM)

    def build(name, *flags):
        exe = str(d / name)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"),
                               str(src), "-o", exe])
        return exe
    return build


def _lines(exe, *args):
    p = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out
    return out.strip().split("\n")


def test_every_route_of_the_grid_matches_the_table(program):
    """every (CU count, length, kind, direction, batch) of the grid: the route, its kernel name, whether a pinned array may
    run on it zero-copy and whether the real pack is a pass of its own; each route is reached; fft_routes() lists it"""
    seen, bad = set(), []
    lines = _lines(program("fft_route_check"))
    for ln in lines:
        cus, n, real, fwd, blue_m, batch, route, name, one_touch, apart, listed = ln.split()
        cus, n, real, blue_m, batch = int(cus), int(n), real == "1", int(blue_m), int(batch)
        assert (blue_m != 0) == (n & (n - 1) != 0) and (not blue_m or blue_m // 2 < 2 * n - 1 <= blue_m), ln
        want, want_apart = expected(cus, n, real, blue_m, batch)
        # zero-copy on a pinned array: every route of the reference's range (powers of two to 65536) except the launch
        # chains with a pack / unpack pass of their own
        want_touch = not blue_m and n <= 65536 and not want_apart
        if (route, name, one_touch == "1", apart == "1", listed) != (want, expected_name(want, n, real), want_touch, want_apart, "1"):
            bad.append((ln, want))
        seen.add(route)
    assert not bad, bad[:10]
    assert len(lines) > 6 * 4 * 9 * 31 and seen == set(NAMES) | {"Lds", "Big"}, seen


def test_kernel_names_are_the_ones_the_device_tests_expect(program):
    """the name a plan reports, for every case of tests/test_gpu_fft_impulses.py that asserts one"""
    cases = [(real, n, kernel) for real, n, _, kernel in impulses.ROUTES if kernel]
    cases += [(False, n, route) for route, n, _, _ in impulses.C2C if route != "spread"] + [(False, 65536, "k_fft_res16")]
    cases += [(True, n, route) for route, n, _, _ in impulses.REAL if route in ("k_rfft_2x", "k_fft_res16", "k_blue_lds", "k_big2_cols")]
    cases += [(False, n, "k_blue_lds" if n in (100, 1000, 4095) else "bluestein") for n in (3, 100, 1000, 4095, 44100)]
    args = [str(v) for real, n, _ in cases for v in (int(real), n // 2 if real else n)]
    got = _lines(program("fft_route_check"), *args)
    assert got == [kernel for _, _, kernel in cases] and len(got) > 40


def test_route_program_under_sanitizers(program):
    """the same program with AddressSanitizer and UBSan, stand-alone: the same output as the plain build"""
    plain = program("fft_route_check")
    san = program("fft_route_check_san", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _lines(san) == _lines(plain)
