"""The filter bank of clfa_pvoc without a device: the numpy model (tests/pvoc_bank_model.py) against its float64 version
within a derived bound, the mutants the device test must notice, the mel bank helper, the setup's plain-C++ part
(opencl_fft_amd/csrc/bank_plan.hpp, built with g++), and the argument rules on an object that found no device.

The bounds.  A band: TERM rounds the product (and the square, with POWER), a lane adds ceil(count / 16) - 1 times, the
tree four times: at most ceil(count / 16) + 6 roundings on any path, so |E32 - E64| <= gamma_n sum |t64| with
n = ceil(count / 16) + 6, gamma_n = n u / (1 - n u), u = 2^-24.  A coefficient: one rounding of the product and B
additions, n = B + 2 over sum |D v|.

The mutants, counted here on the 40-band mel bank at size 512, amps 10^U(-3, 3), 36 frames (36 x 40 = 1440 band sums):
serial differs in 500, halving in 440, w32 in 149, fma in 29, and dct_descending in 379 of the 36 x 13 = 468 coefficients.
On the device test's own frames, over the four banks of a size together (18 x 314 = 5652 band sums): at size 64 serial 2345,
halving 2415, w32 1083, fma 192; at size 512 serial 3446, halving 2911, w32 2437, fma 929.
test_every_mutant_is_noticed asserts > 0 for each and prints the counts (pytest -s): a change of the inputs that
weakens them shows against these."""
import os
import subprocess

import numpy as np
import pytest

import opencl_fft_amd as fa
from tests import pvoc_bank_model as bm

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, INVALID_OPERATION = -30, -59
SIZES = (64, 512, 16384)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def differ(a, b):
    """how many values differ, a NaN in both places being equal"""
    return int(((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))).sum())


@pytest.mark.parametrize("power", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_float32_model_within_the_bound_of_the_float64_one(size, power):
    plain, _ = bm.frames(size)
    amps = plain[..., 0]
    for name, bank in bm.banks(size).items():
        E32 = bm.bands32(amps, bank, power)
        E64, A = bm.bands64(amps, bank, power)
        n = -(-bank.count // 16) + 6
        assert (np.abs(E32 - E64) <= bm.gamma(n) * A).all(), (size, name)
        D = bm.dct_table(bank.B).astype(f32)
        for v in (E32, bm.log32(E32, 1e-10)):
            C64, AD = bm.dct64(v, D, bank.B)
            assert (np.abs(bm.dct32(v, D, bank.B) - C64) <= bm.gamma(bank.B + 2) * AD).all(), (size, name)


def test_every_mutant_is_noticed():
    bank = bm.mel(512)
    rng = np.random.default_rng(5)
    amps = (10.0 ** rng.uniform(-3, 3, (36, 257))).astype(f32)
    want = bm.bands32(amps, bank)
    D = bm.dct_table(bank.B).astype(f32)
    for m in ("serial", "halving", "w32", "fma"):
        n = differ(bm.bands32(amps, bank, mutant=m), want)
        print("PVOCBANK mutant %s: %d of %d band sums differ" % (m, n, want.size))
        assert n > 0, m
    n = differ(bm.dct32(want, D, 13, "dct_descending"), bm.dct32(want, D, 13))
    print("PVOCBANK mutant dct_descending: %d of %d coefficients differ" % (n, 36 * 13))
    assert n > 0
    # and on the device test's own inputs, each mutant at the stage it touches: the sums over the four banks of a size
    # together (the mel bands at size 64 have at most 5 bins, where every order gives one sum; the other banks notice),
    # the DCT and the NaN rule on every bank
    for size in (64, 512):
        plain, odd = bm.frames(size)
        banks = bm.banks(size)
        for m in ("serial", "halving", "w32", "fma"):
            n = sum(differ(bm.bands32(plain[..., 0], bank, True, m), bm.bands32(plain[..., 0], bank, True)) for bank in banks.values())
            print("PVOCBANK size %d mutant %s: %d band sums differ" % (size, m, n))
            assert n > 0, (size, m)
        for name, bank in banks.items():
            E = bm.bands32(odd[..., 0], bank, True)
            assert np.isnan(E).any() and differ(bm.log32(E, 1e-10, "nan_no_floor"), bm.log32(E, 1e-10)) > 0, (size, name)
            if bank.B > 1:
                D, v = bm.dct_table(bank.B).astype(f32), bm.log32(bm.bands32(plain[..., 0], bank, True), 1e-10)
                assert differ(bm.dct32(v, D, min(13, bank.B), "dct_descending"), bm.dct32(v, D, min(13, bank.B))) > 0, (size, name)


@pytest.mark.parametrize("size, empty", [(64, 12), (512, 0), (16384, 0)])
def test_mel_bank(size, empty):
    M, B = size // 2, 40
    first, count, weights = fa.Pvoc.mel_bank(size, bm.SR, B)
    assert weights.dtype == f32 and bm.valid(M, first, count, weights)
    bank = bm.Bank(first, count, weights)
    dense = np.zeros((B, M + 1))
    for b in range(B):
        w = bank.w(b)
        dense[b, first[b]:first[b] + count[b]] = w
        if w.any():
            assert w[0] != 0 and w[-1] != 0, "trimmed"
            k = int(np.argmax(w))
            assert (np.diff(w[:k + 1]) >= 0).all() and (np.diff(w[k:]) <= 0).all(), "rises, then falls"
        else:
            assert count[b] == 1
    assert sum(not bank.w(b).any() for b in range(B)) == empty
    # neighbouring triangles sum to 1 between the first and the last centre
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    edges = 700.0 * (10.0 ** (np.linspace(mel(0.0), mel(bm.SR / 2), B + 2) / 2595.0) - 1.0)
    f = np.arange(M + 1) * bm.SR / size
    inside = (f >= edges[1]) & (f <= edges[B])
    assert inside.any() and np.allclose(dense.sum(axis=0)[inside], 1.0, atol=1e-6)
    if size == 16384:
        assert (count.min(), count.max()) == (45, 1345)


PLAN_MAIN = r"""
#include "bank_plan.hpp"
#include <cstdio>
using namespace clfa;
int main() {
  const int M = 32;
  int first[20], count[20];
  float w[20 * 33];
  for (int i = 0; i < 20 * 33; i++) w[i] = 0.5f;
  for (int b = 0; b < 20; b++) { first[b] = b % 3; count[b] = 1 + (b * 7) % 30; }
  int ok = bank_ok(M, 20, first, count, w);
  int bad = 0;
  bad += bank_ok(M, 0, first, count, w) + bank_ok(M, 257, first, count, w) + bank_ok(M, 20, nullptr, count, w);
  count[3] = 0; bad += bank_ok(M, 20, first, count, w); count[3] = 22;
  first[4] = -1; bad += bank_ok(M, 20, first, count, w); first[4] = 1;
  first[5] = 30; count[5] = 4; bad += bank_ok(M, 20, first, count, w); count[5] = 3; ok += bank_ok(M, 20, first, count, w);
  w[7] = INFINITY; bad += bank_ok(M, 20, first, count, w); w[7] = NAN; bad += bank_ok(M, 20, first, count, w); w[7] = -2.f;
  printf("%d %d\n", ok, bad);
  std::vector<int> s = bank_schedule(20, count);
  for (int v : s) printf("%d ", v);
  printf("\n");
  std::vector<BankBand> v = bank_bands(20, first, count);
  for (const BankBand &b : v) printf("%d ", b.woff);
  printf("\n");
  std::vector<float> D = bank_dct(5);
  for (float d : D) printf("%.9g ", d);
  printf("\n");
  return 0;
}
"""


def test_bank_plan_header(tmp_path):
    """bank_plan.hpp with g++: the validation's rules, a schedule that holds every band once with the longest bands at the
    head of the rows, the weights' offsets, the DCT table"""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(src), "-o", str(exe)])
    verdicts, sched, woff, dct = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    assert verdicts.split() == ["2", "0"]
    count = np.array([1 + (b * 7) % 30 for b in range(20)])
    count[3], count[5] = 22, 3
    s = [int(x) for x in sched.split()]
    starts, order = s[:17], s[17:]
    assert starts[0] == 0 and starts[16] == 20 and all(a <= b for a, b in zip(starts, starts[1:]))
    assert sorted(order) == list(range(20))
    heads = [order[starts[r]] for r in range(16)]
    assert sorted(count[heads]) == sorted(np.sort(count)[-16:]), "the sixteen longest bands lead the rows"
    for r in range(16):
        c = count[order[starts[r]:starts[r + 1]]]
        assert (np.diff(c) <= 0).all()
    steps = [-(-count[order[starts[r]:starts[r + 1]]] // 16).sum() for r in range(16)]
    assert max(steps) - min(steps) <= 2
    assert [int(x) for x in woff.split()] == list(np.concatenate([[0], np.cumsum(count)[:-1]]))
    D = np.array([float(x) for x in dct.split()], f32).reshape(5, 5)
    assert np.abs(D - bm.dct_table(5)).max() <= 2.0 ** -24 and np.allclose(D @ D.T, np.eye(5), atol=5 * 2.0 ** -23)


def test_argument_rules_without_a_device():
    """one row per rule of the header: an invalid value before an invalid operation before the object's error"""
    if fa.device_count() > 0:
        pytest.skip("a HIP device is present: tests/test_gpu_pvoc_bank.py makes these checks on device memory")
    import torch
    size, C, F = 64, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, 16, bm.SR, C)
    err = pv.get_error()
    assert err == -1 and pv.bands_kernel_name() == "" and pv.bank_bands() == -1 and pv.bank_state_bytes() == 0
    first, count, weights = fa.Pvoc.mel_bank(size, bm.SR, 40)
    # the setup: what is wrong is an invalid value, what is right the object's error
    assert pv.bank_setup(first, count, weights) == err
    bad = [([0] * 257, [1] * 257, [1.0] * 257), ([], [], []), ([M + 1], [1], [1.0]), ([M], [2], [1.0, 1.0]),
           ([-1], [1], [1.0]), ([0], [0], []), ([0], [1], [np.inf]), ([0], [2], [1.0, np.nan]), ([0], [2], [1.0]),
           ([0, 1], [1], [1.0])]
    for f, c, w in bad:
        assert pv.bank_setup(f, c, w) == INVALID, (f[:3], c[:3])
    assert pv.bank_bands() == -1
    with pytest.raises(fa.ClError) as e:
        pv.bank_dct()
    assert e.value.code == err
    fr, out = torch.zeros((C, F, M + 1, 2)), torch.zeros((C, F, 5))
    call = lambda **kw: pv.bands_device(fr, out, stream=0, **kw)
    # a good call before the setup: an invalid operation, ahead of the object's error
    assert call() == INVALID_OPERATION and call(power=True, log=True, ncoef=5) == INVALID_OPERATION
    # bad arguments: invalid values, ahead of that
    assert call(log=True, floor=0.0) == INVALID and call(log=True, floor=-1.0) == INVALID
    assert call(log=True, floor=float("nan")) == INVALID and call(log=True, floor=float("inf")) == INVALID
    assert call(floor=-1.0) == INVALID_OPERATION, "the floor is not looked at without LOG"
    assert call(ncoef=-1) == INVALID and call(ncoef=257) == INVALID
    lib = fa.lib()
    raw = lambda flags, ncoef, F=F, o=out: lib.clfa_pvoc_bands_dev(pv._h, fr.data_ptr(), o.data_ptr(), F, flags, ncoef, 1e-10, 0)
    assert raw(8, 0) == INVALID and raw(0, 3) == INVALID and raw(4, 0) == INVALID and raw(-1, 0) == INVALID
    assert raw(0, 0, F=-1) == INVALID and raw(0, 0, F=0) == err, "F == 0 is a good call, before the setup too"
    assert lib.clfa_pvoc_bands_dev(pv._h, fr.data_ptr(), None, F, 0, 0, 1e-10, 0) == INVALID
    assert lib.clfa_pvoc_bands_dev(pv._h, None, out.data_ptr(), F, 0, 0, 1e-10, 0) == INVALID
    assert lib.clfa_pvoc_bands_dev(None, fr.data_ptr(), out.data_ptr(), F, 0, 0, 1e-10, 0) == INVALID
    # an out that overlaps the frames, even by one float
    flat = fr.view(-1)
    assert lib.clfa_pvoc_bands_dev(pv._h, fr.data_ptr(), flat[flat.numel() - 1:].data_ptr(), F, 0, 0, 1e-10, 0) == INVALID
    # the Python layer's own refusals
    assert pv.bands_device(fr, torch.zeros((C, F + 1, 5)), stream=0) == INVALID
    assert pv.bands_device(fr, torch.zeros((C, F, 5), dtype=torch.float64), stream=0) == INVALID
    assert pv.bands_device(fr, torch.zeros((C, F, 5)), ncoef=4, stream=0) == INVALID
    assert pv.bands_device(fr[:, :, :M].contiguous(), out, stream=0) == INVALID
    # the blocking form
    x = np.zeros((C, F, M + 1, 2), f32)
    for kw, code in (({}, INVALID_OPERATION), ({"log": True, "floor": 0.0}, INVALID), ({"ncoef": 300}, INVALID)):
        with pytest.raises(fa.ClError) as e:
            pv.bands(x, **kw)
        assert e.value.code == code, kw
    assert lib.clfa_pvoc_bank_bands(None) == -1 and lib.clfa_pvoc_bank_state_bytes(None) == 0
    assert lib.clfa_pvoc_bank_read_dct(pv._h, None) == INVALID and lib.clfa_pvoc_bank_setup(None, 1, None, None, None) == INVALID
