"""The analysis of a stored signal at given time points (clfa_pvoc_tanal*, Pvoc.tanal*) without a device: the exported
symbols, the Python surface and the order of its checks, stretch_starts, and facts of the numpy model
(tests/pvoc_tanal_model.py) the device test leans on.

CAPS_TANAL (tests/pvoc_tanal_model.py) caps what the float32 yardstick alone reaches on the impulse probe, so that a probe
which inflated the device test's bound would fail here.  By the project's rule a cap is the next power of two above the
worst value measured on the CPU.  MEASURED here over the nine sizes, the hops size / 4, 3 and size / 4 + 1, two rows each,
in the units of pvoc_tanal_model.probe_errors:
  amp   3.10 .. 7.11 (the largest at size 16384, hop 4096; 2^-24 of the frame's largest amp: the reference's float32
        radix-2 transform of an impulse, log2(size) roundings deep)                 -> cap 8
  dev   0.00 .. 0.71 (the largest at size 8192, hop 3)                              -> cap 1
"""
import ctypes

import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from opencl_fft_amd._base import CL_INVALID_VALUE
from tests import pvoc_model as pm
from tests import pvoc_probe as pp
from tests import pvoc_tanal_model as tm
from tests import stft_model
from tests.pvoc_inputs import hann, two_tones

SR = 48000.0
f32 = np.float32
NAMES = ("clfa_pvoc_tanal_dev", "clfa_pvoc_tanal", "clfa_pvoc_tanal_kernel_name")


def test_library_exports_the_tanal_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in NAMES:
        assert hasattr(L, n) and n in bound, n
    assert fa.Pvoc(0, 48, 16, SR).tanal_kernel_name() == ""
    pv = fa.Pvoc(0, 64, 16, SR, 2)
    assert pv.tanal_kernel_name() == ("k_pvoc_tanal" if pv.get_error() == 0 else "")
    assert _lib.lib().clfa_pvoc_tanal_kernel_name(None) == b""
    for m in ("tanal", "tanal_device", "tanal_kernel_name", "stretch_starts"):
        assert callable(getattr(pv, m))


def test_argument_errors_come_before_the_device_lookup():
    """an object created on device 99: a bad argument is CLFA_INVALID_VALUE, a good call the object's error"""
    size, hop, C, Fout = 64, 16, 2, 5
    n, stride = 3 * size + 5, 3 * size + 8
    none = fa.Pvoc(99, size, hop, SR, C)
    good = none.get_error()
    assert good != 0 and none.tanal_kernel_name() == ""
    L = _lib.lib()
    sig = np.zeros(C * stride, f32)
    win, starts = hann(size), np.arange(Fout, dtype=np.int32)
    out = np.zeros((C, Fout, size // 2 + 1, 2), f32)
    assert out.ctypes.data % 8 == 0
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)

    def host(x=sig, st=stride, n=n, w=win, s=starts, o=out, F=Fout, h=none._h):
        return L.clfa_pvoc_tanal(h, ptr(x), st, n, ptr(w), ptr(s), ptr(o), F)

    def devf(x=sig, st=stride, n=n, w=win, s=starts, o=out, F=Fout, h=none._h):
        return L.clfa_pvoc_tanal_dev(h, ptr(x), st, n, ptr(w), ptr(s), ptr(o), F, None)

    for f in (host, devf):
        assert f() == good and f(st=n) == good and f(n=1, st=1) == good
        assert f(F=0) == good and f(F=0, x=None, w=None, s=None, o=None) == good
        assert f(F=-1) == CL_INVALID_VALUE and f(h=None) == CL_INVALID_VALUE
        for kw in (dict(x=None), dict(w=None), dict(s=None), dict(o=None), dict(n=0), dict(n=-1), dict(n=2 ** 31),
                   dict(st=n - 1), dict(st=0)):
            assert f(**kw) == CL_INVALID_VALUE, kw
        # the output over the window, over starts, and inside the signal's strided extent: the pad behind row 0
        assert f(o=ptr(win)) == CL_INVALID_VALUE and f(o=ptr(starts)) == CL_INVALID_VALUE
        assert sig.ctypes.data % 8 == 0 and f(o=ptr(sig) + 4 * (n + 1)) == CL_INVALID_VALUE
        one = np.zeros(8 + out.size, f32)
        assert f(x=one, n=4, st=4, o=ptr(one) + 32) == good                          # the output right behind the signal
        assert f(x=one, n=4, st=4, o=ptr(one) + 24) == CL_INVALID_VALUE              # ... and one pair into it
    # what only a device form can object to: misaligned pointers
    assert devf(x=ptr(sig) + 2) == CL_INVALID_VALUE and devf(w=ptr(win) + 1) == CL_INVALID_VALUE
    assert devf(s=ptr(starts) + 2) == CL_INVALID_VALUE and devf(o=ptr(out) + 4) == CL_INVALID_VALUE
    assert devf(x=ptr(sig) + 4, st=stride - 1) == good
    bad = fa.Pvoc(0, 48, 16, SR)                # bad creation arguments: that error, whatever the call's arguments
    assert L.clfa_pvoc_tanal(bad._h, None, 0, 0, None, None, None, -1) == bad.get_error() == CL_INVALID_VALUE


def test_the_python_surface_without_a_device():
    size, hop, C, Fout, n = 64, 16, 2, 4, 200
    M = size // 2
    PV, PV1 = fa.Pvoc(99, size, hop, SR, C), fa.Pvoc(99, size, hop, SR, 1)
    NO_DEVICE = PV.get_error()
    assert NO_DEVICE != 0
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    sig, win, st, out = z(C, n), z(size), z(Fout, dt=torch.int32), z(C, Fout, M + 1, 2)
    cases = [
        ("good", lambda: PV.tanal_device(sig, win, st, out, stream=0), NO_DEVICE),
        ("a row stride", lambda: PV.tanal_device(z(C, n + 3)[:, :n], win, st, out, stream=0), NO_DEVICE),
        ("one channel, no axis", lambda: PV1.tanal_device(z(n), win, st, z(Fout, M + 1, 2), stream=0), NO_DEVICE),
        ("no frames", lambda: PV.tanal_device(sig, win, z(0, dt=torch.int32), z(C, 0, M + 1, 2), stream=0), NO_DEVICE),
        ("signal float64", lambda: PV.tanal_device(z(C, n, dt=torch.float64), win, st, out, stream=0), CL_INVALID_VALUE),
        ("signal of other channels", lambda: PV.tanal_device(z(C + 1, n), win, st, out, stream=0), CL_INVALID_VALUE),
        ("signal without an axis", lambda: PV.tanal_device(z(n), win, st, out, stream=0), CL_INVALID_VALUE),
        ("signal with an inner stride", lambda: PV.tanal_device(z(C, 2 * n)[:, ::2], win, st, out, stream=0), CL_INVALID_VALUE),
        ("signal rows that overlap", lambda: PV.tanal_device(z(n + 1).as_strided((C, n), (1, 1)), win, st, out, stream=0),
         CL_INVALID_VALUE),
        ("empty signal", lambda: PV.tanal_device(z(C, 0), win, st, out, stream=0), CL_INVALID_VALUE),
        ("window of another size", lambda: PV.tanal_device(sig, z(size + 1), st, out, stream=0), CL_INVALID_VALUE),
        ("window float64", lambda: PV.tanal_device(sig, z(size, dt=torch.float64), st, out, stream=0), CL_INVALID_VALUE),
        ("window strided", lambda: PV.tanal_device(sig, z(2 * size)[::2], st, out, stream=0), CL_INVALID_VALUE),
        ("no window", lambda: PV.tanal_device(sig, None, st, out, stream=0), CL_INVALID_VALUE),
        ("starts int64", lambda: PV.tanal_device(sig, win, z(Fout, dt=torch.int64), out, stream=0), CL_INVALID_VALUE),
        ("starts float32", lambda: PV.tanal_device(sig, win, z(Fout), out, stream=0), CL_INVALID_VALUE),
        ("starts of another count", lambda: PV.tanal_device(sig, win, z(Fout + 1, dt=torch.int32), out, stream=0), CL_INVALID_VALUE),
        ("frames float64", lambda: PV.tanal_device(sig, win, st, z(C, Fout, M + 1, 2, dt=torch.float64), stream=0), CL_INVALID_VALUE),
        ("frames of M bins", lambda: PV.tanal_device(sig, win, st, z(C, Fout, M, 2), stream=0), CL_INVALID_VALUE),
        ("frames strided", lambda: PV.tanal_device(sig, win, st, z(C, Fout, M + 1, 4)[..., ::2], stream=0), CL_INVALID_VALUE),
    ]
    for name, call, want in cases:
        assert call() == want, name
    # the host form: shapes are ValueErrors, a good call raises the object's error
    with pytest.raises(fa.ClError):
        PV.tanal(np.zeros((C, n), f32), hann(size), [0, 5])
    for bad in (lambda: PV.tanal(np.zeros((C + 1, n), f32), hann(size), [0]), lambda: PV.tanal(np.zeros(n, f32), hann(size), [0]),
                lambda: PV.tanal(np.zeros((C, n), f32), hann(size + 2), [0]), lambda: PV.tanal(np.zeros((C, 0), f32), hann(size), [0])):
        with pytest.raises(ValueError):
            bad()


def test_stretch_starts():
    s = fa.Pvoc.stretch_starts(1000, 16, 2.0)
    assert s.dtype == np.int32 and s.size == 125 and np.array_equal(s, np.arange(125) * 8)
    s = fa.Pvoc.stretch_starts(1000, 16, 1.0)
    assert s.size == 63 and np.array_equal(s, np.arange(63) * 16)
    s = fa.Pvoc.stretch_starts(100, 7, 0.3)
    g = np.arange(int(np.ceil(0.3 * 100 / 7)), dtype=np.float64)
    assert s.size == 5 and np.array_equal(s, np.floor(g * 7 / 0.3).astype(np.int32))
    assert np.array_equal(fa.Pvoc.stretch_starts(48, 16, 3)[:7], [0, 5, 10, 16, 21, 26, 32])
    assert fa.Pvoc.stretch_starts(0, 16, 2.0).size == 0
    for bad in (0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            fa.Pvoc.stretch_starts(1000, 16, bad)


def test_slices_pad_with_zeros_and_keep_the_dtype():
    x = np.arange(1, 21, dtype=np.float64).reshape(2, 10)
    sl = tm.slices(x, [-9, 0, 3, 8, 40], 4, 2)
    assert sl.dtype == np.float64 and sl.shape == (2, 5, 6)
    assert not sl[:, 0].any() and not sl[:, 4].any()
    assert np.array_equal(sl[0, 1], [0, 0, 1, 2, 3, 4]) and np.array_equal(sl[1, 2], [12, 13, 14, 15, 16, 17])
    assert np.array_equal(sl[0, 3], [7, 8, 9, 10, 0, 0])
    assert tm.slices(x.astype(f32), [1], 4, 2).dtype == f32


@pytest.mark.parametrize("size, hop", [(64, 16), (256, 3), (1024, 257)])
def test_on_the_hop_grid_the_truth_is_the_stft_route(size, hop):
    """starts = g hop: for g >= 1 tanal64 is analyze64's formula on the float64 STFT of the whole signal"""
    C, F = 2, 9
    x = two_tones(size, hop, C, F, 11).astype(f32)
    w = hann(size)
    amp, dev, freq = tm.tanal64(x, w, np.arange(F) * hop, size, hop, SR)
    P = tm.pack64(stft_model.windowed_frames_f32(x, size, hop, w))
    a2, d2, f2 = tm.pair64(P[:, :-1], P[:, 1:], size, hop, SR)
    assert np.array_equal(amp[:, 1:], a2) and np.array_equal(dev[:, 1:], d2) and np.array_equal(freq[:, 1:], f2)
    # ... and analyze64 itself, which rounds the spectra to complex64 first, agrees to that rounding
    a3, _, _, _ = pm.analyze64(P.astype(np.complex64), pm.initial_prev(C, size), size, hop, SR)
    assert np.allclose(a3[:, 1:], a2, rtol=2.0 ** -22, atol=0)


def test_a_stretched_cosine_keeps_its_frequency():
    """a stationary cosine stretched by 3 under a Hann window: the peak bin of every interior frame reports its frequency"""
    size, hop, n = 1024, 256, 16384
    f0 = 37.3 * SR / size
    x = np.cos(2 * np.pi * f0 / SR * np.arange(n))[None, :].astype(f32)
    starts = fa.Pvoc.stretch_starts(n, hop, 3.0)
    amp, _, freq = tm.tanal64(x, hann(size), starts, size, hop, SR)
    inner = (starts >= hop) & (starts + size <= n)
    assert inner.sum() > 100
    peak = amp[0, inner].argmax(axis=-1)
    assert np.all(peak == 37)
    assert np.abs(freq[0, inner, 37] - f0).max() < 1e-3 * SR / size


CASES = [(size, hop) for size in pp.SIZES for hop in (size // 4, 3, size // 4 + 1)]


@pytest.mark.parametrize("size, hop", CASES)
def test_the_yardstick_stays_under_its_caps_on_the_probe(size, hop):
    """tanal32 against the analytic truth on the impulse probe, in the units of the device test's bound"""
    n, w = tm.samples_of(size), tm.int_window(size)
    starts = tm.starts_for(size, hop, tm.fout_for(size))
    worst = {"amp": 0.0, "dev": 0.0}
    for seed in (0, 2):
        row, pos, amps = tm.impulse_row(size, hop, n, seed)
        amp64, dev64, freq64, kind = tm.impulse_truth(size, hop, SR, w, pos, amps, starts)
        assert (kind == tm.BOTH).sum() >= 3, "the probe needs frames with the impulse in both windows"
        # the closed form is the transform of the windowed slices
        a64, d64, _ = tm.tanal64(row[None, :], w, starts, size, hop, SR)
        assert np.allclose(a64[0], amp64, rtol=1e-9, atol=1e-12)
        fr = tm.tanal32(row[None, :], w, starts, size, hop, SR)[0]
        e = tm.probe_errors(fr, amp64, dev64, kind, size, hop, SR)
        for q in worst:
            worst[q] = max(worst[q], e[q][0])
        # the frames without an impulse in both windows: silent where B is empty, the bin centre to the bit everywhere
        quiet = kind != tm.BOTH
        assert np.array_equal(fr[quiet][..., 1].view(np.uint32), np.broadcast_to(tm.centre(size, SR), fr[quiet][..., 1].shape).view(np.uint32))
        assert not fr[(kind == tm.NEITHER) | (kind == tm.A_ONLY)][..., 0].view(np.uint32).any()
    print("PVOCTANAL yardstick size %d hop %d: amp %.2f dev %.2f" % (size, hop, worst["amp"], worst["dev"]))
    for q in worst:
        assert worst[q] <= tm.CAPS_TANAL[q], "%s %.2f" % (q, worst[q])
