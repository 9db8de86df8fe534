"""The pitch of clfa_pvoc without a GPU: planted frames that pin the definition and tell the numpy model
(tests/pvoc_pitch_model.py) from seven mutants of it, the accuracy of the method on harmonic tones as a condition on the
model, the library's new symbols and device-free argument checks — which answer on a machine without a device too — and
the kernel's own score and peak test (opencl_fft_amd/csrc/pvoc_pitch_score.hpp) built with g++ against the model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_model as pm
from tests import pvoc_pitch_model as pt
from tests import stft_model as sm
from tests.pvoc_inputs import SR, hann, raw_freq_first

CL_INVALID_VALUE = -30
f32 = np.float32
GPU_SIZES = (64, 128, 256, 512, 2048, 16384)


@pytest.fixture(autouse=True, scope="module")
def the_library_has_the_feature():
    """the model and the planted cases are the yardstick of clfa_pvoc_pitch*: without those entry points in the library
    and in the Python layer no test of this file says anything, and every one fails"""
    missing = [n for n in ("clfa_pvoc_pitch_dev", "clfa_pvoc_pitch", "clfa_pvoc_pitch_kernel_name")
               if not hasattr(ctypes.CDLL(_lib.LIB_PATH), n)]
    assert not missing and all(hasattr(fa.Pvoc, m) for m in ("pitch", "pitch_device", "pitch_kernel_name")), missing


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differs(good, bad):
    """the rows or the lists differ, a NaN in the same place counting as equal bits"""
    return any(np.any((bits(g) != bits(b)) & ~(np.isnan(g) & np.isnan(b))) for g, b in zip(good, bad))


def cases_by_name(size, C=2, F=3):
    return {name: (x, args) for name, x, args in pt.planted(size, C, F)}


# ---- 1. the planted cases ----

@pytest.mark.parametrize("size", (64, 256, 2048))
def test_the_planted_cases_give_what_the_definition_says(size):
    C, F = 2, 3
    cases = cases_by_name(size, C, F)

    def run(name):
        x, args = cases[name]
        return pt.pitch(x, **args)

    rows, lst = run("plateau")
    assert np.all(rows[..., pt.NPEAKS] == 2)
    assert np.all(lst[..., 0, :] == (1.0, 300.0)) and np.all(lst[..., 1, :] == (0.5, 600.0)) and not lst[..., 2:, :].any()
    assert np.all(rows[..., pt.F0] == 300.0) and np.all(rows[..., pt.SAL] == f32(1.0) + f32(0.5) * f32(f32(0.84)))
    rows, lst = run("NaN amps")
    assert np.all(rows[..., pt.NPEAKS] == 2) and np.all(lst[..., 0, :] == (0.25, 440.0)) and np.all(lst[..., 1, :] == (0.125, 880.0))
    assert np.all(rows[..., pt.F0] == 440.0) and np.all(rows[..., pt.CONF] == (f32(0.25) + f32(0.125) * f32(0.84)) / f32(0.375))
    rows, lst = run("bad freqs")
    assert np.all(rows[..., pt.NPEAKS] == 2) and np.all(lst[..., 0, :] == (0.5, 220.0)) and np.all(lst[..., 1, :] == (0.25, 441.0))
    rows, lst = run("louder outside")
    assert np.all(rows[..., pt.NPEAKS] == 1) and np.all(lst[..., 0, 0] == 0.5) and np.all(rows[..., pt.F0] == lst[..., 0, 1])
    rows, lst = run("more peaks than npeaks")
    assert np.all(rows[..., pt.NPEAKS] == 5) and np.all(lst[..., 0] == np.arange(1, 6)) and lst.shape[2] == 5
    assert np.all(rows[..., pt.F0] == 110.0)
    rows, lst = run("as many peaks as npeaks")
    assert np.all(rows[..., pt.NPEAKS] == 12) and np.all(lst[..., 0] == np.arange(1, 13))
    rows, lst = run("no peak")
    assert not bits(rows).any() and not bits(lst).any()
    rows, lst = run("no candidate")
    assert np.all(rows[..., pt.NPEAKS] == 2) and not bits(rows[..., :3]).any() and np.all(lst[..., 1, :] == (0.5, 4000.0))
    rows, lst = run("equal scores")
    assert np.all(rows[..., pt.F0] == 200.0) and np.all(rows[..., pt.CONF] == 1.0)
    rows, lst = run("decay")
    assert np.all(rows[..., pt.F0] == 200.0) and np.all(rows[..., pt.CONF] < 1.0)
    rows, lst = run("deviation over h")
    assert np.all(rows[..., pt.F0] == 100.0) and np.all(rows[..., pt.SAL] == f32(1.0) + f32(0.5) * pt.weights(0.84)[2])
    rows, lst = run("deviation equal to tol")
    assert np.all(rows[..., pt.F0] == 128.0) and np.all(rows[..., pt.SAL] == 1.5)
    rows, lst = run("order of the sum")
    assert np.all(rows[..., pt.SAL] == 1.0) and np.all(rows[..., pt.CONF] == 1.0)
    rows, lst = run("inf amp")
    assert np.all(rows[..., pt.F0] == 450.0) and np.all(np.isposinf(rows[..., pt.SAL])) and np.all(np.isnan(rows[..., pt.CONF]))
    rows, lst = run("inf amp times a zero weight")
    assert np.all(rows[..., pt.F0] == 450.0) and np.all(np.isposinf(rows[..., pt.SAL]))
    x, args = cases["inf amp times a zero weight"]
    only = pt.pitch(x, **dict(args, fmax=200.0))[0]     # 150 and 112.5 alone: both meet the inf amp at a zero weight
    assert not bits(only[..., :3]).any() and np.all(only[..., pt.NPEAKS] == 2)


KILLS = {"right_gt": "plateau", "tie_low": "equal scores", "loudest": "more peaks than npeaks", "w_h": "decay",
         "no_div_h": "deviation over h", "reverse": "order of the sum", "lt_tol": "deviation equal to tol"}


@pytest.mark.parametrize("mutant", pt.MUTANTS)
def test_the_planted_cases_tell_every_mutant_from_the_model(mutant):
    """at every size the GPU test runs, in every frame of the case planted against the mutant"""
    assert set(KILLS) == set(pt.MUTANTS)
    for size in GPU_SIZES:
        hit = []
        for name, x, args in pt.planted(size, 2, 3):
            good, bad = pt.pitch(x, **args), pt.pitch(x, mutant=mutant, **args)
            if differs(good, bad):
                hit.append(name)
            if name == KILLS[mutant]:
                rows = np.any(bits(good[0]) != bits(bad[0]), axis=-1) | np.any(bits(good[1]) != bits(bad[1]), axis=(-2, -1))
                assert rows.all(), "size %d: a frame of '%s' does not notice the mutant %s" % (size, name, mutant)
        print("PVOCPITCH mutant %s size %d: differs in %s" % (mutant, size, hit))
        assert KILLS[mutant] in hit


def test_the_list_and_the_row_do_not_depend_on_the_other_frames():
    """a row is a function of one frame: any cut of the stream, any order of the frames"""
    size, C, F = 256, 2, 9
    x = pt.tones(size, C, F, 3)
    args = dict(thresh=0.01, fmin=50.0, fmax=2000.0)
    rows, lst = pt.pitch(x, **args)
    assert np.all(rows[..., pt.F0] > 0)
    for c in range(C):
        for f in range(F):
            r1, l1 = pt.pitch(x[c:c + 1, f:f + 1], **args)
            assert np.array_equal(bits(r1[0, 0]), bits(rows[c, f])) and np.array_equal(bits(l1[0, 0]), bits(lst[c, f]))


# ---- 2. the accuracy of the method, as a condition on the model ----

KINDS = ("plain", "noise", "no fundamental", "odd harmonics")


def tone(size, f0, kind, rng):
    """3 x size samples at 48 kHz: 20 harmonics of amplitude 1 / h with a random phase each (those below sr / 2: a
    harmonic above it would fold back as a partial that is none of f0's)"""
    t = np.arange(3 * size) / SR
    x = np.zeros(3 * size)
    for h in range(1, 21):
        ph = rng.uniform(0, 2 * np.pi)
        if h * f0 >= SR / 2 or (kind == "no fundamental" and h == 1) or (kind == "odd harmonics" and h % 2 == 0):
            continue
        x += np.cos(2 * np.pi * h * f0 * t + ph) / h
    if kind == "noise":
        x += 0.02 * rng.standard_normal(len(x))
    return x


def analysed_tones(size):
    """(f0 of every tone, the frames (tones, 8, M + 1, 2)): Hann at hop size / 4 through the CPU models, without the
    frame whose previous spectrum is the initial state"""
    hop, cf = size // 4, SR / size
    rng = np.random.default_rng(size)
    f0s = np.geomspace(3.2 * cf, min(SR / 8, 40 * cf), 13)
    sig = np.stack([tone(size, f0, kind, rng) for f0 in f0s for kind in KINDS])
    X = np.fft.rfft(sm.windowed_frames_f32(sig, size, hop, hann(size)).astype(np.float64), axis=-1)
    P = pm.unbins(X).astype(np.complex64)
    fr = pm.analyze32(P, pm.initial_prev(len(sig), size), size, hop, SR)
    return np.repeat(f0s, len(KINDS)), fr[:, 1:]


@pytest.mark.parametrize("size", (64, 256, 2048))
def test_every_frame_of_a_harmonic_tone_is_within_50_cents(size):
    """50 cents is the usual criterion of a correct pitch; an octave or harmonic error is hundreds of cents"""
    f0, fr = analysed_tones(size)
    assert fr.shape[:2] == (13 * 4, 8)
    thresh = 0.01 * fr[..., 0].max(axis=-1, keepdims=True)
    rows, _ = pt.pitch(fr, thresh, 2 * SR / size, SR / 4, npeaks=16, tol=0.03, decay=0.84)
    with np.errstate(divide="ignore"):
        cents = 1200 * np.log2(rows[..., pt.F0].astype(np.float64) / f0[:, None])
    worst = np.abs(cents).max(axis=1)
    for i in np.argsort(-worst)[:3]:
        print("PVOCPITCH size %d f0 %.1f Hz %s: worst frame %.2f cents" % (size, f0[i], KINDS[i % 4], worst[i]))
    print("PVOCPITCH size %d: %d frames, %d off by more than 50 cents, the worst %.2f cents"
          % (size, cents.size, int((np.abs(cents) > 50).sum()), worst.max()))
    assert np.all(np.abs(cents) <= 50)


# ---- 3. the library: symbols and argument rules on an object without a device ----

def test_library_exports_the_pitch_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in ("clfa_pvoc_pitch_dev", "clfa_pvoc_pitch", "clfa_pvoc_pitch_kernel_name"):
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.pitch_kernel_name() == ""
    pv = fa.Pvoc(0, 64, 16, SR, 2)
    assert pv.pitch_kernel_name() == ("k_pvoc_pitch" if pv.get_error() == 0 else "")
    assert _lib.lib().clfa_pvoc_pitch_kernel_name(None) == b""
    for m in ("pitch", "pitch_device", "pitch_kernel_name"):
        assert callable(getattr(pv, m))
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/clfft_amd.h").read()
    assert "CLFA_PVOC_PITCH_DIV = 8, CLFA_PVOC_PITCH_HARM = 32, CLFA_PVOC_PITCH_PEAKS_MAX = 32" in header
    assert "CLFA_PVOC_PITCH_F0 = 0, CLFA_PVOC_PITCH_SAL = 1, CLFA_PVOC_PITCH_CONF = 2, CLFA_PVOC_PITCH_NPEAKS = 3" in header
    assert (fa.Pvoc.PITCH_F0, fa.Pvoc.PITCH_SAL, fa.Pvoc.PITCH_CONF, fa.Pvoc.PITCH_NPEAKS) == (0, 1, 2, 3)
    assert (pt.DIV, pt.HARM, pt.PEAKS_MAX, fa.Pvoc.PITCH_PEAKS_MAX) == (8, 32, 32, 32)


def test_argument_errors_come_before_the_device_lookup():
    size, C, F, NP = 64, 2, 3, 5
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    a = pt.tones(size, C, F, 5)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    rows = np.full((C, F, 4), 7, f32)
    lst = np.full((C, F, NP, 2), 9, f32)
    assert a.ctypes.data % 8 == 0 and lst.ctypes.data % 8 == 0
    nan, inf = float("nan"), float("inf")

    def host(a=a, r=rows, p=lst, F=F, first=1, nbins=M - 1, npk=NP, thresh=0.01, fmin=50.0, fmax=2000.0, tol=0.03, decay=0.84,
             h=pv._h):
        return L.clfa_pvoc_pitch(h, ptr(a), ptr(r), ptr(p), F, first, nbins, npk, thresh, fmin, fmax, tol, decay)

    def devf(a=a, r=rows, p=lst, F=F, first=1, nbins=M - 1, npk=NP, thresh=0.01, fmin=50.0, fmax=2000.0, tol=0.03, decay=0.84,
             h=pv._h):                     # the device form's checks, on host addresses
        return L.clfa_pvoc_pitch_dev(h, ptr(a), ptr(r), ptr(p), F, first, nbins, npk, thresh, fmin, fmax, tol, decay, None)

    def accepted(f, **kw):
        """a call that passes every check answers `good`; with a device present the device form would hand these host
        addresses to a kernel, so there only the blocking form is made"""
        return (f is devf and good == 0) or f(**kw) == good

    for f in (host, devf):
        assert accepted(f) and accepted(f, p=None)
        assert f(F=0) == good and f(F=-1) == CL_INVALID_VALUE
        assert f(F=0, a=None, r=None, p=None) == good
        for kw in (dict(a=None), dict(r=None), dict(h=None)):
            assert f(**kw) == CL_INVALID_VALUE, kw
        # the range: every bin of it has both neighbours
        for first, nbins in ((0, 1), (0, M), (1, M), (1, 0), (-1, 3), (M, 1), (M - 1, 2), (2, M - 1), (1, -1),
                             (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(first=first, nbins=nbins) == CL_INVALID_VALUE, (first, nbins)
            assert f(first=first, nbins=nbins, F=0) == CL_INVALID_VALUE, (first, nbins)
        for first, nbins in ((1, M - 1), (1, 1), (M - 1, 1), (M - 2, 2)):
            assert accepted(f, first=first, nbins=nbins), (first, nbins)
        for npk in (0, -1, 33, 2 ** 31 - 1):
            assert f(npk=npk) == CL_INVALID_VALUE and f(npk=npk, p=None) == CL_INVALID_VALUE, npk
            assert f(npk=npk, F=0) == CL_INVALID_VALUE, npk
        assert accepted(f, npk=1, p=None) and accepted(f, npk=32, p=None)
        bad = (dict(thresh=nan), dict(thresh=-1.0), dict(thresh=inf), dict(thresh=-1e-45),
               dict(fmin=nan), dict(fmin=0.0), dict(fmin=-50.0), dict(fmin=1e-40), dict(fmin=inf), dict(fmin=2001.0),
               dict(fmax=nan), dict(fmax=inf), dict(fmax=49.0), dict(fmax=-inf),
               dict(tol=nan), dict(tol=-0.01), dict(tol=0.51), dict(tol=inf),
               dict(decay=nan), dict(decay=0.0), dict(decay=-0.5), dict(decay=1.01), dict(decay=inf))
        for kw in bad:
            assert f(**kw) == CL_INVALID_VALUE, kw
            assert f(F=0, **kw) == CL_INVALID_VALUE, kw
        for kw in (dict(thresh=0.0), dict(thresh=-0.0), dict(thresh=3e38), dict(fmin=1.2e-38, fmax=1.2e-38), dict(fmin=50.0, fmax=50.0),
                   dict(fmax=3e38), dict(tol=0.0), dict(tol=0.5), dict(decay=1.0), dict(decay=1e-45)):
            assert accepted(f, **kw), kw
        # each output against the input and against the other output: the two share the last two words of the lower one
        args = {"a": a, "r": rows, "p": lst}
        for lower, upper in (("a", "r"), ("r", "a"), ("a", "p"), ("p", "a"), ("r", "p"), ("p", "r")):
            n0, n1 = args[lower].size, args[upper].size
            both = np.zeros(n0 + n1 + 2, f32)
            start = (-both.ctypes.data % 8) // 4
            s1 = start + n0 - 2
            v0 = both[start:start + n0].reshape(args[lower].shape)
            v1 = both[s1:s1 + n1].reshape(args[upper].shape)
            assert v0.ctypes.data % 8 == 0 and v1.ctypes.data % 8 == 0 and v1.ctypes.data < v0.ctypes.data + v0.nbytes
            assert f(**{lower: v0, upper: v1}) == CL_INVALID_VALUE, (lower, upper)
    # the device form's alignment: the frames and the list on 8 bytes, the rows on 4 (the blocking form takes any address)
    bytes_ = np.zeros(a.nbytes + 16, np.uint8)
    base = bytes_.ctypes.data + (-bytes_.ctypes.data % 8)
    for kw, off, refused in (("a", 4, True), ("p", 4, True), ("r", 2, True), ("a", 8, False), ("p", 8, False), ("r", 4, False)):
        assert devf(**{kw: base + off}) == CL_INVALID_VALUE if refused else accepted(devf, **{kw: base + off}), (kw, off)
    if good != 0:
        assert np.all(rows == 7.0) and np.all(lst == 9.0)
    # the Python layer: shapes, ranges and values; a good call gives the object's error
    with pytest.raises(ValueError):
        pv.pitch(a[:, :, :-1], 0.01, 50.0, 2000.0)
    for kw in (dict(first_bin=0), dict(first_bin=M), dict(nbins=0), dict(first_bin=2, nbins=M - 1), dict(npeaks=0), dict(npeaks=33),
               dict(tol=0.6), dict(decay=0.0), dict(decay=nan)):
        for peaks in (False, True):
            with pytest.raises(fa.ClError) as e:
                pv.pitch(a, 0.01, 50.0, 2000.0, peaks=peaks, **kw)
            assert e.value.code == CL_INVALID_VALUE
    for t, lo, hi in ((nan, 50.0, 2000.0), (0.01, 0.0, 2000.0), (0.01, 50.0, 40.0), (-1.0, 50.0, 2000.0)):
        with pytest.raises(fa.ClError) as e:
            pv.pitch(a, t, lo, hi)
        assert e.value.code == CL_INVALID_VALUE
    if good != 0:
        with pytest.raises(fa.ClError) as e:
            pv.pitch(a, 0.01, 50.0, 2000.0, peaks=True)
        assert e.value.code == good


# ---- 4. the kernel's score and peak test, built with g++ ----

SCORE_SRC = r"""
#include "pvoc_pitch_score.hpp"
extern "C" void pitch_scores(const float *A, const float *Q, const int *L, long frames, int npeaks, const float *w, float tol,
                             float *s) {
  for (long f = 0; f < frames; f++)
    for (int i = 0; i < npeaks; i++)
      for (int m = 1; m <= clfa::kPitchDiv; m++)
        s[(f * npeaks + i) * clfa::kPitchDiv + m - 1] =
            i < L[f] ? clfa::pitch_score(A + f * npeaks, Q + f * npeaks, L[f], Q[f * npeaks + i] / (float)m, w, tol) : 0.f;
}
extern "C" void pitch_peaks(const float *a, const float *q, long bins, float thresh, int *out) {
  for (long k = 1; k + 1 < bins; k++) out[k] = clfa::pitch_is_peak(a[k - 1], a[k], a[k + 1], q[k], thresh);
}
extern "C" int pitch_constants(int i) {
  return i == 0 ? clfa::kPitchDiv : (i == 1 ? clfa::kPitchHarm : clfa::kPitchPeaksMax);
}
"""


@pytest.fixture(scope="module")
def host_score(tmp_path_factory):
    d = tmp_path_factory.mktemp("pitch_score")
    src, so = str(d / "pitch_score.cpp"), str(d / "libpitch_score.so")
    with open(src, "w") as fh:
        fh.write(SCORE_SRC)
    inc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", inc, src, "-o", so])
    return ctypes.CDLL(so)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def model_scores(A, Q, L, w, tol):
    """the model's SCORE of every (i, m), serial over the list: (frames, npeaks, 8); 0 where i >= L"""
    n = A.shape[-1]
    have = np.arange(n) < L[:, None]
    with np.errstate(all="ignore"):
        c = Q[..., None] / np.arange(1, pt.DIV + 1, dtype=f32)
        s = np.zeros(c.shape, f32)
        for j in range(n):
            r = Q[:, j, None, None] / c
            h = np.rint(r)
            counts = have[:, j, None, None] & (h >= 1) & (h <= pt.HARM) & (np.abs(r - h) / h <= f32(tol))
            s = np.where(counts, s + A[:, j, None, None] * w[np.where(counts, h, 1).astype(np.int64) - 1], s)
    return np.where(have[..., None], s, f32(0))


def test_the_kernels_score_gives_the_models_bits(host_score):
    assert [host_score.pitch_constants(i) for i in range(3)] == [pt.DIV, pt.HARM, pt.PEAKS_MAX]
    host_score.pitch_scores.restype = None
    inputs = [(pt.tones(size, 3, 37, size), dict(thresh=0.01, tol=0.03, decay=0.84, npeaks=16)) for size in (64, 2048)]
    inputs += [(raw_freq_first(512, 2, 20, 5), dict(thresh=0.0, tol=0.5, decay=0.5, npeaks=32))]
    inputs += [(x, dict(pt.DEFAULTS, **args)) for _, x, args in pt.planted(256, 2, 3)]
    for x, args in inputs:
        npk, tol, first = args["npeaks"], f32(args["tol"]), args.get("first_bin", 1)
        nbins = args.get("nbins") or x.shape[2] - 1 - first
        A, Q, L = pt.peak_list(x, first, nbins, npk, args["thresh"])
        A, Q = np.ascontiguousarray(A.reshape(-1, npk)), np.ascontiguousarray(Q.reshape(-1, npk))
        L = np.ascontiguousarray(L.reshape(-1).astype(np.int32))
        w = pt.weights(args["decay"])
        got = np.full(A.shape + (pt.DIV,), 5, f32)
        host_score.pitch_scores(_ptr(A), _ptr(Q), _ptr(L), ctypes.c_long(len(L)), npk, _ptr(w), ctypes.c_float(tol), _ptr(got))
        want = model_scores(A, Q, L, w, tol)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
        # and the model's rows are the best of these scores
        rows = pt.pitch(x, **{k: v for k, v in args.items() if k != "fmin" and k != "fmax"}, fmin=1.0, fmax=3e38)[0].reshape(-1, 4)
        ok = (np.arange(npk) < L[:, None])[..., None] & ~np.isnan(got) & (Q[..., None] / np.arange(1, 9, dtype=f32) >= 1)
        best = np.where(ok, got, f32(-1)).reshape(len(L), -1).max(axis=-1)
        assert np.array_equal(rows[:, pt.SAL], np.where(best < 0, 0, best))


def test_the_kernels_peak_test_gives_the_models_mask(host_score):
    host_score.pitch_peaks.restype = None
    x = raw_freq_first(512, 2, 20, 5).copy()
    x[0, 0, 40:44, 0] = 3.0e30            # a plateau
    x[1, 3, 50, 1] = np.inf
    x[1, 3, 52, 1] = 0.0
    B = x.shape[2]
    for thresh in (0.0, 1e-3, 1e20):
        want = pt.peak_mask(x, 1, B - 2, thresh)
        assert want.any() and not want.all()
        for c in range(x.shape[0]):
            for f in range(x.shape[1]):
                a, q = np.ascontiguousarray(x[c, f, :, 0]), np.ascontiguousarray(x[c, f, :, 1])
                out = np.zeros(B, np.int32)
                host_score.pitch_peaks(_ptr(a), _ptr(q), ctypes.c_long(B), ctypes.c_float(thresh), _ptr(out))
                assert np.array_equal(out[1:B - 1].astype(bool), want[c, f]), (thresh, c, f)
