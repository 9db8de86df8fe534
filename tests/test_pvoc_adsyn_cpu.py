"""The oscillator bank of clfa_pvoc (clfa_pvoc_adsyn) without a GPU: the integer arithmetic the kernels use
(opencl_fft_amd/csrc/pvoc_adsyn_plan.hpp, built here with g++) against Python integers; properties of the model of its
definition (tests/pvoc_adsyn_model.py); and the library's new symbols and argument checks, which come before any device
lookup, so they answer on a machine without a device too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_adsyn_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL_INVALID_VALUE = -30
f32 = np.float32

WRAPPERS = r"""
#include "pvoc_adsyn_plan.hpp"
using namespace clfa;
extern "C" {
float t_turns(float freq, float fmod, int has, float ks) { return adsyn_turns(freq, fmod, has != 0, ks); }
int t_word(float t, int *w) { int32_t v; const bool ok = adsyn_word(t, v); *w = v; return ok; }
void t_endpoint(float amp, float freq, float fmod, int has, float ks, int *w, float *a) {
  int32_t v; adsyn_endpoint(amp, freq, fmod, has != 0, ks, v, *a); *w = v;
}
int t_start(float a0, int w0, int wf) { return adsyn_start(a0, w0, wf); }
unsigned long long t_slope(int w0, int wf, int hop) { return adsyn_slope(w0, wf, hop); }
unsigned long long t_advance(int w0, unsigned long long d, int hop) { return adsyn_advance(w0, d, hop); }
// one frame step: (*w, *a) moves on to the frame's endpoint
unsigned long long t_step(int *w, float *a, float amp, float freq, float fmod, int has, float ks, int hop, int *ws,
                          unsigned long long *d) {
  int32_t w1 = *w, s; uint64_t dd;
  const uint64_t adv = adsyn_step(w1, *a, amp, freq, fmod, has != 0, ks, hop, s, dd);
  *w = w1; *ws = s; *d = dd;
  return adv;
}
// phase(j) and the hot loop's top word, j = 1..hop
void t_phases(unsigned long long p, int w0, unsigned long long d, int hop, unsigned long long *out, unsigned *hi) {
  for (int j = 1; j <= hop; j++) {
    out[j - 1] = adsyn_phase(p, w0, d, (uint32_t)j);
    hi[j - 1] = adsyn_phase_hi(p, w0, d, (uint32_t)j, adsyn_tri((uint32_t)j));
  }
}
}
"""

HOPS = list(range(1, 65)) + [255, 256, 16384]
TOP = 2 ** 31 - 128


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("adsyn_plan")
    src, so = d / "adsyn_plan.cpp", str(d / "adsyn_plan.so")
    src.write_text(WRAPPERS)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I",
                           os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(src), "-o", so])
    L = ctypes.CDLL(so)
    u64, i32, fl = ctypes.c_ulonglong, ctypes.c_int, ctypes.c_float
    L.t_turns.restype, L.t_turns.argtypes = fl, [fl, fl, i32, fl]
    L.t_word.restype, L.t_word.argtypes = i32, [fl, ctypes.POINTER(i32)]
    L.t_endpoint.restype, L.t_endpoint.argtypes = None, [fl, fl, fl, i32, fl, ctypes.POINTER(i32), ctypes.POINTER(fl)]
    L.t_start.restype, L.t_start.argtypes = i32, [fl, i32, i32]
    L.t_slope.restype, L.t_slope.argtypes = u64, [i32, i32, i32]
    L.t_advance.restype, L.t_advance.argtypes = u64, [i32, u64, i32]
    L.t_phases.restype, L.t_phases.argtypes = None, [u64, i32, u64, i32, ctypes.c_void_p, ctypes.c_void_p]
    L.t_step.restype = u64
    L.t_step.argtypes = [ctypes.POINTER(i32), ctypes.POINTER(fl), fl, fl, fl, i32, fl, i32, ctypes.POINTER(i32), ctypes.POINTER(u64)]
    return L


def _words(rng, n):
    special = [0, 1, -1, TOP, -TOP, 2, -2, 12345, -12345, 2 ** 30, -(2 ** 30), TOP - 128]
    return special + [int(v) for v in rng.integers(-TOP, TOP + 1, n)]


def test_header_words_and_start_rule(plan):
    ks = f32(1.0 / 48000.0)
    rng = np.random.default_rng(1)
    freqs = np.concatenate([[0.0, -0.0, 1e-30, 23999.9, 24000.0, -24000.0, 23999.998, -23999.998, 1e9, np.inf, -np.inf, np.nan],
                            rng.uniform(-30000, 30000, 300)]).astype(f32)
    w, a = ctypes.c_int(), ctypes.c_float()
    seen = set()
    for fr in freqs:
        for fm in (None, f32(0.5), f32(2.0), f32(np.nan)):
            with np.errstate(invalid="ignore", over="ignore"):
                t = fr * ks if fm is None else (fr * fm) * ks
            got_t = plan.t_turns(fr, 1.0 if fm is None else fm, int(fm is not None), ks)
            assert np.array_equal(f32(got_t).view(np.uint32), f32(t).view(np.uint32)) or (np.isnan(t) and np.isnan(got_t))
            want, good = am.word(t)
            assert (plan.t_word(t, ctypes.byref(w)) != 0) == good and w.value == want, (fr, fm)
            plan.t_endpoint(3.0, fr, 1.0 if fm is None else fm, int(fm is not None), ks, ctypes.byref(w), ctypes.byref(a))
            assert w.value == want and a.value == (3.0 if good else 0.0)
            seen.add(good)
    assert seen == {True, False}
    # the largest float below 1/2 gives 2^31 - 128, the float 1/2 itself is silent
    assert am.word(np.nextafter(f32(0.5), f32(0))) == (TOP, True) and am.word(f32(-0.5)) == (0, False)
    assert plan.t_word(np.nextafter(f32(0.5), f32(0)), ctypes.byref(w)) == 1 and w.value == TOP
    assert plan.t_word(np.nextafter(f32(-0.5), f32(0)), ctypes.byref(w)) == 1 and w.value == -TOP
    # a NaN amp with a good t is kept
    plan.t_endpoint(np.nan, 100.0, 1.0, 0, ks, ctypes.byref(w), ctypes.byref(a))
    assert np.isnan(a.value) and w.value == am.word(f32(100.0) * ks)[0]
    for a0 in (0.0, -0.0, 1e-45, 1.0, np.nan):
        assert plan.t_start(a0, 7, -9) == am.start(a0, 7, -9) == (-9 if a0 == 0 else 7)


def test_header_slope_phase_and_advance_against_python_integers(plan):
    rng = np.random.default_rng(2)
    words = _words(rng, 14)
    negative_inexact = 0
    for hop in HOPS:
        out, hi = np.zeros(hop, np.uint64), np.zeros(hop, np.uint32)
        # every pair of words for D and the advance; phase(j) for every j on a few pairs (every pair for small hops)
        stride = 1 if hop <= 64 else (29 if hop <= 256 else 97)
        for n, (w0, wf) in enumerate((a, b) for a in words for b in words):
            d = am.slope(w0, wf, hop)
            assert plan.t_slope(w0, wf, hop) == d, (hop, w0, wf)
            q, r = divmod((wf - w0) << 30, hop)
            assert d == (4 * q) & am.MASK64 and 0 <= r < hop
            negative_inexact += wf < w0 and r != 0
            assert plan.t_advance(w0, d, hop) == am.advance(w0, d, hop), (hop, w0, wf)
            if n % stride:
                continue
            p = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
            plan.t_phases(p, w0, d, hop, out.ctypes.data, hi.ctypes.data)
            want = [am.phase(p, w0, d, j) for j in range(1, hop + 1)]
            assert out.tolist() == want, (hop, w0, wf)
            assert hi.tolist() == [v >> 32 for v in want], (hop, w0, wf)
            assert want[-1] == (p + am.advance(w0, d, hop)) & am.MASK64
    assert negative_inexact > 1000      # the floor towards minus infinity was exercised


def _same_float(a, b):
    return np.array_equal(f32(a).view(np.uint32), f32(b).view(np.uint32)) or (np.isnan(a) and np.isnan(b))


def test_header_step_is_the_composition_of_its_parts(plan):
    """adsyn_step, which k_adsyn_sums calls, against endpoint, start rule, slope and advance called one by one: over the
    frequencies and multipliers of the endpoint test (silent endpoints among them), the words of the slope test as the
    endpoint before and previous amps that do and do not restart the oscillator (0, -0, a denormal, 1, NaN), each with a
    frame amp of 3, 0, -0 or NaN and a hop of 1 .. 16384 drawn independently (the whole product: tests/cpp/adsyn_step_check.cpp)"""
    ks = f32(1.0 / 48000.0)
    rng = np.random.default_rng(6)
    freqs = np.concatenate([[0.0, -0.0, 1e-30, 23999.9, 24000.0, -24000.0, 23999.998, -23999.998, 1e9, np.inf, -np.inf, np.nan],
                            rng.uniform(-30000, 30000, 12)]).astype(f32)
    words = _words(rng, 2)
    amps = [f32(3.0), f32(0.0), f32(-0.0), f32(np.nan)]
    hops = [1, 2, 3, 7, 16, 63, 64, 255, 256, 16384]
    i32, fl, u64 = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong
    wf, af, w, a, ws, d = i32(), fl(), i32(), fl(), i32(), u64()
    silent = restarted = negative_inexact = 0
    for fr in freqs:
        for fm in (None, f32(0.5), f32(2.0), f32(np.nan)):
            has, fmv = int(fm is not None), 1.0 if fm is None else fm
            for w0 in words:
                for a0 in (0.0, -0.0, 1e-45, 1.0, np.nan):
                    amp, hop = amps[rng.integers(len(amps))], hops[rng.integers(len(hops))]
                    plan.t_endpoint(amp, fr, fmv, has, ks, ctypes.byref(wf), ctypes.byref(af))
                    ws_want = plan.t_start(a0, w0, wf.value)
                    d_want = plan.t_slope(ws_want, wf.value, hop)
                    w.value, a.value = w0, a0
                    adv = plan.t_step(ctypes.byref(w), ctypes.byref(a), amp, fr, fmv, has, ks, hop, ctypes.byref(ws), ctypes.byref(d))
                    what = (fr, fm, w0, a0, amp, hop)
                    assert (w.value, ws.value, d.value) == (wf.value, ws_want, d_want), what
                    assert _same_float(a.value, af.value), what
                    assert adv == plan.t_advance(ws_want, d_want, hop) == am.advance(ws_want, d_want, hop), what
                    silent += not am.word(f32(plan.t_turns(fr, fmv, has, ks)))[1]
                    restarted += ws_want != w0
                    negative_inexact += wf.value < ws_want and ((wf.value - ws_want) << 30) % hop != 0
    assert silent > 100 and restarted > 100 and negative_inexact > 100, (silent, restarted, negative_inexact)


def test_step_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/cpp/adsyn_step_check.cpp, a program of its own: adsyn_step against the composition over the full grid (every
    hop), built with -fsanitize=address,undefined; any report ends it with a non-zero status"""
    exe = str(tmp_path / "adsyn_step_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",     # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "adsyn_step_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "adsyn_step ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def _random_frames(rng, C, F, size, sr):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32)
    freq = (np.arange(B) * (sr / size) + rng.standard_normal((C, F, B)) * sr / size).astype(f32)
    amp[rng.random((C, F, B)) < 0.125] = 0
    freq[rng.random((C, F, B)) < 0.125] = sr        # silent endpoints
    return np.stack([amp, freq], axis=-1)


def test_model_numpy_integers_equal_python_integers():
    size, hop, sr, C, F = 64, 5, 48000.0, 2, 7
    rng = np.random.default_rng(3)
    fr = _random_frames(rng, C, F, size, sr)
    fmod = np.array([1, 0.5, 2, np.nan, 1, 1.5, 0.99], f32)
    st = am.initial_state(C, size)
    seg, new = am.segments(fr, st, hop, sr, fmod)
    ks = f32(1.0 / sr)
    for c in range(C):
        for k in range(size // 2 + 1):
            p, w0, a0 = 0, 0, 0.0
            for f in range(F):
                with np.errstate(invalid="ignore"):
                    wf, good = am.word((fr[c, f, k, 1] * fmod[f]) * ks)
                af = float(fr[c, f, k, 0]) if good else 0.0
                ws = am.start(a0, w0, wf)
                d = am.slope(ws, wf, hop)
                assert (int(seg["base"][c, f, k]), int(seg["W0"][c, f, k]), int(seg["D"][c, f, k])) == (p, ws, d)
                assert [int(v) for v in am._frame_phase(seg, f)[c, :, k]] == [am.phase(p, ws, d, j) for j in range(1, hop + 1)]
                p, w0, a0 = am.phase(p, ws, d, hop), wf, af
            assert (int(new[0][c, k]), int(new[1][c, k]), float(new[2][c, k])) == (p, w0, a0)


@pytest.mark.parametrize("sel", [(0, None, 1), (1, 5, 3)])
def test_model_split_at_every_position(sel):
    size, hop, sr, C, F = 64, 6, 48000.0, 2, 9
    rng = np.random.default_rng(4)
    fr = _random_frames(rng, C, F, size, sr)
    fmod = rng.uniform(0.5, 2.0, F).astype(f32)
    bins = am.selection(size // 2, *sel)
    seg, whole = am.segments(fr, am.initial_state(C, size), hop, sr, fmod, bins)
    y32, y64 = am.samples32(seg, 0.5), am.samples64(seg, 0.5)
    for cut in range(0, F + 1):
        sa, mid = am.segments(fr[:, :cut], am.initial_state(C, size), hop, sr, fmod[:cut], bins)
        sb, end = am.segments(fr[:, cut:], mid, hop, sr, fmod[cut:], bins)
        assert all(np.array_equal(a, b) for a, b in zip(end, whole)), cut
        parts32 = [am.samples32(s, 0.5) for s in (sa, sb) if s is not None]
        parts64 = [am.samples64(s, 0.5) for s in (sa, sb) if s is not None]
        assert np.array_equal(np.concatenate(parts32, axis=1).view(np.uint32), y32.view(np.uint32)), cut
        assert np.array_equal(np.concatenate(parts64, axis=1), y64), cut
    # the bins outside the selection kept their state
    rest = np.setdiff1d(np.arange(size // 2 + 1), bins)
    assert not whole[0][:, rest].any() and not whole[1][:, rest].any() and not whole[2][:, rest].any()


def test_model_constant_frame_is_a_cosine():
    """sr = 32768 makes ks and f0 / sr exact in float32, so the oscillator's frequency is f0 itself"""
    size, hop, sr, F = 64, 16, 32768.0, 40
    M = size // 2
    A, f0, k0 = 0.75, 1000.5, 3
    fr = np.zeros((1, F, M + 1, 2), f32)
    fr[0, :, k0] = (A, f0)
    seg, st = am.segments(fr, am.initial_state(1, size), hop, sr)
    y = am.samples64(seg)[0]
    n = np.arange(1, F * hop + 1)
    want = A * np.cos(2 * np.pi * f0 * n / sr)
    # the frame whose previous amp is 0 starts at its own frequency (no glide from W = 0): only its amplitude ramps
    assert seg["W0"][0, 0, k0] == seg["W0"][0, 1, k0] == am.word(f32(f0) * f32(1 / sr))[0] != 0
    assert np.abs(y[hop:] - want[hop:]).max() < 1e-12
    assert np.abs(y[:hop] - want[:hop] * (np.arange(1, hop + 1) / hop)).max() < 1e-12
    assert np.abs(am.samples32(seg)[0] - want * np.minimum(n / hop, 1)).max() < 1e-5
    assert st[1][0, k0] == seg["W0"][0, 0, k0] and st[2][0, k0] == f32(A)


def test_model_silent_endpoints():
    size, hop, sr, F = 64, 8, 48000.0, 3
    M = size // 2
    fr = np.zeros((1, F, M + 1, 2), f32)
    fr[..., 0] = 1.0
    for k, bad in enumerate([24000.0, -24000.0, 30000.0, np.nan, np.inf, -np.inf]):
        fr[0, :, k, 1] = bad
    seg, st = am.segments(fr, am.initial_state(1, size), hop, sr)
    assert not st[0][0, :6].any() and not st[1][0, :6].any() and not st[2][0, :6].any()
    y = am.samples64(seg)
    assert np.isfinite(y).all()
    # the other bins are at 0 Hz with amp 1: a ramp, then a constant
    assert np.allclose(y[0, hop:], M + 1 - 6)
    assert am.word(f32(23999.0) * f32(1 / sr))[1]


NEW_SYMBOLS = ["clfa_pvoc_adsyn_dev", "clfa_pvoc_adsyn", "clfa_pvoc_adsyn_read_state", "clfa_pvoc_adsyn_workspace_bytes",
               "clfa_pvoc_adsyn_tile_bins", "clfa_pvoc_adsyn_kernel_name"]


def test_library_exports_the_adsyn_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, 48000.0)
    assert bad.adsyn_kernel_name() == "" and bad.adsyn_workspace_bytes() == 0
    assert bad.adsyn_tile_bins() >= 64


def test_argument_errors_come_before_the_device_lookup():
    size, hop, C, F = 64, 16, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, hop, 48000.0, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    fr = _random_frames(np.random.default_rng(5), C, F, size, 48000.0)
    out = np.full((C, F * hop), 7.0, f32)
    fmod = np.ones(F, f32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(frames=fr, F=F, fmod=fmod, first=0, nbins=M + 1, step=1, o=out, stride=F * hop):
        return L.clfa_pvoc_adsyn(pv._h, p(frames), F, p(fmod), first, nbins, step, 1.0, p(o), stride)

    assert call() == good and call(fmod=None) == good and call(F=0, stride=0) == good
    assert call(first=M, nbins=1) == good and call(first=1, nbins=M // 2, step=2) == good
    assert call(step=0) == CL_INVALID_VALUE and call(step=-1) == CL_INVALID_VALUE
    assert call(first=1) == CL_INVALID_VALUE                      # a selection past M
    assert call(first=2, nbins=M // 2, step=2) == good and call(first=2, nbins=M // 2 + 1, step=2) == CL_INVALID_VALUE
    assert call(first=-1, nbins=1) == CL_INVALID_VALUE and call(first=M + 1, nbins=1) == CL_INVALID_VALUE
    assert call(nbins=0) == CL_INVALID_VALUE
    assert call(stride=F * hop - 1) == CL_INVALID_VALUE
    assert call(frames=None) == CL_INVALID_VALUE and call(o=None) == CL_INVALID_VALUE
    assert call(F=-1) == CL_INVALID_VALUE
    # an output that overlaps the frames or fmod, even partly
    flat = fr.reshape(-1)
    assert call(o=flat[2:]) == CL_INVALID_VALUE
    both = np.zeros(C * F * hop + F, f32)
    assert call(fmod=both[C * F * hop - 1:C * F * hop - 1 + F], o=both[:C * F * hop]) == CL_INVALID_VALUE
    assert L.clfa_pvoc_adsyn(None, p(fr), F, None, 0, 1, 1, 1.0, p(out), F * hop) == CL_INVALID_VALUE
    assert L.clfa_pvoc_adsyn_dev(pv._h, None, F, None, 0, 1, 1, 1.0, p(out), F * hop, None) == CL_INVALID_VALUE
    assert L.clfa_pvoc_adsyn_dev(pv._h, p(fr), F, None, 0, 1, 0, 1.0, p(out), F * hop, None) == CL_INVALID_VALUE
    if good != 0:
        assert (out == 7.0).all()          # nothing was computed anywhere
        with pytest.raises(fa.ClError):
            pv.adsyn(fr)
        with pytest.raises(fa.ClError):
            pv.adsyn_state()
    # an object whose creation arguments were bad keeps answering with that error
    bad_pv = fa.Pvoc(0, 48, 16, 48000.0)
    assert L.clfa_pvoc_adsyn(bad_pv._h, p(fr), F, None, 0, 1, 1, 1.0, p(out), F * hop) == CL_INVALID_VALUE
    with pytest.raises(fa.ClError) as e:
        pv.adsyn(fr, step=0)
    assert e.value.code == CL_INVALID_VALUE
