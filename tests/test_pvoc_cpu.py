"""The phase vocoder (clfa_pvoc) without a GPU: the numpy model of its definitions (tests/pvoc_model.py) — the integer
phase is the same for every chunking and every split into calls, a stationary sinusoid reports its frequency, synthesis
inverts analysis — and the library's new symbols and creation checks."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_model as pm

CL_INVALID_VALUE = -30
SR = 48000.0


def _freqs(rng, C, F, size, sr=SR):
    """plausible and hostile freq values: around the bin centres, far outside, negative, huge, non-finite"""
    B = size // 2 + 1
    f = (np.arange(B) * (sr / size) + rng.standard_normal((C, F, B)) * sr / 64).astype(np.float32)
    f[0, 0, 1] = np.nan
    f[-1, F // 2, 2] = np.inf
    f[0, F - 1, 3] = -np.float32(3.4e38)
    f[0, 0, 4] = 1e9
    return f


@pytest.mark.parametrize("chunk", [1, 3, 7])
def test_serial_phase_equals_chunked_scan(chunk):
    size, hop, C, F = 64, 16, 2, 23
    rng = np.random.default_rng(chunk)
    freq = _freqs(rng, C, F, size)
    th0 = rng.integers(0, 2 ** 32, (C, size // 2 + 1), dtype=np.uint64).astype(np.uint32)
    serial, s_state = pm.phases(freq, th0, hop, SR)
    chunked, c_state = pm.phases_chunked(freq, th0, hop, SR, chunk)
    assert np.array_equal(serial, chunked) and np.array_equal(s_state, c_state)
    assert serial[0, 0, 1] == th0[0, 1], "a NaN freq must not advance the phase"


@pytest.mark.parametrize("cuts", [(1,), (5, 6), (1, 2, 3, 22), (22,)])
def test_phase_is_the_same_for_any_split_into_calls(cuts):
    size, hop, C, F = 64, 3, 2, 23
    rng = np.random.default_rng(len(cuts))
    freq = _freqs(rng, C, F, size)
    th0 = pm.initial_phase(C, size)
    whole, w_state = pm.phases(freq, th0, hop, SR)
    parts, state = [], th0
    for a, b in zip((0,) + cuts, cuts + (F,)):
        th, state = pm.phases_chunked(freq[:, a:b], state, hop, SR, 3)
        parts.append(th)
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(state, w_state)


def test_increment_is_the_stated_arithmetic():
    """one value by hand: freq 1000.5 Hz, hop 64, sr 48000 -> t = fl(freq * fl(64 / 48000)), r = t - rint(t), inc = r 2^32"""
    kf = np.float32(64 / 48000.0)
    t = np.float32(1000.5) * kf
    r = np.float32(t - np.rint(t))
    want = int(np.rint(float(r) * 2.0 ** 32)) % 2 ** 32
    got = pm.increments(np.array([[[1000.5]]], np.float32), 64, 48000.0)
    assert int(got[0, 0, 0]) == want and 0 < want < 2 ** 32
    # r = +-1/2 exactly: 2^31 either way
    assert int(pm.increments(np.array([[[0.5, -0.5]]], np.float32), 1, 1.0)[0, 0, 0]) == 2 ** 31
    assert int(pm.increments(np.array([[[0.5, -0.5]]], np.float32), 1, 1.0)[0, 0, 1]) == 2 ** 31
    assert not pm.increments(np.array([[[np.nan, np.inf, -np.inf]]], np.float32), 64, 48000.0).any()


def _stft_packed(x, size, hop, w):
    """float64 frames of x -> the library's packed layout and scaling (Clrfft forward), complex64, (1, F, M)"""
    F = 1 + (x.size - size) // hop
    fr = np.stack([x[f * hop:f * hop + size] * w for f in range(F)])
    return fa.onesided_to_packed(np.fft.rfft(fr, axis=-1)).astype(np.complex64)[None]


def test_stationary_sinusoid_reports_its_frequency():
    size, hop = 256, 64
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)
    f0 = 20.37 * SR / size                                   # between bins 20 and 21
    x = 0.8 * np.cos(2 * np.pi * f0 * np.arange(size + 12 * hop) / SR + 0.3)
    P = _stft_packed(x, size, hop, w)
    for fr in (pm.analyze32(P, pm.initial_prev(1, size), size, hop, SR),
               np.stack(pm.analyze64(P, pm.initial_prev(1, size), size, hop, SR)[0:3:2], axis=-1)):
        for k in (20, 21):                                   # the peak bins, every frame after the first
            assert np.abs(fr[0, 1:, k, 1] - f0).max() < 1e-3 * SR / size, (k, fr[0, 1:, k, 1])
        assert fr[0, 1:, 20, 0].min() > 10 * fr[0, 1:, 40, 0].max()


def test_model_synthesis_inverts_model_analysis():
    size, hop, C, F = 64, 16, 2, 9
    M = size // 2
    rng = np.random.default_rng(7)
    P = (rng.standard_normal((C, F, M)) + 1j * rng.standard_normal((C, F, M))).astype(np.complex64)
    P[0, :, 0] = -np.abs(P[0, :, 0].real) - 1j * np.abs(P[0, :, 0].imag)     # Re P[0] < 0 and Im P[0] < 0
    P[1, 3, 0] = -2.5 + 0.75j
    amp, dev, freq, prev = pm.analyze64(P, pm.initial_prev(C, size), size, hop, SR)
    assert np.array_equal(prev, pm.bins(P[:, -1]))
    frames = np.stack([amp, freq], axis=-1).astype(np.float32)
    theta, _ = pm.phases(frames[..., 1], pm.initial_phase(C, size), hop, SR)
    back = pm.synth64(frames, theta)
    # freq is a float32 of about k + 4 dev: dev, and with it every phase increment, carries about 2^-24 (M / 4) turns of
    # rounding, accumulated over F frames
    tol = 2 * np.pi * F * 2.0 ** -24 * M
    assert pm.rel_l2(back, P) < tol, (pm.rel_l2(back, P), tol)
    for k in (0, M // 2):
        assert pm.rel_l2(back[..., k], P[..., k]) < tol, k
    assert np.all(back[0, :, 0].real < 0) and np.all(back[0, :, 0].imag < 0)      # bins 0 and M keep their signs
    assert pm.rel_l2(pm.synth32(frames, theta), P) < tol
    # the float32 analysis agrees with the float64 one on the phasors
    f32 = pm.analyze32(P, pm.initial_prev(C, size), size, hop, SR)
    assert pm.rel_l2(pm.phasors(f32, size, hop, SR), amp * np.exp(2j * np.pi * dev)) < tol


def test_bins_and_unbins_are_the_layout_map():
    P = np.array([[1 - 2j, 3 + 4j, 5 + 6j, 7 - 8j]], np.complex64)       # M = 4
    z = pm.bins(P)
    assert np.array_equal(z, np.array([[1, 3 + 4j, 5 - 6j, 7 - 8j, -2]], np.complex64))
    assert np.array_equal(pm.unbins(z), P)
    # a zero spectrum: amp 0, dev 0, the bin-centre frequencies
    amp, dev, freq, _ = pm.analyze64(np.zeros((1, 2, 32), np.complex64), pm.initial_prev(1, 64), 64, 16, SR)
    assert not amp.any() and not dev.any() and np.array_equal(freq[0, 1], np.arange(33) * SR / 64)


def test_library_exports_the_pvoc_symbols():
    names = ["clfa_pvoc_create", "clfa_pvoc_destroy", "clfa_pvoc_get_error", "clfa_pvoc_get_log", "clfa_pvoc_reset",
             "clfa_pvoc_analyze_dev", "clfa_pvoc_synthesize_dev", "clfa_pvoc_analyze", "clfa_pvoc_synthesize",
             "clfa_pvoc_kernel_name", "clfa_pvoc_workspace_bytes", "clfa_pvoc_scan_chunk", "clfa_pvoc_read_phase",
             "clfa_pvoc_read_prev"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    assert fa.Pvoc(0, 48, 16, SR).scan_chunk() >= 1


@pytest.mark.parametrize("size,hop,sr,channels", [(48, 16, SR, 1), (32, 8, SR, 1), (32768, 64, SR, 1), (256, 0, SR, 1),
                                                  (256, 257, SR, 1), (256, 64, 0.0, 1), (256, 64, -1.0, 1),
                                                  (256, 64, float("nan"), 1), (256, 64, float("inf"), 1), (256, 64, SR, 0)])
def test_create_reports_bad_arguments_without_a_device(size, hop, sr, channels):
    pv = fa.Pvoc(0, size, hop, sr, channels)
    assert pv.get_error() == CL_INVALID_VALUE and pv.get_log() != ""
    assert pv.kernel_name() == "" and pv.workspace_bytes() == 0
    assert pv.reset() == CL_INVALID_VALUE


def test_valid_arguments_reach_the_device_lookup():
    pv = fa.Pvoc(0, 256, 64, SR, channels=3)
    assert pv.get_error() == (0 if fa.device_count() > 0 else -1)
