"""Nupconv's timed crossfade of response changes without a GPU: the new ABI symbols, the Python surface's answers without
a device, and the float64 model of the schedule (tests/nupconv_fade_model.py: a tail ring of n1 + 2 frames, the second
path primed from the rings alone, the sets exchanged at the end) against the definition, two objects fed alike and mixed
by g, at every push position and fade length that takes another way through the priming."""
import functools

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests.nupconv_fade_model import NupFadeModel, mixed, plain

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
GEOMS = [(4, 8, 1), (4, 16, 3), (8, 64, 2)]   # pts0, pts1, n1


@pytest.mark.parametrize("name", ["clfa_nupconv_push_ir_fade", "clfa_nupconv_push_ir_fade_dev", "clfa_nupconv_fade_remaining"])
def test_symbol_exported(name):
    assert hasattr(lib(), name)


def test_python_surface():
    for name in ("push_ir_fade", "push_ir_fade_device", "fade_remaining"):
        assert hasattr(fa.Nupconv, name), name
    assert "push_ir_fade" in fa.Nupconv.push_ir.__doc__
    assert lib().clfa_nupconv_fade_remaining(None) == 0


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_nupconv_fade.py)")
    import torch
    cvs, pts0, pts1 = 5 * 256 + 7, 64, 256
    p = fa.Nupconv(0, cvs, pts0, pts1, channels=2)
    assert p.get_error() == CL_DEVICE_NOT_FOUND
    assert p.fade_remaining() == 0
    assert p.push_ir_fade(np.zeros((2, cvs), np.float32), 3) == CL_DEVICE_NOT_FOUND
    assert p.push_ir_fade_device(torch.zeros((2, cvs)), 3, stream=0) == CL_DEVICE_NOT_FOUND
    # a failed object answers with its error, whatever the fade length
    assert p.push_ir_fade(np.zeros((2, cvs), np.float32), 0) == CL_DEVICE_NOT_FOUND
    assert p.fade_remaining() == 0
    # the row checks of the Python layer come first (without a device the object has no partitions: any row is long enough)
    assert p.push_ir_fade(np.zeros((3, cvs), np.float32), 3) == CL_INVALID_VALUE
    assert p.push_ir_fade(np.zeros((2, 2, cvs), np.float32), 3) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.push_ir_fade_device(torch.zeros((3, cvs)), 3, stream=0)


def _cvs(pts1, n1):
    return 2 * pts1 + n1 * pts1 + 3   # a remainder, dropped


@functools.lru_cache(maxsize=None)
def _case(pts0, pts1, n1):
    """(hA, hB, hC, x, yA, yB, yC): responses, a signal long enough for every case of the grid, and what the objects that
    always held A, B, C return for it; read-only"""
    m, channels = pts1 // pts0, 2
    cvs = _cvs(pts1, n1)
    nblocks = (n1 + 4) * m + (m - 1) + (2 * m + 3) + (n1 + 4) * m   # the latest push, the longest fade, n1 + 4 periods
    rng = np.random.default_rng(1000 * pts0 + pts1 + n1)
    hs = [rng.random((channels, cvs)) - 0.5 for _ in range(3)]
    x = rng.random((channels, nblocks * pts0)) - 0.5
    out = hs + [x] + [plain(h, x, cvs, pts0, pts1) for h in hs]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _fade(pts0, pts1, n1, c, fade, nblocks, extra=2, hB=None):
    """the model pushed at position c: its output over nblocks blocks, fade_remaining() checked block by block"""
    hA, hB_, _, x, _, _, _ = _case(pts0, pts1, n1)
    model = NupFadeModel(_cvs(pts1, n1), pts0, pts1, x.shape[0], extra=extra)
    model.push_ir(hA)
    out = [model.process(x[:, :c * pts0])]
    assert model.position == c
    model.push_ir_fade(hB_ if hB is None else hB, fade)
    for j in range(c, nblocks):
        assert model.fade_remaining() == max(0, fade - (j - c))
        out.append(model.process(x[:, j * pts0:(j + 1) * pts0]))
    assert model.fade_remaining() == 0
    return np.concatenate(out, axis=1)


def _grid(pts0, pts1, n1):
    m = pts1 // pts0
    return [(P, s, fade) for P in range(n1 + 5) for s in sorted({0, 1, m - 1}) for fade in sorted({1, m - 1, m + 1, 2 * m + 3})]


def test_the_grid_has_216_cases():
    assert sum(len(_grid(*g)) for g in GEOMS) == 216


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_model_matches_the_definition(pts0, pts1, n1):
    m = pts1 // pts0
    _, _, _, x, yA, yB, _ = _case(pts0, pts1, n1)
    peak = np.max(np.abs(yA))
    for P, s, fade in _grid(pts0, pts1, n1):
        c = P * m + s
        nblocks = c + fade + (n1 + 4) * m       # n1 + 4 periods past the fade's end: a wrong exchange shows
        assert nblocks * pts0 <= x.shape[1]
        L = nblocks * pts0
        want = mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        got = _fade(pts0, pts1, n1, c, fade, nblocks)
        err = np.max(np.abs(got - want)) / peak
        assert err < 1e-12, ("P %d s %d fade %d" % (P, s, fade), err)
        # the fade is audible: the two ends differ after it
        after = (c + fade) * pts0
        assert np.max(np.abs(yA[:, after:L] - yB[:, after:L])) > 1e-3 * peak


def test_a_ring_of_n1_plus_1_frames_is_too_short():
    """at phase s > 0 of period P tail block P - 3 reads input block P - 2 - n1, which a ring of n1 + 1 frames has lost"""
    pts0, pts1, n1 = 4, 8, 1
    m, P, s, fade = 2, 3, 1, 3
    _, _, _, _, yA, yB, _ = _case(pts0, pts1, n1)
    c = P * m + s
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    peak = np.max(np.abs(yA))
    assert np.max(np.abs(_fade(pts0, pts1, n1, c, fade, nblocks, extra=1) - want)) > 1e-3 * peak
    assert np.max(np.abs(_fade(pts0, pts1, n1, c, fade, nblocks, extra=2) - want)) < 1e-12 * peak


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_a_fade_from_a_to_a_is_no_push(pts0, pts1, n1):
    m = pts1 // pts0
    hA, _, _, _, yA, _, _ = _case(pts0, pts1, n1)
    peak = np.max(np.abs(yA))
    for c, fade in ((0, 1), (1, m + 1), (2 * m + m - 1, 2 * m + 3), ((n1 + 3) * m + 1, m + 1)):
        nblocks = c + fade + (n1 + 4) * m
        got = _fade(pts0, pts1, n1, c, fade, nblocks, hB=hA)
        assert np.max(np.abs(got - yA[:, :nblocks * pts0])) < 1e-12 * peak, (c, fade)


def test_a_second_fade_gives_b_then_c():
    pts0, pts1, n1 = 4, 16, 3
    m = pts1 // pts0
    hA, hB, hC, x, yA, yB, yC = _case(pts0, pts1, n1)
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                          # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    model = NupFadeModel(_cvs(pts1, n1), pts0, pts1, x.shape[0])
    model.push_ir(hA)
    out = [model.process(x[:, :c1 * pts0])]
    model.push_ir_fade(hB, f1)
    with pytest.raises(AssertionError):
        model.push_ir_fade(hC, f2)                # one fade at a time
    out.append(model.process(x[:, c1 * pts0:c2 * pts0]))
    assert model.fade_remaining() == 0
    model.push_ir_fade(hC, f2)
    out.append(model.process(x[:, c2 * pts0:L]))
    got = np.concatenate(out, axis=1)
    want = mixed(mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    peak = np.max(np.abs(yA))
    assert np.max(np.abs(got - want)) < 1e-12 * peak
    assert np.max(np.abs(yB[:, (c2 + f2) * pts0:L] - yC[:, (c2 + f2) * pts0:L])) > 1e-3 * peak
