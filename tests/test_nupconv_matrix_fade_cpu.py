"""NupconvMatrix's timed crossfade of response changes without a GPU: the new ABI symbols, the Python surface's answers
without a device, and the float64 model of the schedule (tests/nupconv_matrix_fade_model.py: a tail ring of n1 + 2 frames
per input, the second set primed from the rings alone, the sets exchanged at the end, segments included) against the
definition — `mixed` of two tests.nupconv_matrix_model.definition results, two objects fed alike — at every push position
and fade length that takes another way through the priming."""
import functools

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests.nupconv_matrix_fade_model import NupMatrixFadeModel, mixed
from tests.nupconv_matrix_model import definition
from tests.test_nupconv_matrix_cpu import _cutting

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
GEOMS = [(4, 8, 1), (4, 16, 3), (8, 64, 2)]   # pts0, pts1, n1
NAMES = ["clfa_nupconv_matrix_push_ir_fade", "clfa_nupconv_matrix_push_ir_fade_dev", "clfa_nupconv_matrix_fade_remaining"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported_and_bound(name):
    assert hasattr(lib(), name)
    assert name in {s[0] for s in fa._lib.SYMBOLS}


def test_python_surface():
    for name in ("fade_ir", "fade_ir_device", "fade_remaining"):
        assert hasattr(fa.NupconvMatrix, name), name
    assert "fade_ir" in fa.NupconvMatrix.push_ir.__doc__
    assert lib().clfa_nupconv_matrix_fade_remaining(None) == 0


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_nupconv_matrix_fade.py)")
    import torch
    cvs, pts0, pts1, I, O = 5 * 256 + 7, 64, 256, 3, 2
    p = fa.NupconvMatrix(0, cvs, pts0, pts1, I, O)
    assert p.get_error() == CL_DEVICE_NOT_FOUND
    assert p.fade_remaining() == 0
    assert p.fade_ir(np.zeros((O, I, cvs), np.float32), 3) == CL_DEVICE_NOT_FOUND
    assert p.fade_ir_device(torch.zeros((O, I, cvs)), 3, stream=0) == CL_DEVICE_NOT_FOUND
    # a failed object answers with its error, whatever the fade length
    assert p.fade_ir(np.zeros((O, I, cvs), np.float32), 0) == CL_DEVICE_NOT_FOUND
    assert p.fade_ir_device(torch.zeros((O, I, cvs)), -1, stream=0) == CL_DEVICE_NOT_FOUND
    assert p.fade_remaining() == 0
    # the row checks of the Python layer come first, as the plain pushes'
    assert p.fade_ir(np.zeros((I, O, cvs), np.float32), 3) == CL_INVALID_VALUE
    assert p.fade_ir(np.zeros((O * I, cvs), np.float32), 3) == CL_INVALID_VALUE
    assert p.fade_ir_device(torch.zeros((I, O, cvs)), 3, stream=0) == CL_INVALID_VALUE
    assert p.fade_ir_device(torch.zeros((O, I, cvs))[:, :, ::2], 3, stream=0) == CL_INVALID_VALUE
    assert p.push_ir(np.zeros((I, O, cvs), np.float32)) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.fade_ir(np.array([["a"]]), 3)              # (what numpy says of rows that are no numbers)


def _cvs(pts1, n1):
    return 2 * pts1 + n1 * pts1 + 3   # a remainder, dropped


def _segments(pts0, pts1, n1, I):
    return ((1, 1), (_cutting(I, 2 * pts1 // pts0), _cutting(I, n1)))


@functools.lru_cache(maxsize=None)
def _case(pts0, pts1, n1, I, O, segs):
    """(hA, hB, hC, x, yA, yB, yC): responses, a signal long enough for every case of the grid, and what the definition
    gives for the objects that always held A, B, C; read-only"""
    m = pts1 // pts0
    cvs = _cvs(pts1, n1)
    nblocks = (n1 + 4) * m + (m - 1) + (2 * m + 3) + (n1 + 4) * m   # the latest push, the longest fade, n1 + 4 periods
    rng = np.random.default_rng(1000 * pts0 + pts1 + n1 + 7 * I + O)
    hs = [rng.random((O, I, cvs)) - 0.5 for _ in range(3)]
    x = rng.random((I, nblocks * pts0)) - 0.5
    out = hs + [x] + [definition(h, x, cvs, pts0, pts1, segs) for h in hs]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _fade(geom, I, O, segs, c, fade, nblocks, extra=2, hB=None):
    """the model pushed at position c: its output over nblocks blocks, fade_remaining() checked block by block"""
    pts0, pts1, n1 = geom
    hA, hB_, _, x, _, _, _ = _case(pts0, pts1, n1, I, O, segs)
    model = NupMatrixFadeModel(_cvs(pts1, n1), pts0, pts1, I, O, segs, extra=extra)
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


def _check_grid(geom, I, O):
    pts0, pts1, n1 = geom
    m = pts1 // pts0
    for segs in _segments(pts0, pts1, n1, I):
        _, _, _, x, yA, yB, _ = _case(pts0, pts1, n1, I, O, segs)
        peak = np.max(np.abs(yA))
        for P, s, fade in _grid(pts0, pts1, n1):
            c = P * m + s
            nblocks = c + fade + (n1 + 4) * m       # n1 + 4 periods past the fade's end: a wrong exchange shows
            assert nblocks * pts0 <= x.shape[1]
            L = nblocks * pts0
            want = mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
            got = _fade(geom, I, O, segs, c, fade, nblocks)
            err = np.max(np.abs(got - want)) / peak
            assert err < 1e-12, (segs, "P %d s %d fade %d" % (P, s, fade), err)
            # the fade is audible: the two ends differ after it
            after = (c + fade) * pts0
            assert np.max(np.abs(yA[:, after:L] - yB[:, after:L])) > 1e-3 * peak


@pytest.mark.parametrize("geom", GEOMS)
def test_model_matches_the_definition(geom):
    _check_grid(geom, 2, 3)


def test_model_matches_the_definition_three_inputs_one_output():
    _check_grid(GEOMS[0], 3, 1)


def test_a_ring_of_n1_plus_1_frames_is_too_short():
    """at phase s > 0 of period P tail block P - 3 reads input block P - 2 - n1, which a ring of n1 + 1 frames has lost"""
    geom, I, O = (4, 8, 1), 2, 3
    pts0, pts1, n1 = geom
    m, P, s, fade = 2, 3, 1, 3
    for segs in _segments(pts0, pts1, n1, I):
        _, _, _, _, yA, yB, _ = _case(pts0, pts1, n1, I, O, segs)
        c = P * m + s
        nblocks = c + fade + (n1 + 4) * m
        L = nblocks * pts0
        want = mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        peak = np.max(np.abs(yA))
        assert np.max(np.abs(_fade(geom, I, O, segs, c, fade, nblocks, extra=1) - want)) > 1e-3 * peak
        assert np.max(np.abs(_fade(geom, I, O, segs, c, fade, nblocks, extra=2) - want)) < 1e-12 * peak


@pytest.mark.parametrize("geom", GEOMS)
def test_a_fade_from_a_to_a_is_no_push(geom):
    pts0, pts1, n1 = geom
    m, I, O = pts1 // pts0, 2, 3
    segs = _segments(pts0, pts1, n1, I)[1]
    hA, _, _, _, yA, _, _ = _case(pts0, pts1, n1, I, O, segs)
    peak = np.max(np.abs(yA))
    for c, fade in ((0, 1), (1, m + 1), (2 * m + m - 1, 2 * m + 3), ((n1 + 3) * m + 1, m + 1)):
        nblocks = c + fade + (n1 + 4) * m
        got = _fade(geom, I, O, segs, c, fade, nblocks, hB=hA)
        assert np.max(np.abs(got - yA[:, :nblocks * pts0])) < 1e-12 * peak, (c, fade)


def test_a_second_fade_gives_b_then_c():
    pts0, pts1, n1, I, O = 4, 16, 3, 2, 3
    m = pts1 // pts0
    segs = _segments(pts0, pts1, n1, I)[1]
    hA, hB, hC, x, yA, yB, yC = _case(pts0, pts1, n1, I, O, segs)
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                          # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    model = NupMatrixFadeModel(_cvs(pts1, n1), pts0, pts1, I, O, segs)
    model.push_ir(hA)
    out = [model.process(x[:, :c1 * pts0])]
    model.push_ir_fade(hB, f1)
    with pytest.raises(AssertionError):
        model.push_ir_fade(hC, f2)                # one fade at a time
    with pytest.raises(AssertionError):
        model.push_ir(hC)
    out.append(model.process(x[:, c1 * pts0:c2 * pts0]))
    assert model.fade_remaining() == 0
    model.push_ir_fade(hC, f2)
    out.append(model.process(x[:, c2 * pts0:L]))
    got = np.concatenate(out, axis=1)
    want = mixed(mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    peak = np.max(np.abs(yA))
    assert np.max(np.abs(got - want)) < 1e-12 * peak
    assert np.max(np.abs(yB[:, (c2 + f2) * pts0:L] - yC[:, (c2 + f2) * pts0:L])) > 1e-3 * peak
