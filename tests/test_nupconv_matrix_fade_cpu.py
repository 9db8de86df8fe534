"""NupconvMatrix's timed crossfade of response changes without a GPU: the new ABI symbols, the Python surface's answers
without a device, and the float64 model of the schedule (tests/nupconv_model.py: a tail ring of n1 + 2 frames
per input, the second set primed from the rings alone, the sets exchanged at the end, segments included) against the
definition — `mixed` of two tests.nupconv_definitions.matrix_definition results, two objects fed alike — at every push position
and fade length that takes another way through the priming."""
import functools

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import nupconv_cases as nc
from tests.nupconv_definitions import matrix_definition
from tests.nupconv_model import NupMatrixFadeModel

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
GEOMS = nc.MODEL_GEOMS   # pts0, pts1, n1
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


def _segments(pts0, pts1, n1, I):
    return ((1, 1), (nc.cutting(I, 2 * pts1 // pts0), nc.cutting(I, n1)))


@functools.lru_cache(maxsize=None)
def _case(pts0, pts1, n1, I, O, segs):
    """(hA, hB, hC, x, yA, yB, yC): responses, a signal long enough for every case of the grid, and what the definition
    gives for the objects that always held A, B, C; read-only"""
    m = pts1 // pts0
    cvs = nc.cvs(pts1, n1, 3)
    rng = np.random.default_rng(1000 * pts0 + pts1 + n1 + 7 * I + O)
    hs = [rng.random((O, I, cvs)) - 0.5 for _ in range(3)]
    x = rng.random((I, nc.model_blocks(m, n1) * pts0)) - 0.5
    out = hs + [x] + [matrix_definition(h, x, cvs, pts0, pts1, segs) for h in hs]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _new(geom, I, O, segs):
    pts0, pts1, n1 = geom
    return functools.partial(NupMatrixFadeModel, nc.cvs(pts1, n1, 3), pts0, pts1, I, O, segs)


def _check_grid(geom, I, O):
    for segs in _segments(*geom, I):
        nc.check_model_grid(_new(geom, I, O, segs), _case(*geom, I, O, segs), geom, segs)


@pytest.mark.parametrize("geom", GEOMS)
def test_model_matches_the_definition(geom):
    _check_grid(geom, 2, 3)


def test_model_matches_the_definition_three_inputs_one_output():
    _check_grid(GEOMS[0], 3, 1)


def test_a_ring_of_n1_plus_1_frames_is_too_short():
    geom, I, O = (4, 8, 1), 2, 3
    for segs in _segments(*geom, I):
        nc.check_a_short_ring(_new(geom, I, O, segs), _case(*geom, I, O, segs))


@pytest.mark.parametrize("geom", GEOMS)
def test_a_fade_from_a_to_a_is_no_push(geom):
    I, O = 2, 3
    segs = _segments(*geom, I)[1]
    nc.check_a_to_a(_new(geom, I, O, segs), _case(*geom, I, O, segs), geom)


def test_a_second_fade_gives_b_then_c():
    geom, I, O = (4, 16, 3), 2, 3
    segs = _segments(*geom, I)[1]
    nc.check_a_second_fade(_new(geom, I, O, segs), _case(*geom, I, O, segs), geom)
