"""Nupconv's timed crossfade of response changes without a GPU: the new ABI symbols, the Python surface's answers without
a device, and the float64 model of the schedule (tests/nupconv_model.py: a tail ring of n1 + 2 frames, the second
path primed from the rings alone, the sets exchanged at the end) against the definition, two objects fed alike and mixed
by g, at every push position and fade length that takes another way through the priming."""
import functools

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import nupconv_cases as nc
from tests.nupconv_model import NupFadeModel, plain

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
GEOMS = nc.MODEL_GEOMS   # pts0, pts1, n1


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


@functools.lru_cache(maxsize=None)
def _case(pts0, pts1, n1):
    """(hA, hB, hC, x, yA, yB, yC): responses, a signal long enough for every case of the grid, and what the objects that
    always held A, B, C return for it; read-only"""
    m, channels = pts1 // pts0, 2
    cvs = nc.cvs(pts1, n1, 3)
    rng = np.random.default_rng(1000 * pts0 + pts1 + n1)
    hs = [rng.random((channels, cvs)) - 0.5 for _ in range(3)]
    x = rng.random((channels, nc.model_blocks(m, n1) * pts0)) - 0.5
    out = hs + [x] + [plain(h, x, cvs, pts0, pts1) for h in hs]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _new(pts0, pts1, n1):
    return functools.partial(NupFadeModel, nc.cvs(pts1, n1, 3), pts0, pts1, 2)


def test_the_grid_has_216_cases():
    assert sum(len(nc.model_grid(*g)) for g in GEOMS) == 216


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_model_matches_the_definition(pts0, pts1, n1):
    nc.check_model_grid(_new(pts0, pts1, n1), _case(pts0, pts1, n1), (pts0, pts1, n1))


def test_a_ring_of_n1_plus_1_frames_is_too_short():
    nc.check_a_short_ring(_new(4, 8, 1), _case(4, 8, 1))


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_a_fade_from_a_to_a_is_no_push(pts0, pts1, n1):
    nc.check_a_to_a(_new(pts0, pts1, n1), _case(pts0, pts1, n1), (pts0, pts1, n1))


def test_a_second_fade_gives_b_then_c():
    nc.check_a_second_fade(_new(4, 16, 3), _case(4, 16, 3), (4, 16, 3))
