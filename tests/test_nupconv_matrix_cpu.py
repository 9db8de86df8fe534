"""Non-uniformly partitioned convolution matrix without a GPU: the new ABI symbols, the Python surface's answers without a
device, the refusals of create before the device is looked for, and the float64 model of the schedule, segments included
(tests/nupconv_model.py), checked against the definition: two MatrixModel objects, the tail delayed by 2 * pts1
(tests/nupconv_definitions.py).
Every model test also creates the library's object at the model's geometry (scaled to pts0 = 32)."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import nupconv_cases as nc
from tests.nupconv_definitions import definition as definition_1x1
from tests.nupconv_definitions import matrix_definition as definition
from tests.nupconv_model import NupMatrixModel

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
NAMES = ["clfa_nupconv_matrix_" + n for n in (
    "create", "destroy", "get_error", "get_log", "nparts", "segments", "position", "state_bytes", "workspace_bytes",
    "kernel_name", "push_ir", "push_ir_dev", "process_dev", "convolution", "reset")]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported_and_bound(name):
    assert hasattr(lib(), name)
    assert name in {s[0] for s in fa._lib.SYMBOLS}


def test_python_surface():
    assert "NupconvMatrix" in fa.__all__
    for name in ("push_ir", "push_ir_device", "convolution", "process_device", "reset", "position", "nparts", "segments",
                 "state_bytes", "workspace_bytes", "kernel_name", "get_error", "get_log"):
        assert hasattr(fa.NupconvMatrix, name), name
    assert not hasattr(fa.NupconvMatrix, "push_ir_fade")   # the timed crossfade is not part of this object


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_nupconv_matrix.py)")
    import torch
    cvs, pts0, pts1, I, O = 5 * 256 + 7, 64, 256, 3, 2
    p = fa.NupconvMatrix(0, cvs, pts0, pts1, I, O)
    assert p.get_error() == CL_DEVICE_NOT_FOUND and p.get_log() == ""
    assert p.nparts(0) == 0 and p.nparts(1) == 0 and p.nparts(2) == 0 and p.position == 0
    assert p.segments(0) == 0 and p.segments(1) == 0 and p.segments(2) == 0
    assert p.state_bytes() == 0 and p.workspace_bytes() == 0 and p.kernel_name() == ""
    assert p.push_ir(np.zeros((O, I, cvs), np.float32)) == CL_DEVICE_NOT_FOUND
    assert p.push_ir_device(torch.zeros((O, I, cvs)), stream=0) == CL_DEVICE_NOT_FOUND
    x = np.zeros((I, 3 * pts0), np.float32)
    assert p.convolution(np.zeros((O, 3 * pts0), np.float32), x) == CL_DEVICE_NOT_FOUND
    assert p.process_device(torch.zeros((O, 3 * pts0)), torch.zeros((I, 3 * pts0)), stream=0) == CL_DEVICE_NOT_FOUND
    assert p.reset(stream=0) == CL_DEVICE_NOT_FOUND
    # the shape checks of the Python layer come first
    assert p.convolution(np.zeros((O, 3 * pts0 + 1), np.float32), np.zeros((I, 3 * pts0 + 1), np.float32)) == CL_INVALID_VALUE
    assert p.convolution(np.zeros((I, 3 * pts0), np.float32), x) == CL_INVALID_VALUE
    assert p.process_device(torch.zeros((O, 2 * pts0)), torch.zeros((I, 3 * pts0)), stream=0) == CL_INVALID_VALUE
    assert p.process_device(torch.zeros((O, pts0 + 1)), torch.zeros((I, pts0 + 1)), stream=0) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.process_device(torch.zeros((O + 1, pts0)), torch.zeros((I, pts0)), stream=0)
    with pytest.raises(ValueError):
        p.process_device(torch.zeros((O, pts0)), torch.zeros((I + 1, pts0)), stream=0)
    assert p.push_ir(np.zeros((I, O, cvs), np.float32)) == CL_INVALID_VALUE
    assert p.push_ir_device(torch.zeros((I, O, cvs)), stream=0) == CL_INVALID_VALUE


@pytest.mark.parametrize("cvs,pts0,pts1,inputs,outputs,named", [
    (4096, 64, 64, 2, 2, "pts1"),          # pts1 <= pts0
    (4096, 128, 64, 2, 2, "pts1"),
    (4096, 48, 256, 2, 2, "pts0"),         # not a power of two
    (4096, 64, 384, 2, 2, "pts1"),
    (4096, 16, 256, 2, 2, "pts0"),         # below the blocks kernels' range
    (3 * 8192, 64, 8192, 2, 2, "pts1"),    # above it
    (3 * 256 - 1, 64, 256, 2, 2, "cvs"),   # no tail partition
    (4096, 64, 256, 0, 2, "inputs"),
    (4096, 64, 256, 2, 0, "outputs"),
    (4096, 64, 256, -1, 2, "inputs"),
])
def test_bad_geometries_fail_before_the_device(cvs, pts0, pts1, inputs, outputs, named):
    p = fa.NupconvMatrix(0, cvs, pts0, pts1, inputs, outputs)
    assert p.get_error() == CL_INVALID_VALUE
    assert named in p.get_log(), p.get_log()
    assert p.nparts(0) == 0 and p.segments(0) == 0 and p.kernel_name() == ""


def test_smallest_good_geometry_reaches_the_device_lookup():
    p = fa.NupconvMatrix(0, 3 * 64, 32, 64, 1, 1)
    assert p.get_error() in (0, CL_DEVICE_NOT_FOUND) and p.get_log() == ""


def _streams(rng, cvs, nblocks, pts0, I, O):
    h = rng.random((O, I, cvs)) - 0.5
    x = rng.random((I, nblocks * pts0)) - 0.5
    return h, x


def _library_twin(model, cvs):
    """the library's object at the model's geometry scaled to its smallest partition (pts0 -> 32): it reaches the device
    lookup, and where a device answers it has the model's partitions on both levels"""
    k = 32 // model.pts0
    p = fa.NupconvMatrix(0, cvs * k, model.pts0 * k, model.pts1 * k, model.rows_in, model.rows_out)
    assert p.get_error() in (0, CL_DEVICE_NOT_FOUND) and p.get_log() == ""
    if p.get_error() == 0:
        assert (p.nparts(0), p.nparts(1)) == (model.n0, model.n1)


@pytest.mark.parametrize("I,O", [(2, 3), (3, 1)])
@pytest.mark.parametrize("pts0,pts1,n1", nc.MODEL_GEOMS)
def test_schedule_matches_the_definition(pts0, pts1, n1, I, O):
    m = pts1 // pts0
    cvs = nc.cvs(pts1, n1, 3)
    nblocks = (n1 + 5) * m + 3                # past the whole response, ending inside a period
    rng = np.random.default_rng(pts0 * 100 + pts1 + n1 + 7 * I + O)
    h, x = _streams(rng, cvs, nblocks, pts0, I, O)
    # the definition in the words of util.pconv_f64 as well: the segments change no float64 sum beyond rounding
    sums = np.stack([sum(definition_1x1(h[o, i], x[i], cvs, pts0, pts1) for i in range(I)) for o in range(O)])
    head = [1, m + 2, 2, 0, 2 * m + 1]        # odd calls that cross period boundaries, and an empty one
    for segs in ((1, 1), (nc.cutting(I, 2 * m), nc.cutting(I, n1))):
        want = definition(h, x, cvs, pts0, pts1, segs)
        peak = np.max(np.abs(want))
        assert np.max(np.abs(want - sums)) < 1e-12 * peak
        for splits in ([nblocks], [1] * nblocks, head + [nblocks - sum(head)]):
            model = NupMatrixModel(cvs, pts0, pts1, I, O, segs)
            assert (model.n0, model.n1) == (2 * m, n1)
            _library_twin(model, cvs)
            model.push_ir(h)
            got = nc.model_calls(model, x, splits)
            err = np.max(np.abs(got - want)) / peak
            assert err < 1e-12, (segs, splits[:6], err)
    # the tail is silent for 2 * pts1 samples and present after them
    h0 = h.copy()
    h0[:, :, 2 * pts1:] = 0
    head_only = definition(h0, x, cvs, pts0, pts1)
    assert np.array_equal(head_only[:, :2 * pts1], definition(h, x, cvs, pts0, pts1)[:, :2 * pts1])
    assert np.max(np.abs(want[:, 2 * pts1:] - head_only[:, 2 * pts1:])) > 1e-3 * peak


def test_reset_repeats_the_first_output():
    pts0, pts1, cvs, I, O = 4, 16, 5 * 16, 2, 3
    rng = np.random.default_rng(9)
    h, x = _streams(rng, cvs, 23, pts0, I, O)
    model = NupMatrixModel(cvs, pts0, pts1, I, O, (3, 2))
    _library_twin(model, cvs)
    model.push_ir(h)
    first = model.process(x)
    model.reset()
    assert model.position == 0
    assert np.array_equal(model.process(x), first)


@pytest.mark.parametrize("period", [1, 3])
def test_push_at_phase_0_equals_the_push_on_both_levels(period):
    """A push at position c = period * m: the head object pushed before its block c, the tail object before its block
    period - 1 — the tail block whose multiply-accumulate begins at c (block 0 for a push in the first period)"""
    pts0, pts1, n1, I, O = 4, 16, 3, 2, 3
    m, cvs = pts1 // pts0, 2 * pts1 + n1 * pts1
    nblocks = (period + n1 + 4) * m
    rng = np.random.default_rng(period)
    h1, x = _streams(rng, cvs, nblocks, pts0, I, O)
    h2 = rng.random(h1.shape) - 0.5
    segs = (3, 2)
    model = NupMatrixModel(cvs, pts0, pts1, I, O, segs)
    _library_twin(model, cvs)
    model.push_ir(h1)
    c = period * m
    a = model.process(x[:, :c * pts0])
    assert model.position % m == 0
    model.push_ir(h2)
    got = np.concatenate([a, model.process(x[:, c * pts0:])], axis=1)
    want = definition(h1, x, cvs, pts0, pts1, segs, push=(h2, c, period - 1))
    assert np.max(np.abs(got - want)) < 1e-12 * np.max(np.abs(want))
    # and the push is audible: the old responses alone give something else
    assert np.max(np.abs(want - definition(h1, x, cvs, pts0, pts1, segs))) > 1e-3 * np.max(np.abs(want))
