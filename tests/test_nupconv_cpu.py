"""Non-uniformly partitioned convolution without a GPU: the new ABI symbols, the Python surface's answers without a
device, the refusals of create before the device is looked for, and the float64 model of the schedule
(tests/nupconv_model.py) checked against the definition built from tests/util.pconv_f64
(tests/nupconv_definitions.py)."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import nupconv_cases as nc
from tests.nupconv_definitions import definition, delayed_tail
from tests.nupconv_model import NupModel
from tests.pconv_matrix_model import truth_with_push

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
NAMES = ["clfa_nupconv_create", "clfa_nupconv_destroy", "clfa_nupconv_get_error", "clfa_nupconv_get_log",
         "clfa_nupconv_nparts", "clfa_nupconv_position", "clfa_nupconv_state_bytes", "clfa_nupconv_workspace_bytes",
         "clfa_nupconv_kernel_name", "clfa_nupconv_push_ir", "clfa_nupconv_push_ir_dev", "clfa_nupconv_process_dev",
         "clfa_nupconv_convolution", "clfa_nupconv_reset"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    assert hasattr(lib(), name)


def test_python_surface():
    assert "Nupconv" in fa.__all__
    for name in ("push_ir", "push_ir_device", "convolution", "process_device", "reset", "position", "nparts",
                 "state_bytes", "workspace_bytes", "kernel_name", "get_error", "get_log"):
        assert hasattr(fa.Nupconv, name), name


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_nupconv.py)")
    import torch
    cvs, pts0, pts1 = 5 * 256 + 7, 64, 256
    p = fa.Nupconv(0, cvs, pts0, pts1, channels=2)
    assert p.get_error() == CL_DEVICE_NOT_FOUND and p.get_log() == ""
    assert p.nparts(0) == 0 and p.nparts(1) == 0 and p.nparts(2) == 0 and p.position == 0
    assert p.state_bytes() == 0 and p.workspace_bytes() == 0 and p.kernel_name() == ""
    assert p.push_ir(np.zeros((2, cvs), np.float32)) == CL_DEVICE_NOT_FOUND
    assert p.push_ir_device(torch.zeros((2, cvs)), stream=0) == CL_DEVICE_NOT_FOUND
    x = np.zeros((2, 3 * pts0), np.float32)
    assert p.convolution(np.zeros_like(x), x) == CL_DEVICE_NOT_FOUND
    assert p.process_device(torch.zeros((2, 3 * pts0)), torch.zeros((2, 3 * pts0)), stream=0) == CL_DEVICE_NOT_FOUND
    assert p.reset(stream=0) == CL_DEVICE_NOT_FOUND
    # the shape checks of the Python layer come first
    assert p.convolution(np.zeros((2, 3 * pts0 + 1), np.float32), np.zeros((2, 3 * pts0 + 1), np.float32)) == CL_INVALID_VALUE
    assert p.process_device(torch.zeros((2, 2 * pts0)), torch.zeros((2, 3 * pts0)), stream=0) == CL_INVALID_VALUE
    assert p.process_device(torch.zeros((2, pts0 + 1)), torch.zeros((2, pts0 + 1)), stream=0) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.process_device(torch.zeros((3, pts0)), torch.zeros((3, pts0)), stream=0)
    assert p.push_ir(np.zeros((3, cvs), np.float32)) == CL_INVALID_VALUE


@pytest.mark.parametrize("cvs,pts0,pts1,channels,named", [
    (4096, 64, 64, 1, "pts1"),          # pts1 <= pts0
    (4096, 128, 64, 1, "pts1"),
    (4096, 48, 256, 1, "pts0"),         # not a power of two
    (4096, 64, 384, 1, "pts1"),
    (4096, 16, 256, 1, "pts0"),         # below the blocks kernels' range
    (3 * 8192, 64, 8192, 1, "pts1"),    # above it
    (3 * 256 - 1, 64, 256, 1, "cvs"),   # no tail partition
    (4096, 64, 256, 0, "channels"),
])
def test_bad_geometries_fail_before_the_device(cvs, pts0, pts1, channels, named):
    p = fa.Nupconv(0, cvs, pts0, pts1, channels=channels)
    assert p.get_error() == CL_INVALID_VALUE
    assert named in p.get_log(), p.get_log()
    assert p.nparts(0) == 0 and p.kernel_name() == ""


def test_smallest_good_geometry_reaches_the_device_lookup():
    p = fa.Nupconv(0, 3 * 64, 32, 64)
    assert p.get_error() in (0, CL_DEVICE_NOT_FOUND) and p.get_log() == ""


def _streams(rng, cvs, nblocks, pts0, channels):
    h = rng.random((channels, cvs)) - 0.5
    x = rng.random((channels, nblocks * pts0)) - 0.5
    return h, x


@pytest.mark.parametrize("pts0,pts1,n1", nc.MODEL_GEOMS)
def test_schedule_matches_the_definition(pts0, pts1, n1):
    m, channels = pts1 // pts0, 2
    cvs = nc.cvs(pts1, n1, 3)
    nblocks = (n1 + 5) * m + 3                # past the whole response, ending inside a period
    rng = np.random.default_rng(pts0 * 100 + pts1 + n1)
    h, x = _streams(rng, cvs, nblocks, pts0, channels)
    want = np.stack([definition(h[c], x[c], cvs, pts0, pts1) for c in range(channels)])
    peak = np.max(np.abs(want))
    head = [1, m + 2, 2, 0, 2 * m + 1]        # odd calls that cross period boundaries, and an empty one
    for splits in ([nblocks], [1] * nblocks, head + [nblocks - sum(head)]):
        model = NupModel(cvs, pts0, pts1, channels)
        assert (model.n0, model.n1) == (2 * m, n1)
        model.push_ir(h)
        got = nc.model_calls(model, x, splits)
        err = np.max(np.abs(got - want)) / peak
        assert err < 1e-12, (splits[:6], err)
    # the tail is silent for 2 * pts1 samples and present after them
    assert np.max(np.abs(want[:, 2 * pts1:] - np.stack([definition(np.r_[h[c, :2 * pts1], 0 * h[c, 2 * pts1:]], x[c], cvs, pts0, pts1)
                                                        for c in range(channels)])[:, 2 * pts1:])) > 1e-3 * peak


def test_reset_repeats_the_first_output():
    pts0, pts1, cvs = 4, 16, 5 * 16
    rng = np.random.default_rng(9)
    h, x = _streams(rng, cvs, 23, pts0, 1)
    model = NupModel(cvs, pts0, pts1)
    model.push_ir(h)
    first = model.process(x)
    model.reset()
    assert model.position == 0
    assert np.array_equal(model.process(x), first)


@pytest.mark.parametrize("period", [1, 3])
def test_push_at_phase_0_equals_the_push_on_both_levels(period):
    """A push at position c = period * m: the head object pushed before its block c, the tail object before its block
    period - 1 — the tail block whose multiply-accumulate begins at c (block 0 for a push in the first period)"""
    pts0, pts1, n1 = 4, 16, 3
    m, cvs = pts1 // pts0, 2 * pts1 + n1 * pts1
    nblocks = (period + n1 + 4) * m
    rng = np.random.default_rng(period)
    h1, x = _streams(rng, cvs, nblocks, pts0, 1)
    h2 = rng.random((1, cvs)) - 0.5
    model = NupModel(cvs, pts0, pts1)
    model.push_ir(h1)
    c = period * m
    a = model.process(x[:, :c * pts0])
    assert model.position % m == 0
    model.push_ir(h2)
    got = np.concatenate([a, model.process(x[:, c * pts0:])], axis=1)[0]
    yh = truth_with_push(h1[None, :, :2 * pts1], h2[None, :, :2 * pts1], c, x, pts0)[0]
    yt = truth_with_push(h1[None, :, 2 * pts1:], h2[None, :, 2 * pts1:], period - 1, x, pts1)[0]
    want = yh + delayed_tail(yt, pts1, x.shape[1])
    assert np.max(np.abs(got - want)) < 1e-12 * np.max(np.abs(want))
    # and the push is audible: the old responses alone give something else
    assert np.max(np.abs(want - definition(h1[0], x[0], cvs, pts0, pts1))) > 1e-3 * np.max(np.abs(want))
