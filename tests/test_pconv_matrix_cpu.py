"""Convolution matrix without a GPU: the new ABI symbols, the Python surface's answers without a device, and the float64
model of the sub-batch algebra of pconv_matrix.hip checked against the definition, sum_i pconv_f64(h_{o,i}, x_i)."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import util
from tests.pconv_matrix_model import MatrixModel, seg_bounds, truth_with_push

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
NAMES = ["clfa_pconv_matrix_create", "clfa_pconv_matrix_destroy", "clfa_pconv_matrix_get_error",
         "clfa_pconv_matrix_get_log", "clfa_pconv_matrix_push_ir", "clfa_pconv_matrix_push_ir_dev",
         "clfa_pconv_matrix_process_dev", "clfa_pconv_matrix_convolution", "clfa_pconv_matrix_nparts",
         "clfa_pconv_matrix_state_bytes", "clfa_pconv_matrix_workspace_bytes", "clfa_pconv_matrix_kernel_name"]


@pytest.mark.parametrize("name", NAMES)
def test_symbol_exported(name):
    assert hasattr(lib(), name)


def test_methods_without_a_device():
    if fa.device_count() > 0:
        pytest.skip("a device is present (tests/test_gpu_pconv_matrix.py)")
    m = fa.PconvMatrix(0, 4 * 64, 64, 3, 2)
    assert m.get_error() == CL_DEVICE_NOT_FOUND
    assert m.nparts == 0 and m.state_bytes() == 0 and m.workspace_bytes() == 0 and m.kernel_name() == ""
    assert m.push_ir(np.zeros((2, 3, 4 * 64), np.float32)) == CL_DEVICE_NOT_FOUND
    x = np.zeros((3, 5 * 64), np.float32)
    assert m.convolution(np.zeros((2, 5 * 64), np.float32), x) == CL_DEVICE_NOT_FOUND
    import torch
    assert m.process_device(torch.zeros((2, 5 * 64)), torch.zeros((3, 5 * 64)), stream=0) == CL_DEVICE_NOT_FOUND


@pytest.mark.parametrize("pts", [16, 8192, 48])
def test_bad_partition_sizes_fail_before_the_device(pts):
    m = fa.PconvMatrix(0, 4 * pts, pts, 2, 2)
    assert m.get_error() == CL_INVALID_VALUE
    assert "pts" in m.get_log()


def test_segment_bounds_cover_the_sequence():
    for total in (1, 3, 16, 94 * 16, 1000):
        for segs in (1, 2, 7, 64):
            b = seg_bounds(total, segs)
            assert b[0][0] == 0 and b[-1][1] == total
            assert all(b[k][1] == b[k + 1][0] for k in range(segs - 1))


def _truth(ir, x, pts):
    O, I = ir.shape[:2]
    return np.stack([sum(util.pconv_f64(ir[o, i].astype(np.float64), x[i].astype(np.float64), pts) for i in range(I))
                     for o in range(O)])


@pytest.mark.parametrize("inputs,outputs", [(1, 1), (3, 2), (2, 3)])
@pytest.mark.parametrize("nparts,cap,segs", [(1, 1, 1), (3, 1, 2), (3, 2, 1), (4, 5, 3), (5, 3, 7), (7, 100, 4)])
def test_sub_batch_algebra_matches_the_definition(inputs, outputs, nparts, cap, segs):
    pts = 16
    rng = np.random.default_rng(nparts * 100 + cap * 10 + segs + inputs)
    ir = rng.random((outputs, inputs, nparts * pts), dtype=np.float32) - 0.5
    m = MatrixModel(nparts, pts, inputs, outputs, cap, segs)
    m.push_ir(ir)
    splits = [1, nparts + 2, 2 * nparts + 3, nparts, 4]   # more blocks than nparts: the rings wrap
    x = rng.random((inputs, sum(splits) * pts), dtype=np.float32) - 0.5
    got, j = [], 0
    for n in splits:
        got.append(m.process(x[:, j * pts:(j + n) * pts]))
        j += n
    got = np.concatenate(got, axis=1)
    want = _truth(ir, x, pts)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-12, err
    assert m.wp == sum(splits) % nparts


def test_push_between_calls_applies_from_the_next_block():
    pts, nparts, I, O = 16, 3, 2, 3
    rng = np.random.default_rng(3)
    h1 = rng.random((O, I, nparts * pts), dtype=np.float32) - 0.5
    h2 = rng.random((O, I, nparts * pts), dtype=np.float32) - 0.5
    x = rng.random((I, 11 * pts), dtype=np.float32) - 0.5
    m = MatrixModel(nparts, pts, I, O, cap=4, segs=2)
    m.push_ir(h1)
    a = m.process(x[:, :5 * pts])
    m.push_ir(h2)
    b = m.process(x[:, 5 * pts:])
    want = truth_with_push(h1, h2, 5, x, pts)
    assert np.max(np.abs(np.concatenate([a, b], axis=1) - want)) < 1e-12 * np.max(np.abs(want))
    assert np.allclose(truth_with_push(h1, h1, 5, x, pts), _truth(h1, x, pts), rtol=0, atol=1e-12)
