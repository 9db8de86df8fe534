"""Timed crossfade of the convolution matrix without a GPU: the ABI symbols and their answers on a NULL handle, and the
float64 model of the fade (tests/pconv_fade_model.py: shared ring, second tails primed from the ring, the cut at the fade's
end, the copy-over) checked against the definition, two models fed alike and mixed by g."""
import ctypes as C

import numpy as np
import pytest

from opencl_fft_amd._lib import lib
from tests.pconv_fade_model import FadeModel, definition
from tests.pconv_matrix_model import MatrixModel

CL_INVALID_VALUE = -30


def test_symbols_and_null_handle():
    L = lib()
    for name in ("clfa_pconv_matrix_push_ir_fade", "clfa_pconv_matrix_push_ir_fade_dev", "clfa_pconv_matrix_fade_remaining"):
        assert hasattr(L, name), name
    rows = np.zeros(64, np.float32)
    assert L.clfa_pconv_matrix_push_ir_fade(None, rows.ctypes.data, C.c_long(1)) == CL_INVALID_VALUE
    assert L.clfa_pconv_matrix_push_ir_fade_dev(None, rows.ctypes.data, C.c_long(64), C.c_long(1), None) == CL_INVALID_VALUE
    assert L.clfa_pconv_matrix_fade_remaining(None) == 0


def _run(nparts, cap, segs, inputs, outputs, t_push, fade_blocks, splits, pts=16):
    rng = np.random.default_rng(nparts * 1000 + cap * 100 + segs * 10 + fade_blocks)
    ha = rng.random((outputs, inputs, nparts * pts)) - 0.5
    hb = rng.random((outputs, inputs, nparts * pts)) - 0.5
    n = t_push + sum(splits)
    x = rng.random((inputs, n * pts)) - 0.5
    m = FadeModel(nparts, pts, inputs, outputs, cap, segs)
    m.push_ir(ha)
    got = [m.process(x[:, :t_push * pts])]
    m.push_ir_fade(hb, fade_blocks)
    assert m.fade_remaining() == fade_blocks
    j = t_push
    for k in splits:
        got.append(m.process(x[:, j * pts:(j + k) * pts]))
        j += k
        assert m.fade_remaining() == max(0, fade_blocks - (j - t_push))
    got = np.concatenate(got, axis=1)
    want = definition(ha, hb, x, t_push, fade_blocks, pts, nparts)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-12, err
    return m, hb, x


@pytest.mark.parametrize("cap", [1, 3, 100])
@pytest.mark.parametrize("segs", [1, 3])
@pytest.mark.parametrize("nparts,fade_blocks", [(1, 1), (1, 4), (5, 1), (5, 4), (5, 8), (3, 11)])
def test_model_matches_the_definition(cap, segs, nparts, fade_blocks):
    """pushes after 7 blocks (the ring has wrapped); the second call starts inside the fade (for fade_blocks > 2) and ends
    after it; fades of nparts + 3 and more blocks outlast the ring"""
    _run(nparts, cap, segs, 3, 2, 7, fade_blocks, [2, fade_blocks + 3])


def test_fade_from_the_first_block_and_one_input():
    _run(4, 3, 2, 1, 1, 0, 6, [1, 4, 5])


def test_after_the_fade_the_state_is_that_of_the_new_responses():
    """a fade that ends mid-call leaves exactly the object that held B all along (a further call agrees with it), and a
    second fade may follow"""
    pts, nparts = 16, 5
    m, hb, x = _run(nparts, 3, 3, 3, 2, 7, 4, [3, 6])
    ref = MatrixModel(nparts, pts, 3, 2, cap=100, segs=3)
    ref.push_ir(hb)
    ref.process(x)
    more = np.random.default_rng(9).random((3, 6 * pts)) - 0.5
    assert np.max(np.abs(m.process(more) - ref.process(more))) < 1e-12
    m.push_ir_fade(hb, 2)
    assert m.fade_remaining() == 2


def test_fade_to_the_same_responses_changes_nothing():
    pts, nparts = 16, 5
    rng = np.random.default_rng(4)
    h = rng.random((2, 3, nparts * pts)) - 0.5
    x = rng.random((3, 20 * pts)) - 0.5
    a, b = FadeModel(nparts, pts, 3, 2, 3, 3), MatrixModel(nparts, pts, 3, 2, 3, 3)
    a.push_ir(h)
    b.push_ir(h)
    ya = [a.process(x[:, :7 * pts])]
    a.push_ir_fade(h, 8)
    ya.append(a.process(x[:, 7 * pts:]))
    assert np.max(np.abs(np.concatenate(ya, axis=1) - b.process(x))) < 1e-13


def test_model_refusals():
    m = FadeModel(3, 16, 1, 1, 2)
    h = np.zeros((1, 1, 48))
    with pytest.raises(ValueError):
        m.push_ir_fade(h, 0)
    m.push_ir_fade(h, 2)
    with pytest.raises(RuntimeError):
        m.push_ir_fade(h, 2)
    with pytest.raises(RuntimeError):
        m.push_ir(h)
