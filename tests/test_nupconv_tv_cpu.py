"""Nupconv's time-varying second input without a GPU: the new ABI symbols with their bound types, the Python surface and
its refusals, and the float64 model (tests/nupconv_model.NupTvModel) against the three properties of the rule: the push
composition, static equivalence from head block R0 + 2m on, the closed-form impulse readout; cut-invariance and freeze."""
import ctypes as C
import functools

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import nupconv_cases as nc
from tests.nupconv_definitions import Composition, readout, readout_stream
from tests.nupconv_model import NupModel, NupTvModel

CL_DEVICE_NOT_FOUND, CL_INVALID_VALUE = -1, -30
GEOMS = nc.TV_MODEL_GEOMS   # pts0, pts1, n1
_vp = C.c_void_p


@pytest.mark.parametrize("name,restype,argtypes", [
    ("clfa_nupconv_process_tv_dev", C.c_int, [_vp, _vp, C.c_long, _vp, C.c_long, _vp, C.c_long, C.c_long, _vp]),
    ("clfa_nupconv_convolution_tv", C.c_int, [_vp, _vp, _vp, _vp, C.c_long]),
    ("clfa_nupconv_tv_period", C.c_long, [_vp]),
])
def test_symbol_exported_with_its_types(name, restype, argtypes):
    f = getattr(lib(), name)
    assert f.restype is restype and list(f.argtypes) == argtypes


def test_python_surface():
    for name in ("process_tv_device", "convolution_tv", "tv_period"):
        assert hasattr(fa.Nupconv, name), name
    assert isinstance(fa.Nupconv.tv_period, property)
    assert not hasattr(fa.NupconvMatrix, "process_tv_device")


def test_refusals_that_need_no_device():
    L = lib()
    assert L.clfa_nupconv_tv_period(None) == 0
    assert L.clfa_nupconv_process_tv_dev(None, None, 0, None, 0, None, 0, 1, None) == CL_INVALID_VALUE
    assert L.clfa_nupconv_convolution_tv(None, None, None, None, 1) == CL_INVALID_VALUE
    import torch
    cvs, pts0, pts1 = 5 * 256 + 7, 64, 256
    p = fa.Nupconv(0, cvs, pts0, pts1, channels=2)
    x = np.zeros((2, 3 * pts0), np.float32)
    # the Python layer's checks come before the object is asked: shapes, lengths that differ, a length off the block grid
    assert p.convolution_tv(np.zeros_like(x), x, x[:, :2 * pts0]) == CL_INVALID_VALUE
    assert p.convolution_tv(np.zeros_like(x), x[:, :pts0 + 1], x[:, :pts0 + 1]) == CL_INVALID_VALUE
    assert p.convolution_tv(np.zeros((3, 3 * pts0), np.float32), np.zeros((3, 3 * pts0), np.float32), x) == CL_INVALID_VALUE
    t = torch.zeros((2, 3 * pts0))
    assert p.process_tv_device(t.clone(), t, t[:, :2 * pts0], stream=0) == CL_INVALID_VALUE
    assert p.process_tv_device(t[:, :pts0 + 1].clone(), t[:, :pts0 + 1], t[:, :pts0 + 1], stream=0) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.process_tv_device(torch.zeros((3, pts0)), torch.zeros((3, pts0)), torch.zeros((3, pts0)), stream=0)
    if fa.device_count() == 0:   # a failed object answers with its error, and has no period
        assert p.get_error() == CL_DEVICE_NOT_FOUND and p.tv_period == 0
        assert p.convolution_tv(np.zeros_like(x), x, x) == CL_DEVICE_NOT_FOUND
        assert p.process_tv_device(t.clone(), t, t, stream=0) == CL_DEVICE_NOT_FOUND
    else:
        assert p.tv_period == ((cvs - 2 * pts1) // pts1 + 2) * (pts1 // pts0)


@functools.lru_cache(maxsize=None)
def _case(pts0, pts1, n1, channels=2):
    """(h, x, w): pushed responses, a signal and a second input of R0 + 3m + 3 head blocks, float32 values, read-only"""
    m = pts1 // pts0
    nblocks = (n1 + 2) * m + 3 * m + 3
    rng = np.random.default_rng(pts0 + pts1 + 10 * n1 + channels)
    out = (rng.random((channels, nc.cvs(pts1, n1)), dtype=np.float32) - 0.5,
           rng.random((channels, nblocks * pts0), dtype=np.float32) - 0.5,
           rng.random((channels, nblocks * pts0), dtype=np.float32) - 0.5)
    for a in out:
        a.setflags(write=False)
    return out


def _model(pts0, pts1, n1, channels, h=None):
    model = NupTvModel(nc.cvs(pts1, n1), pts0, pts1, channels)
    assert model.R0 == (n1 + 2) * (pts1 // pts0) and model.L == model.need()
    if h is not None:
        model.push_ir(h)
    return model


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_the_push_composition_exactly(pts0, pts1, n1):
    h, x, w = _case(pts0, pts1, n1)
    channels, nblocks, m = x.shape[0], x.shape[1] // pts0, pts1 // pts0
    for plain in ((), (3 * m + 1, nblocks - 2)):   # all time-varying; two blocks sent as plain ones
        comp = Composition(NupModel(nc.cvs(pts1, n1), pts0, pts1, channels), pts0, pts1, n1, channels, ir=h)
        comp.p.push_ir(h)
        want = comp.run(x, w, plain=plain)
        model = _model(pts0, pts1, n1, channels, h)
        got = nc.model_calls(model, x, [1] * nblocks, w, plain)
        assert np.array_equal(got, want), plain
    # the second input is heard: the object that keeps h returns something else
    still = _model(pts0, pts1, n1, channels, h).process(x)
    assert np.max(np.abs(still - want)) > 1e-3 * np.max(np.abs(want))


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_cut_invariance(pts0, pts1, n1):
    h, x, w = _case(pts0, pts1, n1)
    channels, nblocks, m = x.shape[0], x.shape[1] // pts0, pts1 // pts0
    want = nc.model_calls(_model(pts0, pts1, n1, channels, h), x, [nblocks], w)
    for splits in ([1] * nblocks, [1, m - 1, 0, 2 * m - m + 3, nblocks - 2 * m - 3]):
        assert sum(splits) == nblocks
        model = _model(pts0, pts1, n1, channels, h)
        assert np.array_equal(nc.model_calls(model, x, splits, w), want), splits[:5]
        assert model.position == nblocks


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_static_equivalence_from_block_r0_plus_2m(pts0, pts1, n1):
    """a zero object fed w = h repeated with period L against the object that was pushed h: equal, bit for bit in the
    model, from head block R0 + 2m on — the first whose own sum and both overlap tails were formed with every partition
    in place — and not before"""
    h, x, _ = _case(pts0, pts1, n1)
    channels, nblocks, m = x.shape[0], x.shape[1] // pts0, pts1 // pts0
    model = _model(pts0, pts1, n1, channels)
    w = np.concatenate([h[:, :model.L]] * (x.shape[1] // model.L + 1), axis=1)[:, :x.shape[1]]
    got = model.process(x, w)
    want = _model(pts0, pts1, n1, channels, h).process(x)
    first = model.R0 + 2 * m
    assert nblocks > first
    assert np.array_equal(got[:, first * pts0:], want[:, first * pts0:])
    differs = [j for j in range(nblocks) if not np.array_equal(got[:, j * pts0:(j + 1) * pts0], want[:, j * pts0:(j + 1) * pts0])]
    assert differs and differs[-1] == first - 1


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_impulse_readout(pts0, pts1, n1):
    """Bound: the samples are sums of at most 2m + n1 partition products, each through two forward transforms and one
    inverse of 2 * pts1 points at most in float64; 64 * eps * log2(2 * pts1) of the largest value covers that with room
    (1.3e-13 at pts1 = 256)."""
    m, R1 = pts1 // pts0, n1 + 2
    R0, L = R1 * m, R1 * pts1
    bound = 64 * np.finfo(np.float64).eps * np.log2(2 * pts1)
    for b, s in ((0, 0), (1, 5), (m - 1, 31), (m, 0), (R0 - 1, 7), (R0 + 3, 1)):
        nblocks = b + R0 + 1
        w = readout_stream(L, nblocks * pts0)
        x = np.zeros(nblocks * pts0)
        x[b * pts0 + s] = 1.0
        y = _model(pts0, pts1, n1, 1).process(x[None], w[None])[0]
        v = readout(w, b, s, pts0, pts1, n1)
        err = np.max(np.abs(y[b * pts0 + s:b * pts0 + s + L] - v)) / np.max(np.abs(v))
        assert err < bound, (b, s, err)
        assert np.max(np.abs(y[:b * pts0 + s]), initial=0.0) < bound * np.max(np.abs(v))   # nothing before the impulse


def test_freeze_a_plain_block_leaves_its_tail_partition_alone():
    pts0, pts1, n1 = 32, 256, 3
    h, x, w = _case(pts0, pts1, n1)
    channels, m = x.shape[0], pts1 // pts0
    U = 3                                   # tail block 3: r = 3, it would rewrite tail partition 1
    stop = (U + 1) * m + 1                  # one block past the phase 0 that files it
    held = _model(pts0, pts1, n1, channels, h)
    H1 = held.H1.copy()
    for spoil in (U * m, U * m + m - 1):    # the block's first and last head block
        model = _model(pts0, pts1, n1, channels, h)
        splits = [spoil, 1, stop - spoil - 1]
        nc.model_calls(model, x[:, :stop * pts0], splits, w[:, :stop * pts0], plain=(1,))
        assert np.array_equal(model.H1[:, 1], H1[:, 1]), spoil
        assert not np.array_equal(model.H1[:, 0], H1[:, 0])   # tail block 2 was whole: partition 0 is the second input's
    model = _model(pts0, pts1, n1, channels, h)
    model.process(x[:, :stop * pts0], w[:, :stop * pts0])
    assert not np.array_equal(model.H1[:, 1], H1[:, 1])
