"""Nupconv's time-varying second input (process_tv_device, clfa_nupconv_process_tv_dev) on the device: the bits of the
push composition that defines it however the stream is cut and however plain calls are interleaved, static equivalence
from head block R0 + 2m on, the float64 model, the host form, reset, refusals that leave the state alone, and
time-varying calls after a fade."""
import functools

import numpy as np
import pytest
import torch

from opencl_fft_amd._lib import lib
from tests import gpu_guard as gg
from tests import nupconv_cases as nc
from tests import util
from tests.nupconv_definitions import Composition
from tests.nupconv_model import NupTvModel

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
# GEOMS; k_nupc_fwd (the forward transform with the stage copy folded in) at every size on both levels; tails on both sides
# of k_nupc_mac's prefetch depth
GEOMS, ALL_GEOMS = nc.GEOMS, nc.ALL_GEOMS


def _signals(pts0, pts1, n1, channels):
    return nc.signals("tv", (pts0, pts1, n1, channels))


def _object(pts0, pts1, n1, channels, h=None):
    return nc.make((pts0, pts1, n1, channels), h)


class _Plain:
    """the plain object of the definition on the device, as tests/nupconv_definitions.Composition drives it"""

    def __init__(self, pts0, pts1, n1, channels, h=None):
        self.p = _object(pts0, pts1, n1, channels, h)

    def push_ir(self, rows):
        torch.cuda.synchronize()
        assert self.p.push_ir(rows) == 0

    def process(self, x):
        xd = gg.dev(x)
        out = torch.empty_like(xd)
        assert self.p.process_device(out, xd) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _compose(pts0, pts1, n1, channels, h, x, w, plain=()):
    comp = Composition(_Plain(pts0, pts1, n1, channels, h), pts0, pts1, n1, channels, ir=h)
    want = comp.run(x, w, plain=plain)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _composition(pts0, pts1, n1, channels):
    """the push composition over the whole signal, every block time-varying, from pushed noise responses"""
    return _compose(pts0, pts1, n1, channels, *_signals(pts0, pts1, n1, channels))


def _run(p, x, w, splits, plain=()):
    return nc.run(nc.NUPCONV, p, x, splits, w, plain)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", ALL_GEOMS)
def test_bits_of_the_push_composition_however_the_stream_is_cut(pts0, pts1, n1, channels):
    h, x, w = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    n0 = 2 * m
    # a 0-block call, cuts inside the head stretch and at a = n0
    irregular = [1, m + 1, 0, n0 - m - 2, 3, nblocks - n0 - 3]
    assert sum(irregular) == nblocks and all(k >= 0 for k in irregular)
    for splits in ([nblocks], [1] * nblocks, irregular):
        got = _run(_object(pts0, pts1, n1, channels, h), x, w, splits)
        gg.same(got, want, "pts0 %d pts1 %d n1 %d, %d channels, calls of %s blocks" % (pts0, pts1, n1, channels, splits[:6]))
    # two blocks sent through plain process_device: block 3m arrives at the phase 0 that files tail block 2 (r = 2: tail
    # partition 0) and spoils tail block 3; the other falls inside tail block R1 + 2 and spoils it
    j1, j2 = 3 * m, (n1 + 4) * m + 1
    splits = [j1, 1, j2 - j1 - 1, 1, nblocks - j2 - 1]
    got = _run(_object(pts0, pts1, n1, channels, h), x, w, splits, plain=(1, 3))
    gg.same(got, _compose(pts0, pts1, n1, channels, h, x, w, plain=(j1, j2)), "two plain blocks")
    assert not np.array_equal(got, want)
    # the second input is heard
    p = _object(pts0, pts1, n1, channels, h)
    assert not np.array_equal(_run(p, x, w, [nblocks], plain=(0,)), want)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_static_equivalence_from_block_r0_plus_2m(pts0, pts1, n1, channels):
    h, x, _ = _signals(pts0, pts1, n1, channels)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    p = _object(pts0, pts1, n1, channels)
    L = p.tv_period * pts0
    assert L == 2 * pts1 + n1 * pts1
    w = np.concatenate([h[:, :L]] * (x.shape[1] // L + 1), axis=1)[:, :x.shape[1]]
    got = _run(p, x, w, [nblocks])
    want = _run(_object(pts0, pts1, n1, channels, h), x, w, [nblocks], plain=(0,))
    first = (p.tv_period + 2 * m) * pts0
    assert first < x.shape[1]
    gg.same(got[:, first:], want[:, first:], "from block R0 + 2m on")
    assert not np.array_equal(got[:, :first], want[:, :first])


@pytest.mark.parametrize("pts0,pts1,n1", ALL_GEOMS)
def test_against_the_float64_model(pts0, pts1, n1):
    """tests/nupconv_model.NupTvModel at the project's parity criterion, tests/util.TOL"""
    channels = 3
    h, x, w = _signals(pts0, pts1, n1, channels)
    got = _run(_object(pts0, pts1, n1, channels, h), x, w, [x.shape[1] // pts0])
    model = NupTvModel(nc.cvs(pts1, n1), pts0, pts1, channels)
    model.push_ir(h)
    want = model.process(x, w)
    for c in range(channels):
        l2, mx = util.rel_err(got[c], want[c])
        print("pts0 %d pts1 %d n1 %d channel %d: relL2 %.3g max/max %.3g" % (pts0, pts1, n1, c, l2, mx))
        util.assert_parity(got[c], want[c], what="channel %d" % c)


def test_host_form_reset_and_period():
    pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x, w = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    p = _object(pts0, pts1, n1, channels)
    plain_state, plain_ws = p.state_bytes(), p.workspace_bytes()
    assert p.tv_period == (n1 + 2) * m
    assert p.push_ir(h) == 0
    out = np.zeros_like(x)
    assert p.convolution_tv(out, x, w) == 0 and p.position == nblocks
    gg.same(out, want, "host form")
    # the second stage row is there from the first time-varying call on
    assert p.state_bytes() == plain_state + 4 * channels * pts1 and p.workspace_bytes() >= plain_ws
    # reset repeats the first output: the responses stay (they are what the stream left), so push them again
    assert p.reset() == 0 and p.position == 0
    assert p.push_ir(h) == 0
    part = (2 * m + 3) * pts0   # stops inside a tail block of the second input
    gg.same(_run(p, x[:, :part], w[:, :part], [2 * m + 3]), want[:, :part], "before the second reset")
    assert p.reset() == 0 and p.push_ir(h) == 0
    gg.same(_run(p, x, w, [3, nblocks - 3]), want, "after the reset")
    # a NULL second input is the plain call
    q, r = _object(pts0, pts1, n1, channels, h), _object(pts0, pts1, n1, channels, h)
    a, b = np.zeros_like(x), np.zeros_like(x)
    assert lib().clfa_nupconv_convolution_tv(q._h, a.ctypes.data, x.ctypes.data, None, nblocks) == 0
    assert r.convolution(b, x) == 0
    gg.same(a, b, "NULL second input")
    assert q.state_bytes() == plain_state


def test_the_second_input_may_be_the_first():
    pts0, pts1, n1, channels = 32, 64, 1, 3
    h, x, _ = _signals(pts0, pts1, n1, channels)
    want = _run(_object(pts0, pts1, n1, channels, h), x, x, [3, x.shape[1] // pts0 - 3])
    p = _object(pts0, pts1, n1, channels, h)
    xin = gg.rows(channels, x.shape[1], x.shape[1] + 4).fill(np.array(x))
    out = gg.rows(channels, x.shape[1], x.shape[1] + 9, misalign=1)
    a = 3 * pts0
    assert p.process_tv_device(out.data[:, :a], xin.data[:, :a], xin.data[:, :a]) == 0
    assert p.process_tv_device(out.data[:, a:], xin.data[:, a:], xin.data[:, a:]) == 0
    torch.cuda.synchronize()
    assert out.intact() and xin.unchanged()
    gg.same(out.host(), want, "in2 == in")


def test_refusals_leave_the_state_untouched():
    pts0, pts1, n1, channels = 32, 64, 1, 3
    h, x, w = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    L, first = x.shape[1], 5 * pts0
    p = _object(pts0, pts1, n1, channels, h)
    xin = gg.rows(channels, L, L + 4).fill(np.array(x))
    got0 = _run(p, x[:, :first], w[:, :first], [5])
    pos = p.position
    # out overlaps an input: wholly, and in the last float of every row, x and w in turn
    buf = gg.rows(channels, 2 * pts0 + 1, 2 * pts0 + 6).fill(np.zeros((channels, 2 * pts0 + 1), np.float32))
    one = xin.data[:, :pts0]
    assert p.process_tv_device(buf.data[:, :pts0], buf.data[:, :pts0], one) == CL_INVALID_VALUE
    assert p.process_tv_device(buf.data[:, :pts0], one, buf.data[:, :pts0]) == CL_INVALID_VALUE
    assert p.process_tv_device(buf.data[:, pts0 - 1:2 * pts0 - 1], buf.data[:, :pts0], one) == CL_INVALID_VALUE
    assert p.process_tv_device(buf.data[:, pts0 - 1:2 * pts0 - 1], one, buf.data[:, :pts0]) == CL_INVALID_VALUE
    assert p.process_tv_device(buf.data[:, :pts0], one, buf.data[:, pts0 - 1:2 * pts0 - 1]) == CL_INVALID_VALUE
    # lengths that differ, a length that is no multiple of pts0
    o = gg.rows(channels, 2 * pts0, 2 * pts0 + 3)
    assert p.process_tv_device(o.data[:, :2 * pts0], xin.data[:, :2 * pts0], xin.data[:, :pts0]) == CL_INVALID_VALUE
    assert p.process_tv_device(o.data[:, :2 * pts0], xin.data[:, :pts0], xin.data[:, :2 * pts0]) == CL_INVALID_VALUE
    assert p.process_tv_device(o.data[:, :pts0], xin.data[:, :2 * pts0], xin.data[:, :2 * pts0]) == CL_INVALID_VALUE
    assert p.process_tv_device(o.data[:, :pts0 + 1], xin.data[:, :pts0 + 1], xin.data[:, :pts0 + 1]) == CL_INVALID_VALUE
    # a call under capture: the phase lives on the host
    dummy = torch.zeros(4, device=gg.DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.process_tv_device(o.data[:, :pts0], one, one, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert o.untouched() and buf.unchanged() and xin.unchanged()
    assert p.position == pos
    # the stream goes on as if nothing had been asked
    rest = _run(p, x[:, first:], w[:, first:], [(L - first) // pts0])
    gg.same(np.concatenate([got0, rest], axis=1), want, "after the refusals")


def test_a_time_varying_call_during_a_fade_is_refused():
    pts0, pts1, n1, channels = 32, 64, 1, 3
    h, x, w = _signals(pts0, pts1, n1, channels)
    hB = np.random.default_rng(5).random(h.shape, dtype=np.float32) - 0.5
    fade, c = 3, 2
    p, q = _object(pts0, pts1, n1, channels, h), _object(pts0, pts1, n1, channels, h)
    a, b = c * pts0, (c + fade) * pts0
    for obj in (p, q):
        _run(obj, x[:, :a], w[:, :a], [c], plain=(0,))
        assert obj.push_ir_fade(hB, fade) == 0
    o = gg.rows(channels, pts0, pts0 + 3)
    xd = gg.dev(x[:, a:a + pts0])
    assert p.process_tv_device(o.data, xd, xd) == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert o.untouched() and p.position == c and p.fade_remaining() == fade
    # both go on alike: the fade's blocks as plain ones, then time-varying calls
    outs = [np.concatenate([_run(obj, x[:, a:b], w[:, a:b], [fade], plain=(0,)),
                            _run(obj, x[:, b:], w[:, b:], [x.shape[1] // pts0 - c - fade])], axis=1) for obj in (p, q)]
    gg.same(outs[0], outs[1], "after the refusal")


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_time_varying_calls_after_a_fade(pts0, pts1, n1):
    """object 1: push A, run, fade to B, time-varying calls after the fade.  Object 2: B held from the start, plain calls
    over the same blocks, then the push composition.  Equal from the fade's end."""
    channels = 3
    hA, x, w = _signals(pts0, pts1, n1, channels)
    hB = np.random.default_rng(6).random(hA.shape, dtype=np.float32) - 0.5
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    c, fade = m + 1, m + 2           # the push inside a period, the fade's end inside another
    end = c + fade
    p = _object(pts0, pts1, n1, channels, hA)
    a, b = c * pts0, end * pts0
    _run(p, x[:, :a], w[:, :a], [c], plain=(0,))
    assert p.push_ir_fade(hB, fade) == 0
    _run(p, x[:, a:b], w[:, a:b], [fade], plain=(0,))
    assert p.fade_remaining() == 0
    got = _run(p, x[:, b:], w[:, b:], [2, nblocks - end - 2])
    want = _compose(pts0, pts1, n1, channels, hB, x, w, plain=tuple(range(end)))
    gg.same(got, want[:, b:], "after the fade")
    assert not np.array_equal(got, _composition(pts0, pts1, n1, channels)[:, b:])
