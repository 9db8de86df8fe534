"""Non-uniformly partitioned convolution (Nupconv, clfa_nupconv) on the device: the bits of the Clpconv composition that
defines it however the stream is cut into calls, accuracy against float64, rows at any stride and alignment behind guard
bands, refusals that leave the state alone, reset and a push at phase 0."""
import functools

import numpy as np
import pytest
import torch

from tests import gpu_guard as gg
from tests import nupconv_cases as nc
from tests import util
from tests.nupconv_definitions import definition

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
_run = functools.partial(nc.run, nc.NUPCONV)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", nc.ALL_GEOMS)
def test_bits_of_the_composition_however_the_stream_is_cut(pts0, pts1, n1, channels):
    geom = (pts0, pts1, n1, channels)
    h, x = nc.signals("plain", geom)
    want = nc.composition(geom)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    assert nblocks == (n1 + 3) * m + 3 and nblocks - m - 5 > 0
    for splits in ([nblocks], [1] * nblocks, [1, m + 2, 2, 0, nblocks - m - 5]):
        got = _run(nc.make(geom, h), x, splits)
        gg.same(got, want, "pts0 %d pts1 %d n1 %d, %d channels, calls of %s blocks" % (pts0, pts1, n1, channels, splits[:5]))
    # the tail is in there: the head alone is something else after 2 * pts1 samples
    assert not np.array_equal(got[:, 2 * pts1:3 * pts1], nc.head_only(geom)[:, 2 * pts1:3 * pts1])


@pytest.mark.parametrize("pts0,pts1,n1", nc.ALL_GEOMS)
def test_against_float64(pts0, pts1, n1):
    """the definition in float64 (tests/nupconv_model.definition over tests/util.pconv_f64) at the project's parity
    criterion, tests/util.TOL"""
    channels = 3
    geom = (pts0, pts1, n1, channels)
    h, x = nc.signals("plain", geom)
    got = _run(nc.make(geom, h), x, [x.shape[1] // pts0])
    for c in range(channels):
        want = definition(h[c], x[c], nc.cvs(pts1, n1), pts0, pts1)
        l2, mx = util.rel_err(got[c], want)
        print("pts0 %d pts1 %d n1 %d channel %d: relL2 %.3g max/max %.3g" % (pts0, pts1, n1, c, l2, mx))
        util.assert_parity(got[c], want, what="channel %d" % c)


def test_host_form_and_empty_call():
    geom = pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = nc.signals("plain", geom)
    want = nc.composition(geom)
    p = nc.make(geom, h)
    empty = torch.empty((channels, 0), device=gg.DEV)
    assert p.process_device(empty, empty) == 0 and p.position == 0
    out = np.zeros_like(x)
    half = 13 * pts0
    assert p.convolution(out[:, :half].copy(), x[:, :half]) == 0 and p.position == 13
    assert p.reset() == 0
    assert p.convolution(out, x) == 0
    gg.same(out, want, "host form")
    assert p.workspace_bytes() > 0


def test_refusals_leave_the_state_untouched():
    geom = pts0, pts1, n1, channels = 32, 64, 1, 3
    h, x = nc.signals("plain", geom)
    want = nc.composition(geom)
    L, first = x.shape[1], 5 * pts0
    p = nc.make(geom, h)
    xin = gg.rows(channels, L, L + 4).fill(np.array(x))
    got0 = _run(p, x[:, :first], [5])
    pos = p.position
    # out overlaps in: wholly, and in the last float of every row
    buf = gg.rows(channels, 2 * pts0 + 1, 2 * pts0 + 6).fill(np.zeros((channels, 2 * pts0 + 1), np.float32))
    assert p.process_device(buf.data[:, :pts0], buf.data[:, :pts0]) == CL_INVALID_VALUE
    assert p.process_device(buf.data[:, pts0 - 1:2 * pts0 - 1], buf.data[:, :pts0]) == CL_INVALID_VALUE
    assert p.process_device(buf.data[:, :pts0], buf.data[:, pts0 - 1:2 * pts0 - 1]) == CL_INVALID_VALUE
    # a length that is no multiple of pts0, lengths that differ, a channel count that does not match
    o = gg.rows(channels + 1, 2 * pts0, 2 * pts0 + 3)
    assert p.process_device(o.data[:channels, :pts0 + 1], xin.data[:, :pts0 + 1]) == CL_INVALID_VALUE
    assert p.process_device(o.data[:channels, :2 * pts0], xin.data[:, :pts0]) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.process_device(o.data[:, :pts0], xin.data[:, :pts0])
    with pytest.raises(ValueError):
        p.process_device(o.data[:channels - 1, :pts0], xin.data[:channels - 1, :pts0])
    # a call under capture: the phase lives on the host
    dummy = torch.zeros(4, device=gg.DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.process_device(o.data[:channels, :pts0], xin.data[:, :pts0], stream=torch.cuda.current_stream().cuda_stream)
        rr = p.reset(stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION and rr == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert o.untouched() and buf.unchanged() and xin.unchanged()
    assert p.position == pos
    # the stream goes on as if nothing had been asked
    rest = _run(p, x[:, first:], [(L - first) // pts0])
    gg.same(np.concatenate([got0, rest], axis=1), want, "after the refusals")


def test_reset_repeats_the_first_output():
    geom = pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = nc.signals("plain", geom)
    want = nc.composition(geom)
    m = pts1 // pts0
    p = nc.make(geom, h)
    part = (2 * m + 3) * pts0   # stops inside a period, a tail block half collected and another half multiplied
    gg.same(_run(p, x[:, :part], [2 * m + 3]), want[:, :part], "before the reset")
    assert p.reset() == 0 and p.position == 0
    gg.same(_run(p, x, [3, x.shape[1] // pts0 - 3]), want, "after the reset")


def test_push_at_phase_0_matches_the_composition_pushed_at_the_same_block():
    """position c = 2 m: the head object is pushed before its block c, the tail object before its block 1, the tail block
    whose multiply-accumulate begins at c (clfft_amd.h)"""
    geom = pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = nc.signals("plain", geom)
    h2 = np.random.default_rng(77).random(h.shape, dtype=np.float32) - 0.5
    m = pts1 // pts0
    c = 2 * m
    want = nc.compose(*nc.levels(geom, h), gg.dev(x), pts1, push=(h2, c, 1))
    assert not np.array_equal(want[:, c * pts0:], nc.composition(geom)[:, c * pts0:])
    p = nc.make(geom, h)
    a = _run(p, x[:, :c * pts0], [c])
    assert p.position % m == 0
    # the device push: rows at a longer stride, one float off the 8-byte grid
    need = 2 * pts1 + n1 * pts1
    rows, view = nc.device_rows(h2, need)
    assert p.push_ir_device(view) == 0
    b = _run(p, x[:, c * pts0:], [x.shape[1] // pts0 - c])
    assert rows.unchanged()
    gg.same(np.concatenate([a, b], axis=1), want, "device push at phase 0")
    # the host push gives the same bits
    q = nc.make(geom, h)
    a = _run(q, x[:, :c * pts0], [c])
    assert q.push_ir(h2) == 0
    b = _run(q, x[:, c * pts0:], [1] * (x.shape[1] // pts0 - c))
    gg.same(np.concatenate([a, b], axis=1), want, "host push at phase 0")
