"""Nupconv's timed crossfade of response changes (push_ir_fade, clfa_nupconv_push_ir_fade) on the device: the bits of the
definition, two plain objects fed alike and mixed by g in float32, at every kind of push position, fade length and cut of
the stream into calls; the host form and misaligned rows; a fade from A to A; the exchange at the fade's end (a plain push
and a second fade after it); the refusals; and the float64 model of the schedule."""
import functools

import numpy as np
import pytest
import torch

from opencl_fft_amd._lib import lib
from tests import gpu_guard as gg
from tests import nupconv_cases as nc
from tests import util
from tests.nupconv_model import NupFadeModel

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
_run = functools.partial(nc.run, nc.NUPCONV)
_faded = functools.partial(nc.faded, nc.NUPCONV)


def _plain(geom, which):
    return nc.plain(geom, which)[0]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", nc.FADE_GEOMS)
def test_bits_of_the_definition(pts0, pts1, n1, channels):
    nc.check_fade_bits((pts0, pts1, n1, channels), nc.TABLES[channels])


def test_host_form_gives_the_bits_of_the_device_form():
    geom = pts0, pts1, n1, channels = 32, 256, 3, 3
    hA, hB, _, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = 2 * m + 3, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = nc.mixed(_plain(geom, 0)[:, :L], _plain(geom, 1)[:, :L], c, fade, pts0)
    p = nc.make(geom, hA)
    state, work = p.state_bytes(), p.workspace_bytes()
    gg.same(_faded(p, x, c, hB, fade, "odd", nblocks, host=True), want, "host push")
    # the second set is counted once it exists
    assert p.state_bytes() > state and p.workspace_bytes() > work
    gg.same(_faded(nc.make(geom, hA), x, c, hB, fade, "one", nblocks), want, "device push")
    # rows on 16-byte boundaries take the kernels' other row form: the same bits
    for style in ("singles", "odd"):
        got = _faded(nc.make(geom, hA), x, c, hB, fade, style, nblocks, run=nc.run_aligned)
        gg.same(got, want, "aligned rows, calls: " + style)


@pytest.mark.parametrize("pts0,pts1,n1", nc.GEOMS)
def test_a_fade_from_a_to_a_gives_the_bits_of_no_push(pts0, pts1, n1):
    nc.check_a_to_a_bits((pts0, pts1, n1, 3))


def test_after_the_fade_a_plain_push_at_phase_0_is_the_plain_objects():
    nc.check_a_plain_push_after_the_fade((32, 256, 3, 3))


def test_a_second_fade():
    geom = pts0, pts1, n1, channels = 32, 256, 3, 3
    hA, hB, hC, x = nc.signals("fade", geom)
    yA, yB, yC = (_plain(geom, k) for k in range(3))
    m = pts1 // pts0
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                         # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    assert L <= x.shape[1]
    want = nc.mixed(nc.mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    p = nc.make(geom, hA)
    first = _faded(p, x, c1, hB, f1, "odd", c2 - 2)
    state = p.state_bytes()
    second = _faded(p, x, c2, hC, f2, "one", nblocks)
    assert p.state_bytes() == state              # the second set is kept for the next fade
    gg.same(np.concatenate([first, second], axis=1), want, "A to B, then B to C")
    assert not np.array_equal(yB[:, (c2 + f2) * pts0:L], yC[:, (c2 + f2) * pts0:L])


def test_refusals_leave_the_state_untouched():
    geom = pts0, pts1, n1, channels = 32, 64, 1, 3
    hA, hB, hC, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = 2 * m + 1, 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = nc.mixed(_plain(geom, 0)[:, :L], _plain(geom, 1)[:, :L], c, fade, pts0)
    need = 2 * pts1 + n1 * pts1
    p = nc.make(geom, hA)
    got = [_run(p, x[:, :c * pts0], [c])]
    rows, view = nc.device_rows(hC, need)
    stream = torch.cuda.current_stream().cuda_stream
    # the arguments: the fade length, then those of push_ir_dev
    for blocks in (0, -1, (2 ** 31 - 1) // pts0 + 1):
        assert p.push_ir_fade_device(view, blocks) == CL_INVALID_VALUE
        assert p.push_ir_fade(hC, blocks) == CL_INVALID_VALUE
    assert p.push_ir_fade_device(view[:, :need - 1], 3) == CL_INVALID_VALUE
    assert p.push_ir_fade(hC[:, :need - 1], 3) == CL_INVALID_VALUE
    assert lib().clfa_nupconv_push_ir_fade_dev(p._h, rows.data.data_ptr(), need - 1, 3, stream) == CL_INVALID_VALUE
    assert lib().clfa_nupconv_push_ir_fade_dev(p._h, None, need, 3, stream) == CL_INVALID_VALUE
    assert lib().clfa_nupconv_push_ir_fade_dev(p._h, rows.data.data_ptr() + 2, need, 3, stream) == CL_INVALID_VALUE
    assert lib().clfa_nupconv_push_ir_fade(p._h, None, 3) == CL_INVALID_VALUE
    # a fade push under capture: it allocates what the fade needs
    dummy = torch.zeros(4, device=gg.DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.push_ir_fade_device(view, 3, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert p.fade_remaining() == 0 and p.position == c
    # the fade, and one block of it
    rowsB, viewB = nc.device_rows(hB, need)
    assert p.push_ir_fade_device(viewB, fade) == 0
    got.append(_run(p, x[:, c * pts0:(c + 1) * pts0], [1]))
    # while it is pending: no other push, no reset
    assert p.push_ir_fade_device(view, 3) == CL_INVALID_OPERATION
    assert p.push_ir_fade(hC, 3) == CL_INVALID_OPERATION
    assert p.push_ir_device(view) == CL_INVALID_OPERATION
    assert p.push_ir(hC) == CL_INVALID_OPERATION
    assert p.reset() == CL_INVALID_OPERATION
    assert p.fade_remaining() == fade - 1 and p.position == c + 1
    torch.cuda.synchronize()
    assert rows.unchanged() and rowsB.unchanged()
    # the stream goes on as if nothing had been asked
    got.append(_run(p, x[:, (c + 1) * pts0:L], [2, nblocks - c - 3]))
    assert p.fade_remaining() == 0
    gg.same(np.concatenate(got, axis=1), want, "after the refusals")
    # and with no fade pending the object takes a reset and a push again
    assert p.reset() == 0 and p.position == 0 and p.push_ir(hC) == 0


@pytest.mark.parametrize("pts0,pts1,n1", nc.GEOMS)
def test_against_float64(pts0, pts1, n1):
    """the float64 model of the schedule (tests/nupconv_model.py) over the whole signal at the project's parity
    criterion, tests/util.TOL; the fade segment's figures are printed"""
    channels = 3
    geom = (pts0, pts1, n1, channels)
    hA, hB, _, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = 2 * m + m - 1, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    got = _faded(nc.make(geom, hA), x, c, hB, fade, "one", nblocks)
    model = NupFadeModel(nc.cvs(pts1, n1), pts0, pts1, channels)
    model.push_ir(hA)
    want = [model.process(x[:, :c * pts0])]
    model.push_ir_fade(hB, fade)
    want.append(model.process(x[:, c * pts0:L]))
    want = np.concatenate(want, axis=1)
    seg = slice(c * pts0, (c + fade) * pts0)
    for ch in range(channels):
        l2, mx = util.rel_err(got[ch, seg], want[ch, seg])
        print("pts0 %d pts1 %d n1 %d channel %d, the fade: relL2 %.3g max/max %.3g" % (pts0, pts1, n1, ch, l2, mx))
        l2, mx = util.rel_err(got[ch], want[ch])
        print("pts0 %d pts1 %d n1 %d channel %d, the whole signal: relL2 %.3g max/max %.3g" % (pts0, pts1, n1, ch, l2, mx))
        util.assert_parity(got[ch], want[ch], what="channel %d" % ch)
