"""Non-uniformly partitioned convolution (Nupconv, clfa_nupconv) on the device: the bits of the Clpconv composition that
defines it however the stream is cut into calls, accuracy against float64, rows at any stride and alignment behind guard
bands, refusals that leave the state alone, reset and a push at phase 0."""
import functools

import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard as gg
from tests import util
from tests.nupconv_model import definition

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
GEOMS = [(32, 64, 1), (32, 256, 3), (64, 4096, 2)]   # pts0, pts1, n1
# m = 2 at every transform size of the blocks route: with (32, 64, 1) above each size 32 .. 4096 is once the head's and once
# the tail's (k_pconvb_fwd / k_pconvb_inv, one instantiation per size)
SIZE_GEOMS = [(64, 128, 2), (128, 256, 3), (256, 512, 1), (512, 1024, 2), (1024, 2048, 3), (2048, 4096, 1)]
# tails on both sides of k_nupc_mac's prefetch depth of 16 partitions: one short of a pass, a whole pass, one and two whole
# passes and a partial one after them
DEPTH_GEOMS = [(32, 64, 15), (32, 64, 16), (32, 64, 17), (32, 64, 33), (32, 256, 17)]
ALL_GEOMS = GEOMS + SIZE_GEOMS + DEPTH_GEOMS


def _cvs(pts1, n1):
    return 2 * pts1 + n1 * pts1 + 5   # a remainder, ignored


@functools.lru_cache(maxsize=None)
def _signals(pts0, pts1, n1, channels):
    """(h, x): responses of cvs samples and a signal of (n1 + 3) m + 3 head blocks (the tail's ring of n1 + 2 frames wraps),
    read-only"""
    rng = np.random.default_rng(pts0 + pts1 + 10 * n1 + channels)
    h = rng.random((channels, _cvs(pts1, n1)), dtype=np.float32) - 0.5
    x = rng.random((channels, ((n1 + 3) * (pts1 // pts0) + 3) * pts0), dtype=np.float32) - 0.5
    h.setflags(write=False)
    x.setflags(write=False)
    return h, x


def _levels(pts0, pts1, n1, channels, h):
    """the two Clpconv objects of the definition, holding h"""
    head = fa.Clpconv(0, 2 * pts1, pts0, channels=channels)
    tail = fa.Clpconv(0, _cvs(pts1, n1) - 2 * pts1, pts1, channels=channels)
    assert head.get_cl_err() == 0 and tail.get_cl_err() == 0
    assert head.blocks_kernel_name() == "k_pconvb_mac" and tail.blocks_kernel_name() == "k_pconvb_mac"
    assert head.nparts == 2 * pts1 // pts0 and tail.nparts == n1
    assert head.push_ir(h[:, :2 * pts1]) == 0 and tail.push_ir(h[:, 2 * pts1:]) == 0
    return head, tail


def _compose(head, tail, xd, pts1, push=None):
    """yh + yt delayed by 2 * pts1: both objects through process_blocks_device over the whole signal, the shifted
    concatenation and one torch addition.  push = (h2, head blocks before it, tail blocks before it)"""
    channels, L = xd.shape
    Lt = L // pts1 * pts1
    yh, yt = torch.empty_like(xd), torch.empty((channels, Lt), device=xd.device)
    cuts = [(0, L, 0, Lt)]
    if push is not None:
        h2, cb, tb = push
        a, b = cb * head.pts, tb * pts1
        cuts = [(0, a, 0, b), (a, L, b, Lt)]
    for i, (a0, a1, b0, b1) in enumerate(cuts):
        if i:
            torch.cuda.synchronize()
            assert head.push_ir(h2[:, :2 * pts1]) == 0 and tail.push_ir(h2[:, 2 * pts1:]) == 0
        if a1 > a0:
            assert head.process_blocks_device(yh[:, a0:a1], xd[:, a0:a1]) == 0
        if b1 > b0:
            assert tail.process_blocks_device(yt[:, b0:b1], xd[:, b0:b1]) == 0
    shifted = torch.cat([torch.zeros((channels, 2 * pts1), device=xd.device), yt], dim=1)[:, :L]
    want = yh + shifted
    torch.cuda.synchronize()
    return want.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _composition(pts0, pts1, n1, channels):
    h, x = _signals(pts0, pts1, n1, channels)
    want = _compose(*_levels(pts0, pts1, n1, channels, h), gg.dev(x), pts1)
    want.setflags(write=False)
    return want


def _object(pts0, pts1, n1, channels, h):
    p = fa.Nupconv(0, _cvs(pts1, n1), pts0, pts1, channels=channels)
    assert p.get_error() == 0, p.get_log()
    assert p.nparts(0) == 2 * pts1 // pts0 and p.nparts(1) == n1 and p.kernel_name() == "k_nupc_mac"
    assert p.position == 0 and p.state_bytes() > 0
    assert p.push_ir(h) == 0
    return p


def _run(p, x, splits):
    """the calls of `splits` blocks each on guarded rows: out at a longer stride, 4 bytes past a 16-byte boundary; the
    input at a longer stride, unchanged afterwards; nothing written outside out, every element of it written"""
    channels, L = x.shape
    xin = gg.rows(channels, L, L + 4).fill(np.array(x))   # (a copy: the cached signals are read-only)
    out = gg.rows(channels, L, L + 9, misalign=1)
    j, start = 0, p.position
    for n in splits:
        a, b = j * p.pts0, (j + n) * p.pts0
        assert p.process_device(out.data[:, a:b], xin.data[:, a:b]) == 0
        j += n
        assert p.position == start + j
    torch.cuda.synchronize()
    assert j * p.pts0 == L
    out.check_sides("the output rows")
    assert not out.unwritten(), "an output element was not written"
    assert xin.unchanged(), "the input changed"
    return out.host()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", ALL_GEOMS)
def test_bits_of_the_composition_however_the_stream_is_cut(pts0, pts1, n1, channels):
    h, x = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    assert nblocks == (n1 + 3) * m + 3 and nblocks - m - 5 > 0
    for splits in ([nblocks], [1] * nblocks, [1, m + 2, 2, 0, nblocks - m - 5]):
        got = _run(_object(pts0, pts1, n1, channels, h), x, splits)
        gg.same(got, want, "pts0 %d pts1 %d n1 %d, %d channels, calls of %s blocks" % (pts0, pts1, n1, channels, splits[:5]))
    # the tail is in there: the head alone is something else after 2 * pts1 samples
    assert not np.array_equal(got[:, 2 * pts1:3 * pts1], _head_only(pts0, pts1, n1, channels)[:, 2 * pts1:3 * pts1])


def _head_only(pts0, pts1, n1, channels):
    h, x = _signals(pts0, pts1, n1, channels)
    head, _ = _levels(pts0, pts1, n1, channels, h)
    xd = gg.dev(x)
    yh = torch.empty_like(xd)
    assert head.process_blocks_device(yh, xd) == 0
    torch.cuda.synchronize()
    return yh.cpu().numpy()


@pytest.mark.parametrize("pts0,pts1,n1", ALL_GEOMS)
def test_against_float64(pts0, pts1, n1):
    """the definition in float64 (tests/nupconv_model.definition over tests/util.pconv_f64) at the project's parity
    criterion, tests/util.TOL"""
    channels = 3
    h, x = _signals(pts0, pts1, n1, channels)
    got = _run(_object(pts0, pts1, n1, channels, h), x, [x.shape[1] // pts0])
    for c in range(channels):
        want = definition(h[c], x[c], _cvs(pts1, n1), pts0, pts1)
        l2, mx = util.rel_err(got[c], want)
        print("pts0 %d pts1 %d n1 %d channel %d: relL2 %.3g max/max %.3g" % (pts0, pts1, n1, c, l2, mx))
        util.assert_parity(got[c], want, what="channel %d" % c)


def test_host_form_and_empty_call():
    pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    p = _object(pts0, pts1, n1, channels, h)
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
    pts0, pts1, n1, channels = 32, 64, 1, 3
    h, x = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    L, first = x.shape[1], 5 * pts0
    p = _object(pts0, pts1, n1, channels, h)
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
    pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = _signals(pts0, pts1, n1, channels)
    want = _composition(pts0, pts1, n1, channels)
    m = pts1 // pts0
    p = _object(pts0, pts1, n1, channels, h)
    part = (2 * m + 3) * pts0   # stops inside a period, a tail block half collected and another half multiplied
    gg.same(_run(p, x[:, :part], [2 * m + 3]), want[:, :part], "before the reset")
    assert p.reset() == 0 and p.position == 0
    gg.same(_run(p, x, [3, x.shape[1] // pts0 - 3]), want, "after the reset")


def test_push_at_phase_0_matches_the_composition_pushed_at_the_same_block():
    """position c = 2 m: the head object is pushed before its block c, the tail object before its block 1, the tail block
    whose multiply-accumulate begins at c (clfft_amd.h)"""
    pts0, pts1, n1, channels = 32, 256, 3, 3
    h, x = _signals(pts0, pts1, n1, channels)
    h2 = np.random.default_rng(77).random(h.shape, dtype=np.float32) - 0.5
    m = pts1 // pts0
    c = 2 * m
    want = _compose(*_levels(pts0, pts1, n1, channels, h), gg.dev(x), pts1, push=(h2, c, 1))
    assert not np.array_equal(want[:, c * pts0:], _composition(pts0, pts1, n1, channels)[:, c * pts0:])
    p = _object(pts0, pts1, n1, channels, h)
    a = _run(p, x[:, :c * pts0], [c])
    assert p.position % m == 0
    # the device push: rows at a longer stride, one float off the 8-byte grid
    need = 2 * pts1 + n1 * pts1
    rows = gg.rows(channels, need, need + 3, misalign=1).fill(h2[:, :need])
    assert p.push_ir_device(rows.data) == 0
    b = _run(p, x[:, c * pts0:], [x.shape[1] // pts0 - c])
    assert rows.unchanged()
    gg.same(np.concatenate([a, b], axis=1), want, "device push at phase 0")
    # the host push gives the same bits
    q = _object(pts0, pts1, n1, channels, h)
    a = _run(q, x[:, :c * pts0], [c])
    assert q.push_ir(h2) == 0
    b = _run(q, x[:, c * pts0:], [1] * (x.shape[1] // pts0 - c))
    gg.same(np.concatenate([a, b], axis=1), want, "host push at phase 0")
