"""Non-uniformly partitioned convolution matrix (NupconvMatrix, clfa_nupconv_matrix) on the device: the bits of the
PconvMatrix composition that defines it however the stream is cut into calls, accuracy against float64, rows at any stride
and alignment behind guard bands, refusals that leave the state alone, reset and a push at phase 0."""
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
SEGMENTED = nc.SEGMENTED
_run = functools.partial(nc.run, nc.MATRIX)
_segs = nc.segs


def _bits_however_cut(monkeypatch, geom, env):
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    assert nblocks == (n1 + 3) * m + 3
    want = None
    for splits in ([nblocks], [1] * nblocks, [1, m + 2, 2, 0, nblocks - m - 5]):
        p = nc.make(geom, h, monkeypatch, env)
        if want is None:
            if geom == SEGMENTED and env is None:
                assert p.segments(0) > 1 and p.segments(1) > 1, _segs(p)
            want = nc.composition(geom, monkeypatch, _segs(p))
        got = _run(p, x, splits)
        gg.same(got, want, "%s, segments %s, calls of %s blocks" % (geom, _segs(p), splits[:5]))
    # the tail is in there: the head alone is something else after 2 * pts1 samples
    assert not np.array_equal(got[:, 2 * pts1:3 * pts1], nc.head_only(geom, monkeypatch, _segs(p))[:, 2 * pts1:3 * pts1])


@pytest.mark.parametrize("geom", nc.MATRIX_GEOMS + nc.MATRIX_SIZE_GEOMS)
def test_bits_of_the_composition_however_the_stream_is_cut(monkeypatch, geom):
    _bits_however_cut(monkeypatch, geom, None)


def test_bits_with_segments_that_cut_inside_an_input(monkeypatch):
    """CLFA_PCONV_MATRIX_SEGS=5 for all three objects: the head's cuts fall at r = 9, 19, 28, 38 of 48, inside an input's
    16 partitions"""
    assert [48 * s // 5 for s in range(1, 5)] == [9, 19, 28, 38]
    _bits_however_cut(monkeypatch, SEGMENTED, 5)


@pytest.mark.parametrize("geom", nc.MATRIX_GEOMS + nc.MATRIX_SIZE_GEOMS)
def test_against_float64(monkeypatch, geom):
    """each output against the sum over the inputs of the definition in float64 (tests/nupconv_model.definition over
    tests/util.pconv_f64) at the matrix's tolerance for a sum over inputs, util.TOL * inputs"""
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    got = _run(nc.make(geom, h, monkeypatch), x, [x.shape[1] // pts0])
    for o in range(O):
        want = sum(definition(h[o, i], x[i], nc.cvs(pts1, n1), pts0, pts1) for i in range(I))
        l2, mx = util.rel_err(got[o], want)
        print("%s output %d: relL2 %.3g max/max %.3g" % (geom, o, l2, mx))
        util.assert_parity(got[o], want, tol=util.TOL * I, what="output %d" % o)


def test_host_form_and_empty_call(monkeypatch):
    geom = (32, 256, 3, 4, 1)
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    p = nc.make(geom, h, monkeypatch)
    want = nc.composition(geom, monkeypatch, _segs(p))
    assert p.process_device(torch.empty((O, 0), device=gg.DEV), torch.empty((I, 0), device=gg.DEV)) == 0 and p.position == 0
    out = np.zeros((O, x.shape[1]), np.float32)
    # a call of one block leaves the workspaces as creation made them; a call of many blocks grows the head's
    before = p.workspace_bytes()
    assert before > 0
    assert p.convolution(out[:, :pts0].copy(), x[:, :pts0]) == 0 and p.position == 1
    assert p.workspace_bytes() == before
    half = 13 * pts0
    assert p.convolution(out[:, :half - pts0].copy(), x[:, pts0:half]) == 0 and p.position == 13
    assert p.workspace_bytes() > before
    assert p.reset() == 0
    assert p.convolution(out, x) == 0
    gg.same(out, want, "host form")


def test_refusals_leave_the_state_untouched(monkeypatch):
    geom = (32, 64, 1, 2, 3)
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    p = nc.make(geom, h, monkeypatch)
    want = nc.composition(geom, monkeypatch, _segs(p))
    L, first = x.shape[1], 5 * pts0
    xin = gg.rows(I, L, L + 4).fill(np.array(x))
    got0 = _run(p, x[:, :first], [5])
    pos = p.position
    # out overlaps in: wholly, and in the last float of every row
    rows = max(I, O)
    buf = gg.rows(rows, 2 * pts0 + 1, 2 * pts0 + 6).fill(np.zeros((rows, 2 * pts0 + 1), np.float32))
    assert p.process_device(buf.data[:O, :pts0], buf.data[:I, :pts0]) == CL_INVALID_VALUE
    assert p.process_device(buf.data[:O, pts0 - 1:2 * pts0 - 1], buf.data[:I, :pts0]) == CL_INVALID_VALUE
    assert p.process_device(buf.data[:O, :pts0], buf.data[:I, pts0 - 1:2 * pts0 - 1]) == CL_INVALID_VALUE
    # a length that is no multiple of pts0, lengths that differ, row counts that do not match on either side
    o = gg.rows(O + 1, 2 * pts0, 2 * pts0 + 3)
    assert p.process_device(o.data[:O, :pts0 + 1], xin.data[:, :pts0 + 1]) == CL_INVALID_VALUE
    assert p.process_device(o.data[:O, :2 * pts0], xin.data[:, :pts0]) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        p.process_device(o.data[:, :pts0], xin.data[:, :pts0])
    with pytest.raises(ValueError):
        p.process_device(o.data[:O, :pts0], xin.data[:I - 1, :pts0])
    # a call and a reset under capture: the phase lives on the host
    dummy = torch.zeros(4, device=gg.DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.process_device(o.data[:O, :pts0], xin.data[:, :pts0], stream=torch.cuda.current_stream().cuda_stream)
        rr = p.reset(stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION and rr == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert o.untouched() and buf.unchanged() and xin.unchanged()
    assert p.position == pos
    # the stream goes on as if nothing had been asked
    rest = _run(p, x[:, first:], [(L - first) // pts0])
    gg.same(np.concatenate([got0, rest], axis=1), want, "after the refusals")


def test_reset_repeats_the_first_output(monkeypatch):
    geom = (32, 256, 3, 1, 4)
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    m = pts1 // pts0
    p = nc.make(geom, h, monkeypatch)
    want = nc.composition(geom, monkeypatch, _segs(p))
    part = (2 * m + 3) * pts0   # stops inside a period, a tail block half collected and another half multiplied
    gg.same(_run(p, x[:, :part], [2 * m + 3]), want[:, :part], "before the reset")
    assert p.reset() == 0 and p.position == 0
    gg.same(_run(p, x, [3, x.shape[1] // pts0 - 3]), want, "after the reset")


def test_push_at_phase_0_matches_the_composition_pushed_at_the_same_block(monkeypatch):
    """position c = 2 m: the head object is pushed before its block c, the tail object before its block 1, the tail block
    whose multiply-accumulate begins at c (clfft_amd.h)"""
    geom = SEGMENTED
    pts0, pts1, n1, I, O = geom
    h, x = nc.signals("plain", geom)
    h2 = np.random.default_rng(77).random(h.shape, dtype=np.float32) - 0.5
    m = pts1 // pts0
    c = 2 * m
    p = nc.make(geom, h, monkeypatch)
    want = nc.compose(*nc.levels(geom, h, monkeypatch, _segs(p)), gg.dev(x), pts1, push=(h2, c, 1))
    assert not np.array_equal(want[:, c * pts0:], nc.composition(geom, monkeypatch, _segs(p))[:, c * pts0:])
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
    q = nc.make(geom, h, monkeypatch)
    a = _run(q, x[:, :c * pts0], [c])
    assert q.push_ir(h2) == 0
    b = _run(q, x[:, c * pts0:], [1] * (x.shape[1] // pts0 - c))
    gg.same(np.concatenate([a, b], axis=1), want, "host push at phase 0")
