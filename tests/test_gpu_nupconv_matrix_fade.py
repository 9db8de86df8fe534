"""NupconvMatrix's timed crossfade of response changes (fade_ir, clfa_nupconv_matrix_push_ir_fade) on the device: the bits
of the definition, two plain objects of the same segments fed alike and mixed by g in float32, at every kind of push
position, fade length and cut of the stream into calls; segments that cut inside an input; the host form and rows on
16-byte boundaries; a fade from A to A; the exchange at the fade's end (a plain push and a second fade after it); the
refusals; and the float64 model of the schedule."""
import functools

import numpy as np
import pytest
import torch

from opencl_fft_amd._lib import lib
from tests import gpu_guard as gg
from tests import nupconv_cases as nc
from tests import util
from tests.nupconv_model import NupMatrixFadeModel

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
GEOMS, BIG, SMALL, SEGMENTED = nc.MATRIX_GEOMS, nc.BIG, nc.SMALL, nc.SEGMENTED
_run = functools.partial(nc.run, nc.MATRIX)
_faded = functools.partial(nc.faded, nc.MATRIX)
_segs = nc.segs


# every position, with every fade length and every cut of the stream, met several times over the two tables of
# tests/nupconv_cases.py and the four geometries
@pytest.mark.parametrize("geom,table", list(zip(SMALL, (1, 3, 3, 1))))
def test_bits_of_the_definition(monkeypatch, geom, table):
    nc.check_fade_bits(geom, nc.TABLES[table], monkeypatch)


def test_bits_of_the_definition_at_the_largest_pts1(monkeypatch):
    """P = 1 with s = 1, and P = n1 + 3 with s = 1, where the tail's ring has wrapped"""
    nc.check_fade_bits(BIG, nc.BIG_CASES, monkeypatch)


def test_bits_with_segments_that_cut_inside_an_input(monkeypatch):
    """CLFA_PCONV_MATRIX_SEGS=5 on all three objects: the head's cuts fall at r = 9, 19, 28, 38 of 48 and the tail's at
    6, 13, 19, 26 of 33, inside an input's partitions, in the priming and in the fade's blocks"""
    assert [48 * s // 5 for s in range(1, 5)] == [9, 19, 28, 38] and [33 * s // 5 for s in range(1, 5)] == [6, 13, 19, 26]
    nc.check_fade_bits(SEGMENTED, [(4, 2, "odd"), (5, 1, "singles"), (1, 1, "one")], monkeypatch, env=5)


def test_host_form_aligned_rows_and_the_second_sets_bytes(monkeypatch):
    geom = (32, 256, 3, 4, 1)
    pts0, pts1, n1, I, O = geom
    hA, hB, _, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = 2 * m + 3, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    p = nc.make(geom, hA, monkeypatch)
    yA, yB = nc.ends(geom, p, monkeypatch=monkeypatch)
    want = nc.mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    state, work = p.state_bytes(), p.workspace_bytes()
    gg.same(_faded(p, x, c, hB, fade, "odd", nblocks, host=True), want, "host push")
    # the second set is counted once it exists (the head's sub-batch workspaces grow with the calls: compare after them)
    state1, work1 = p.state_bytes(), p.workspace_bytes()
    assert state1 > state and work1 > work
    q = nc.make(geom, hA, monkeypatch)
    gg.same(_faded(q, x, c, hB, fade, "one", nblocks), want, "device push")
    # rows on 16-byte boundaries take the mix kernel's other row form: the same bits
    for style in ("singles", "odd"):
        got = _faded(nc.make(geom, hA, monkeypatch), x, c, hB, fade, style, nblocks, run=nc.run_aligned)
        gg.same(got, want, "aligned rows, calls: " + style)


@pytest.mark.parametrize("geom", [(32, 64, 1, 2, 3), SEGMENTED, (32, 256, 3, 1, 4)])
def test_a_fade_from_a_to_a_gives_the_bits_of_no_push(monkeypatch, geom):
    nc.check_a_to_a_bits(geom, monkeypatch)


def test_after_the_fade_a_plain_push_at_phase_0_is_the_plain_objects(monkeypatch):
    nc.check_a_plain_push_after_the_fade(SEGMENTED, monkeypatch)


def test_a_second_fade(monkeypatch):
    geom = SEGMENTED
    pts0, pts1, n1, I, O = geom
    hA, hB, hC, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                         # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    assert L <= x.shape[1]
    p = nc.make(geom, hA, monkeypatch)
    yA, yB = nc.ends(geom, p, monkeypatch=monkeypatch)
    _, yC = nc.ends(geom, p, 0, 2, monkeypatch)
    want = nc.mixed(nc.mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    first = _faded(p, x, c1, hB, f1, "odd", c2 - 2)
    first = np.concatenate([first, _run(p, x[:, (c2 - 2) * pts0:c2 * pts0], [2])], axis=1)
    state, work = p.state_bytes(), p.workspace_bytes()
    second = _faded(p, x, c2, hC, f2, "singles", nblocks)
    assert p.state_bytes() == state and p.workspace_bytes() == work   # the second set is kept for the next fade
    gg.same(np.concatenate([first, second], axis=1), want, "A to B, then B to C")
    assert not np.array_equal(yB[:, (c2 + f2) * pts0:L], yC[:, (c2 + f2) * pts0:L])
    # a third fade allocates nothing
    assert p.fade_ir(hA, 1) == 0 and p.state_bytes() == state and p.workspace_bytes() == work


def test_refusals_leave_the_state_untouched(monkeypatch):
    geom = (32, 64, 1, 2, 3)
    pts0, pts1, n1, I, O = geom
    hA, hB, hC, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = 2 * m + 1, 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    need = 2 * pts1 + n1 * pts1
    p = nc.make(geom, hA, monkeypatch)
    yA, yB = nc.ends(geom, p, monkeypatch=monkeypatch)
    want = nc.mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    got = [_run(p, x[:, :c * pts0], [c])]
    rows, view = nc.device_rows(hC, need)
    stream = torch.cuda.current_stream().cuda_stream
    fade_dev, fade_host = lib().clfa_nupconv_matrix_push_ir_fade_dev, lib().clfa_nupconv_matrix_push_ir_fade
    # the arguments: the fade length, then those of push_ir_dev
    for blocks in (0, -1, (2 ** 31 - 1) // pts0 + 1):
        assert p.fade_ir_device(view, blocks) == CL_INVALID_VALUE
        assert p.fade_ir(hC, blocks) == CL_INVALID_VALUE
    assert p.fade_ir_device(view[:, :, :need - 1], 3) == CL_INVALID_VALUE
    assert p.fade_ir(hC[:, :, :need - 1], 3) == CL_INVALID_VALUE
    assert p.fade_ir_device(view.transpose(0, 1), 3) == CL_INVALID_VALUE
    assert p.fade_ir(hC.transpose(1, 0, 2), 3) == CL_INVALID_VALUE
    assert fade_dev(p._h, rows.data.data_ptr(), need - 1, 3, stream) == CL_INVALID_VALUE
    assert fade_dev(p._h, None, need + 3, 3, stream) == CL_INVALID_VALUE
    assert fade_dev(p._h, rows.data.data_ptr() + 2, need + 3, 3, stream) == CL_INVALID_VALUE
    assert fade_host(p._h, None, 3) == CL_INVALID_VALUE
    # a fade push under capture: it allocates what the fade needs
    dummy = torch.zeros(4, device=gg.DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.fade_ir_device(view, 3, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert p.fade_remaining() == 0 and p.position == c
    # the fade, and one block of it
    rowsB, viewB = nc.device_rows(hB, need)
    assert p.fade_ir_device(viewB, fade) == 0
    got.append(_run(p, x[:, c * pts0:(c + 1) * pts0], [1]))
    # while it is pending: no other push, no reset
    assert p.fade_ir_device(view, 3) == CL_INVALID_OPERATION
    assert p.fade_ir(hC, 3) == CL_INVALID_OPERATION
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


@pytest.mark.parametrize("geom", GEOMS)
def test_against_float64(monkeypatch, geom):
    """the float64 model of the schedule (tests/nupconv_model.py) over the whole signal, per output, at the
    matrix's tolerance for a sum over inputs, util.TOL * inputs; the fade segment's figures are printed"""
    pts0, pts1, n1, I, O = geom
    hA, hB, _, x = nc.signals("fade", geom)
    m = pts1 // pts0
    c, fade = (m + 1, 3) if geom == BIG else (2 * m + m - 1, m + 1)
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    p = nc.make(geom, hA, monkeypatch)
    segs = _segs(p)
    got = _faded(p, x, c, hB, fade, "one", nblocks)
    model = NupMatrixFadeModel(nc.cvs(pts1, n1), pts0, pts1, I, O, segs)
    model.push_ir(hA)
    want = [model.process(x[:, :c * pts0])]
    model.push_ir_fade(hB, fade)
    want.append(model.process(x[:, c * pts0:L]))
    want = np.concatenate(want, axis=1)
    seg = slice(c * pts0, (c + fade) * pts0)
    for o in range(O):
        l2, mx = util.rel_err(got[o, seg], want[o, seg])
        print("%s output %d, the fade: relL2 %.3g max/max %.3g" % (geom, o, l2, mx))
        l2, mx = util.rel_err(got[o], want[o])
        print("%s output %d, the whole signal: relL2 %.3g max/max %.3g" % (geom, o, l2, mx))
        util.assert_parity(got[o], want[o], tol=util.TOL * I, what="output %d" % o)
