"""Non-uniformly partitioned convolution matrix (NupconvMatrix, clfa_nupconv_matrix) on the device: the bits of the
PconvMatrix composition that defines it however the stream is cut into calls, accuracy against float64, rows at any stride
and alignment behind guard bands, refusals that leave the state alone, reset and a push at phase 0."""
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
SEGS_ENV = "CLFA_PCONV_MATRIX_SEGS"
# pts0, pts1, n1, inputs, outputs
GEOMS = [(32, 64, 1, 2, 3),       # m = 2: the tail's forward and inverse in consecutive calls; 16-item slices share waves
         (32, 256, 11, 3, 2),     # both levels segmented (3 and 2 on 256 CUs), on both sides of the prefetch depth
         (64, 4096, 2, 2, 2),     # the largest pts1, a head chain of 128 partitions x 2 inputs
         (32, 256, 3, 1, 4),      # one input
         (32, 256, 3, 4, 1)]      # one output
# the transform sizes 128 and 2048, which no geometry above has, as head and as tail (this file's two parametrised tests;
# tests/test_gpu_nupconv_matrix_fade.py keeps GEOMS)
SIZE_GEOMS = [(128, 512, 2, 2, 2), (512, 2048, 1, 2, 3)]
SEGMENTED = (32, 256, 11, 3, 2)


def _cvs(pts1, n1):
    return 2 * pts1 + n1 * pts1 + 5   # a remainder, ignored


@functools.lru_cache(maxsize=None)
def _signals(pts0, pts1, n1, I, O):
    """(h, x): responses of cvs samples and a signal of (n1 + 3) m + 3 head blocks (the tail's ring wraps), read-only"""
    rng = np.random.default_rng(pts0 + pts1 + 10 * n1 + 100 * I + O)
    h = rng.random((O, I, _cvs(pts1, n1)), dtype=np.float32) - 0.5
    x = rng.random((I, ((n1 + 3) * (pts1 // pts0) + 3) * pts0), dtype=np.float32) - 0.5
    h.setflags(write=False)
    x.setflags(write=False)
    return h, x


def _object(monkeypatch, geom, h, env=None):
    pts0, pts1, n1, I, O = geom
    if env is None:
        monkeypatch.delenv(SEGS_ENV, raising=False)
    else:
        monkeypatch.setenv(SEGS_ENV, str(env))
    p = fa.NupconvMatrix(0, _cvs(pts1, n1), pts0, pts1, I, O)
    monkeypatch.delenv(SEGS_ENV, raising=False)
    assert p.get_error() == 0, p.get_log()
    assert p.nparts(0) == 2 * pts1 // pts0 and p.nparts(1) == n1 and p.kernel_name() == "k_nupm_mac"
    assert p.segments(0) >= 1 and p.segments(1) >= 1 and p.segments(2) == 0
    if env is not None:
        assert p.segments(0) == env and p.segments(1) == env
    assert p.position == 0 and p.state_bytes() > 0
    if h is not None:
        assert p.push_ir(h) == 0
    return p


def _levels(monkeypatch, geom, segs, h):
    """the two PconvMatrix objects of the definition, each created with the object's segment count, holding h"""
    pts0, pts1, n1, I, O = geom
    made = []
    for cvs, pts, s in ((2 * pts1, pts0, segs[0]), (_cvs(pts1, n1) - 2 * pts1, pts1, segs[1])):
        monkeypatch.setenv(SEGS_ENV, str(s))
        made.append(fa.PconvMatrix(0, cvs, pts, I, O))
        monkeypatch.delenv(SEGS_ENV, raising=False)
        assert made[-1].get_error() == 0, made[-1].get_log()
    head, tail = made
    assert head.nparts == 2 * pts1 // pts0 and tail.nparts == n1
    assert head.push_ir(h[:, :, :2 * pts1]) == 0 and tail.push_ir(h[:, :, 2 * pts1:]) == 0
    return head, tail


def _compose(head, tail, xd, O, pts1, push=None):
    """yh + yt delayed by 2 * pts1: both objects through process_device over the whole signal, the shifted concatenation
    and one torch addition.  push = (h2, head blocks before it, tail blocks before it)"""
    L = xd.shape[1]
    Lt = L // pts1 * pts1
    yh, yt = torch.empty((O, L), device=xd.device), torch.empty((O, Lt), device=xd.device)
    cuts = [(0, L, 0, Lt)]
    if push is not None:
        h2, cb, tb = push
        a, b = cb * head.pts, tb * pts1
        cuts = [(0, a, 0, b), (a, L, b, Lt)]
    for k, (a0, a1, b0, b1) in enumerate(cuts):
        if k:
            torch.cuda.synchronize()
            assert head.push_ir(h2[:, :, :2 * pts1]) == 0 and tail.push_ir(h2[:, :, 2 * pts1:]) == 0
        if a1 > a0:
            assert head.process_device(yh[:, a0:a1], xd[:, a0:a1]) == 0
        if b1 > b0:
            assert tail.process_device(yt[:, b0:b1], xd[:, b0:b1]) == 0
    shifted = torch.cat([torch.zeros((O, 2 * pts1), device=xd.device), yt], dim=1)[:, :L]
    want = yh + shifted
    torch.cuda.synchronize()
    return want.cpu().numpy()


_cache = {}


def _composition(monkeypatch, geom, segs):
    """the composition's output for the cached signals at these segment counts, computed once, read-only"""
    key = (geom, tuple(segs))
    if key not in _cache:
        h, x = _signals(*geom)
        want = _compose(*_levels(monkeypatch, geom, segs, h), gg.dev(x), geom[4], geom[1])
        want.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def _segs(p):
    return p.segments(0), p.segments(1)


def _run(p, x, splits):
    """the calls of `splits` blocks each on guarded rows: out at a longer stride, 4 bytes past a 16-byte boundary; the
    input at a longer stride, unchanged afterwards; nothing written outside out, every element of it written"""
    L = x.shape[1]
    xin = gg.rows(p.inputs, L, L + 4).fill(np.array(x))   # (a copy: the cached signals are read-only)
    out = gg.rows(p.outputs, L, L + 9, misalign=1)
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


def _head_only(monkeypatch, geom, segs):
    h, x = _signals(*geom)
    head, _ = _levels(monkeypatch, geom, segs, h)
    yh = torch.empty((geom[4], x.shape[1]), device=gg.DEV)
    assert head.process_device(yh, gg.dev(x)) == 0
    torch.cuda.synchronize()
    return yh.cpu().numpy()


def _bits_however_cut(monkeypatch, geom, env):
    pts0, pts1, n1, I, O = geom
    h, x = _signals(*geom)
    m, nblocks = pts1 // pts0, x.shape[1] // pts0
    assert nblocks == (n1 + 3) * m + 3
    want = None
    for splits in ([nblocks], [1] * nblocks, [1, m + 2, 2, 0, nblocks - m - 5]):
        p = _object(monkeypatch, geom, h, env)
        if want is None:
            if geom == SEGMENTED and env is None:
                assert p.segments(0) > 1 and p.segments(1) > 1, _segs(p)
            want = _composition(monkeypatch, geom, _segs(p))
        got = _run(p, x, splits)
        gg.same(got, want, "%s, segments %s, calls of %s blocks" % (geom, _segs(p), splits[:5]))
    # the tail is in there: the head alone is something else after 2 * pts1 samples
    assert not np.array_equal(got[:, 2 * pts1:3 * pts1], _head_only(monkeypatch, geom, _segs(p))[:, 2 * pts1:3 * pts1])


@pytest.mark.parametrize("geom", GEOMS + SIZE_GEOMS)
def test_bits_of_the_composition_however_the_stream_is_cut(monkeypatch, geom):
    _bits_however_cut(monkeypatch, geom, None)


def test_bits_with_segments_that_cut_inside_an_input(monkeypatch):
    """CLFA_PCONV_MATRIX_SEGS=5 for all three objects: the head's cuts fall at r = 9, 19, 28, 38 of 48, inside an input's
    16 partitions"""
    assert [48 * s // 5 for s in range(1, 5)] == [9, 19, 28, 38]
    _bits_however_cut(monkeypatch, SEGMENTED, 5)


@pytest.mark.parametrize("geom", GEOMS + SIZE_GEOMS)
def test_against_float64(monkeypatch, geom):
    """each output against the sum over the inputs of the definition in float64 (tests/nupconv_model.definition over
    tests/util.pconv_f64) at the matrix's tolerance for a sum over inputs, util.TOL * inputs"""
    pts0, pts1, n1, I, O = geom
    h, x = _signals(*geom)
    got = _run(_object(monkeypatch, geom, h), x, [x.shape[1] // pts0])
    for o in range(O):
        want = sum(definition(h[o, i], x[i], _cvs(pts1, n1), pts0, pts1) for i in range(I))
        l2, mx = util.rel_err(got[o], want)
        print("%s output %d: relL2 %.3g max/max %.3g" % (geom, o, l2, mx))
        util.assert_parity(got[o], want, tol=util.TOL * I, what="output %d" % o)


def test_host_form_and_empty_call(monkeypatch):
    geom = (32, 256, 3, 4, 1)
    pts0, pts1, n1, I, O = geom
    h, x = _signals(*geom)
    p = _object(monkeypatch, geom, h)
    want = _composition(monkeypatch, geom, _segs(p))
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
    h, x = _signals(*geom)
    p = _object(monkeypatch, geom, h)
    want = _composition(monkeypatch, geom, _segs(p))
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
    h, x = _signals(*geom)
    m = pts1 // pts0
    p = _object(monkeypatch, geom, h)
    want = _composition(monkeypatch, geom, _segs(p))
    part = (2 * m + 3) * pts0   # stops inside a period, a tail block half collected and another half multiplied
    gg.same(_run(p, x[:, :part], [2 * m + 3]), want[:, :part], "before the reset")
    assert p.reset() == 0 and p.position == 0
    gg.same(_run(p, x, [3, x.shape[1] // pts0 - 3]), want, "after the reset")


def test_push_at_phase_0_matches_the_composition_pushed_at_the_same_block(monkeypatch):
    """position c = 2 m: the head object is pushed before its block c, the tail object before its block 1, the tail block
    whose multiply-accumulate begins at c (clfft_amd.h)"""
    geom = SEGMENTED
    pts0, pts1, n1, I, O = geom
    h, x = _signals(*geom)
    h2 = np.random.default_rng(77).random(h.shape, dtype=np.float32) - 0.5
    m = pts1 // pts0
    c = 2 * m
    p = _object(monkeypatch, geom, h)
    want = _compose(*_levels(monkeypatch, geom, _segs(p), h), gg.dev(x), O, pts1, push=(h2, c, 1))
    assert not np.array_equal(want[:, c * pts0:], _composition(monkeypatch, geom, _segs(p))[:, c * pts0:])
    a = _run(p, x[:, :c * pts0], [c])
    assert p.position % m == 0
    # the device push: rows at a longer stride, one float off the 8-byte grid
    need = 2 * pts1 + n1 * pts1
    rows = gg.rows(O * I, need, need + 3, misalign=1).fill(h2[:, :, :need].reshape(O * I, need))
    assert p.push_ir_device(rows.data.unflatten(0, (O, I))) == 0
    b = _run(p, x[:, c * pts0:], [x.shape[1] // pts0 - c])
    assert rows.unchanged()
    gg.same(np.concatenate([a, b], axis=1), want, "device push at phase 0")
    # the host push gives the same bits
    q = _object(monkeypatch, geom, h)
    a = _run(q, x[:, :c * pts0], [c])
    assert q.push_ir(h2) == 0
    b = _run(q, x[:, c * pts0:], [1] * (x.shape[1] // pts0 - c))
    gg.same(np.concatenate([a, b], axis=1), want, "host push at phase 0")
