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
from tests import util
from tests.nupconv_matrix_fade_model import NupMatrixFadeModel
from tests.test_gpu_nupconv_fade import TABLES, _fades, _mixed, _positions, _splits
from tests.test_gpu_nupconv_matrix import GEOMS, SEGS_ENV, _cvs, _object, _run

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
BIG = (64, 4096, 2, 2, 2)          # the largest pts1 and a head chain of 256 terms: two cases only
SMALL = [g for g in GEOMS if g != BIG]
SEGMENTED = (32, 256, 11, 3, 2)
# the big geometry's cases, as TABLES': indices of the push position and the fade length, the calls
BIG_CASES = [(3, 1, "one"), (5, 2, "odd")]
assert SEGS_ENV == "CLFA_PCONV_MATRIX_SEGS" and BIG in GEOMS and SEGMENTED in SMALL and len(SMALL) == 4


def _nblocks(geom):
    """the latest push, the longest fade and n1 + 4 periods after it"""
    m, n1 = geom[1] // geom[0], geom[2]
    return _positions(m, n1)[-1] + _fades(m)[-1] + (n1 + 4) * m


@functools.lru_cache(maxsize=None)
def _signals(geom):
    """(hA, hB, hC, x), read-only"""
    pts0, pts1, n1, I, O = geom
    rng = np.random.default_rng(7 * pts0 + pts1 + 10 * n1 + 100 * I + O)
    out = [rng.random((O, I, _cvs(pts1, n1)), dtype=np.float32) - 0.5 for _ in range(3)]
    out.append(rng.random((I, _nblocks(geom) * pts0), dtype=np.float32) - 0.5)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def _segs(p):
    return p.segments(0), p.segments(1)


_plain_cache = {}


def _plain(monkeypatch, geom, which, env=None):
    """(what a plain NupconvMatrix that holds response set `which` (0, 1, 2) since its creation returns for the whole
    signal in one call, its segments); computed once, read-only"""
    key = (geom, which, env)
    if key not in _plain_cache:
        sig = _signals(geom)
        p = _object(monkeypatch, geom, sig[which], env)
        out = _run(p, sig[3], [sig[3].shape[1] // geom[0]])
        out.setflags(write=False)
        _plain_cache[key] = (out, _segs(p))
    return _plain_cache[key]


def _ends(monkeypatch, geom, p, a=0, b=1, env=None):
    """yA, yB of the definition: plain objects at the faded object's segments"""
    (ya, sa), (yb, sb) = _plain(monkeypatch, geom, a, env), _plain(monkeypatch, geom, b, env)
    assert sa == _segs(p) and sb == _segs(p), (sa, sb, _segs(p))
    return ya, yb


def _device_rows(h, need):
    """response rows (outputs, inputs, need) at a longer stride, one float off the 8-byte grid"""
    O, I = h.shape[:2]
    rows = gg.rows(O * I, need, need + 3, misalign=1).fill(np.array(h[:, :, :need]).reshape(O * I, need))
    return rows, rows.data.unflatten(0, (O, I))


def _run_aligned(p, x, splits):
    """as _run on packed rows: every row of every call starts on a 16-byte boundary (the mix kernel's 16-byte row form)"""
    xd = gg.dev(x)
    out = torch.full((p.outputs, x.shape[1]), float("nan"), device=gg.DEV)
    j = 0
    for n in splits:
        a, b = j * p.pts0, (j + n) * p.pts0
        assert out[:, a:b].data_ptr() % 16 == 0 and out.stride(0) % 4 == 0
        assert p.process_device(out[:, a:b], xd[:, a:b]) == 0
        j += n
    torch.cuda.synchronize()
    assert j * p.pts0 == x.shape[1]
    return out.cpu().numpy()


def _faded(p, x, c, h2, fade, style, nblocks, host=False, run=_run):
    """p at position `start` <= c: the blocks up to c, the fade push, the blocks up to nblocks; fade_remaining() on the way"""
    pts0, start = p.pts0, p.position
    parts = []
    if c > start:
        parts.append(run(p, x[:, start * pts0:c * pts0], [c - start]))
    need = 2 * p.pts1 + p.nparts(1) * p.pts1
    if host:
        assert p.fade_ir(h2, fade) == 0
    else:
        rows, view = _device_rows(h2, need)
        assert p.fade_ir_device(view, fade) == 0
    assert p.fade_remaining() == fade and p.position == c
    j = c
    for n in _splits(style, fade, nblocks - c):
        parts.append(run(p, x[:, j * pts0:(j + n) * pts0], [n]))
        j += n
        assert p.fade_remaining() == max(0, fade - (j - c)) and p.position == j
    assert p.fade_remaining() == 0
    if not host:
        assert rows.unchanged(), "the response rows changed"
    return np.concatenate(parts, axis=1)


def _check_bits(monkeypatch, geom, cases, env=None):
    pts0, pts1, n1, I, O = geom
    hA, hB, _, x = _signals(geom)
    m = pts1 // pts0
    for ip, jf, style in cases:
        c, fade = _positions(m, n1)[ip], _fades(m)[jf]
        nblocks = c + fade + (n1 + 4) * m
        L = nblocks * pts0
        assert L <= x.shape[1]
        p = _object(monkeypatch, geom, hA, env)
        if geom == SEGMENTED and env is None:
            assert p.segments(0) > 1 and p.segments(1) > 1, _segs(p)
        yA, yB = _ends(monkeypatch, geom, p, env=env)
        want = _mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        got = _faded(p, x, c, hB, fade, style, nblocks)
        what = "%s, segments %s, push at %d, %d fade blocks, calls: %s" % (geom, _segs(p), c, fade, style)
        gg.same(got[:, :c * pts0], want[:, :c * pts0], what + " (before the fade)")
        gg.same(got[:, c * pts0:(c + fade) * pts0], want[:, c * pts0:(c + fade) * pts0], what + " (the fade)")
        gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], what + " (after the fade)")
        # the fade is audible
        assert not np.array_equal(yA[:, (c + fade) * pts0:L], yB[:, (c + fade) * pts0:L])


# every position, with every fade length and every cut of the stream, met several times over the two tables of
# tests/test_gpu_nupconv_fade.py and the four geometries
@pytest.mark.parametrize("geom,table", list(zip(SMALL, (1, 3, 3, 1))))
def test_bits_of_the_definition(monkeypatch, geom, table):
    _check_bits(monkeypatch, geom, TABLES[table])


def test_bits_of_the_definition_at_the_largest_pts1(monkeypatch):
    """P = 1 with s = 1, and P = n1 + 3 with s = 1, where the tail's ring has wrapped"""
    _check_bits(monkeypatch, BIG, BIG_CASES)


def test_bits_with_segments_that_cut_inside_an_input(monkeypatch):
    """CLFA_PCONV_MATRIX_SEGS=5 on all three objects: the head's cuts fall at r = 9, 19, 28, 38 of 48 and the tail's at
    6, 13, 19, 26 of 33, inside an input's partitions, in the priming and in the fade's blocks"""
    assert [48 * s // 5 for s in range(1, 5)] == [9, 19, 28, 38] and [33 * s // 5 for s in range(1, 5)] == [6, 13, 19, 26]
    _check_bits(monkeypatch, SEGMENTED, [(4, 2, "odd"), (5, 1, "singles"), (1, 1, "one")], env=5)


def test_host_form_aligned_rows_and_the_second_sets_bytes(monkeypatch):
    geom = (32, 256, 3, 4, 1)
    pts0, pts1, n1, I, O = geom
    hA, hB, _, x = _signals(geom)
    m = pts1 // pts0
    c, fade = 2 * m + 3, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    p = _object(monkeypatch, geom, hA)
    yA, yB = _ends(monkeypatch, geom, p)
    want = _mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    state, work = p.state_bytes(), p.workspace_bytes()
    gg.same(_faded(p, x, c, hB, fade, "odd", nblocks, host=True), want, "host push")
    # the second set is counted once it exists (the head's sub-batch workspaces grow with the calls: compare after them)
    state1, work1 = p.state_bytes(), p.workspace_bytes()
    assert state1 > state and work1 > work
    q = _object(monkeypatch, geom, hA)
    gg.same(_faded(q, x, c, hB, fade, "one", nblocks), want, "device push")
    # rows on 16-byte boundaries take the mix kernel's other row form: the same bits
    for style in ("singles", "odd"):
        got = _faded(_object(monkeypatch, geom, hA), x, c, hB, fade, style, nblocks, run=_run_aligned)
        gg.same(got, want, "aligned rows, calls: " + style)


@pytest.mark.parametrize("geom", [(32, 64, 1, 2, 3), SEGMENTED, (32, 256, 3, 1, 4)])
def test_a_fade_from_a_to_a_gives_the_bits_of_no_push(monkeypatch, geom):
    pts0, pts1, n1, I, O = geom
    hA, _, _, x = _signals(geom)
    m = pts1 // pts0
    c, fade = _positions(m, n1)[5], 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    p = _object(monkeypatch, geom, hA)
    yA, _ = _ends(monkeypatch, geom, p, 0, 0)
    got = _faded(p, x, c, hA, fade, "odd", nblocks)
    gg.same(got, yA[:, :nblocks * pts0], "a fade from A to A")


def test_after_the_fade_a_plain_push_at_phase_0_is_the_plain_objects(monkeypatch):
    """the exchange: the faded object pushed at phase 0 after its fade equals the object that always held B, pushed at the
    same block"""
    geom = SEGMENTED
    pts0, pts1, n1, I, O = geom
    hA, hB, hC, x = _signals(geom)
    m = pts1 // pts0
    c, fade = 2 * m + 1, m + 1
    c2 = 5 * m                                   # phase 0, after the fade's end
    nblocks = c2 + (n1 + 4) * m
    assert c + fade < c2 and nblocks * pts0 <= x.shape[1]
    ref = _object(monkeypatch, geom, hB)
    want = [_run(ref, x[:, :c2 * pts0], [c2])]
    assert ref.push_ir(hC) == 0
    want.append(_run(ref, x[:, c2 * pts0:nblocks * pts0], [nblocks - c2]))
    want = np.concatenate(want, axis=1)
    assert not np.array_equal(want[:, c2 * pts0:], _plain(monkeypatch, geom, 1)[0][:, c2 * pts0:nblocks * pts0])
    p = _object(monkeypatch, geom, hA)
    assert _segs(p) == _segs(ref)
    got = [_faded(p, x, c, hB, fade, "singles", c2)]
    assert p.position == c2 and p.position % m == 0
    assert p.push_ir(hC) == 0
    got.append(_run(p, x[:, c2 * pts0:nblocks * pts0], [3, nblocks - c2 - 3]))
    got = np.concatenate(got, axis=1)
    gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], "a plain push after the fade")


def test_a_second_fade(monkeypatch):
    geom = SEGMENTED
    pts0, pts1, n1, I, O = geom
    hA, hB, hC, x = _signals(geom)
    m = pts1 // pts0
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                         # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    assert L <= x.shape[1]
    p = _object(monkeypatch, geom, hA)
    yA, yB = _ends(monkeypatch, geom, p)
    _, yC = _ends(monkeypatch, geom, p, 0, 2)
    want = _mixed(_mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
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
    hA, hB, hC, x = _signals(geom)
    m = pts1 // pts0
    c, fade = 2 * m + 1, 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    need = 2 * pts1 + n1 * pts1
    p = _object(monkeypatch, geom, hA)
    yA, yB = _ends(monkeypatch, geom, p)
    want = _mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
    got = [_run(p, x[:, :c * pts0], [c])]
    rows, view = _device_rows(hC, need)
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
    rowsB, viewB = _device_rows(hB, need)
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
    """the float64 model of the schedule (tests/nupconv_matrix_fade_model.py) over the whole signal, per output, at the
    matrix's tolerance for a sum over inputs, util.TOL * inputs; the fade segment's figures are printed"""
    pts0, pts1, n1, I, O = geom
    hA, hB, _, x = _signals(geom)
    m = pts1 // pts0
    c, fade = (m + 1, 3) if geom == BIG else (2 * m + m - 1, m + 1)
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    p = _object(monkeypatch, geom, hA)
    segs = _segs(p)
    got = _faded(p, x, c, hB, fade, "one", nblocks)
    model = NupMatrixFadeModel(_cvs(pts1, n1), pts0, pts1, I, O, segs)
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
