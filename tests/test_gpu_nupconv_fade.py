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
from tests import util
from tests.nupconv_fade_model import NupFadeModel
from tests.test_gpu_nupconv import GEOMS, _cvs, _object, _run

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
# the main fade test also at the head and tail sizes no other geometry has (128, 2048), and with tails past the prefetch
# depth of k_nupc_mac, whose block is the four-job launch during a fade
FADE_GEOMS = GEOMS + [(128, 256, 3), (1024, 2048, 3), (32, 64, 17), (32, 64, 33)]


def _positions(m, n1):
    """the push positions: c = 0; c = 1, in the first period; P = 1 with s = 0 and s = 1; P = 2 with s = m - 1; P = n1 + 3
    with s = 1, where the tail's ring has wrapped"""
    return [0, 1, m, m + 1, 2 * m + m - 1, (n1 + 3) * m + 1]


def _fades(m):
    return [1, m + 1, 2 * m + 3]


def _nblocks(m, n1):
    """the latest push, the longest fade and n1 + 4 periods after it"""
    return _positions(m, n1)[-1] + _fades(m)[-1] + (n1 + 4) * m


@functools.lru_cache(maxsize=None)
def _signals(pts0, pts1, n1, channels):
    """(hA, hB, hC, x), read-only"""
    rng = np.random.default_rng(7 * pts0 + pts1 + 10 * n1 + channels)
    out = [rng.random((channels, _cvs(pts1, n1)), dtype=np.float32) - 0.5 for _ in range(3)]
    out.append(rng.random((channels, _nblocks(pts1 // pts0, n1) * pts0), dtype=np.float32) - 0.5)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _plain(pts0, pts1, n1, channels, which):
    """what a plain Nupconv that holds response set `which` (0, 1, 2) returns for the whole signal in one call"""
    sig = _signals(pts0, pts1, n1, channels)
    x = sig[3]
    out = _run(_object(pts0, pts1, n1, channels, sig[which]), x, [x.shape[1] // pts0])
    out.setflags(write=False)
    return out


def _mixed(a, b, c, fade, pts0):
    """the definition on the host in float32: a before the fade, a + g * (b - a) inside it, b after it"""
    n0, N = c * pts0, fade * pts0
    g = np.arange(N).astype(np.float32) / np.float32(N)
    want = np.array(a)
    sa, sb = a[:, n0:n0 + N], b[:, n0:n0 + N]
    want[:, n0:n0 + N] = sa + g * (sb - sa)
    want[:, n0 + N:] = b[:, n0 + N:]
    assert want.dtype == np.float32
    return want


def _device_rows(h, need):
    """response rows at a longer stride, one float off the 8-byte grid"""
    return gg.rows(h.shape[0], need, need + 3, misalign=1).fill(np.array(h[:, :need]))   # (a copy: the cached rows are read-only)


def _splits(style, fade, rest):
    """the calls after the push: one; single blocks; an odd split whose second call starts inside the fade and ends after it"""
    if style == "one":
        return [rest]
    if style == "singles":
        return [1] * rest
    assert fade >= 2
    first, second = fade // 2, fade - fade // 2 + 2
    return [first, second, rest - first - second]


def _run_aligned(p, x, splits):
    """as _run on packed rows: every row of every call starts on a 16-byte boundary (the kernels' 16-byte row forms)"""
    xd = gg.dev(x)
    out = torch.full_like(xd, float("nan"))
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
        assert p.push_ir_fade(h2, fade) == 0
    else:
        rows = _device_rows(h2, need)
        assert p.push_ir_fade_device(rows.data, fade) == 0
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


# (push position, fade length, calls): indices into _positions and _fades.  Every position, with every fade length and
# every cut of the stream met several times over the two tables and the three geometries
TABLES = {
    1: [(0, 1, "odd"), (1, 0, "singles"), (2, 2, "one"), (3, 1, "singles"), (4, 2, "odd"), (5, 0, "one")],
    3: [(0, 2, "singles"), (1, 1, "odd"), (2, 0, "one"), (3, 2, "odd"), (4, 0, "singles"), (5, 1, "one"), (5, 2, "singles")],
}


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pts0,pts1,n1", FADE_GEOMS)
def test_bits_of_the_definition(pts0, pts1, n1, channels):
    hA, hB, _, x = _signals(pts0, pts1, n1, channels)
    yA, yB = _plain(pts0, pts1, n1, channels, 0), _plain(pts0, pts1, n1, channels, 1)
    m = pts1 // pts0
    for ip, jf, style in TABLES[channels]:
        c, fade = _positions(m, n1)[ip], _fades(m)[jf]
        nblocks = c + fade + (n1 + 4) * m
        L = nblocks * pts0
        want = _mixed(yA[:, :L], yB[:, :L], c, fade, pts0)
        got = _faded(_object(pts0, pts1, n1, channels, hA), x, c, hB, fade, style, nblocks)
        what = "pts0 %d pts1 %d n1 %d, %d channels, push at %d, %d fade blocks, calls: %s" % (pts0, pts1, n1, channels, c, fade, style)
        gg.same(got[:, :c * pts0], want[:, :c * pts0], what + " (before the fade)")
        gg.same(got[:, c * pts0:(c + fade) * pts0], want[:, c * pts0:(c + fade) * pts0], what + " (the fade)")
        gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], what + " (after the fade)")
        # the fade is audible
        assert not np.array_equal(yA[:, (c + fade) * pts0:L], yB[:, (c + fade) * pts0:L])


def test_host_form_gives_the_bits_of_the_device_form():
    pts0, pts1, n1, channels = 32, 256, 3, 3
    hA, hB, _, x = _signals(pts0, pts1, n1, channels)
    m = pts1 // pts0
    c, fade = 2 * m + 3, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = _mixed(_plain(pts0, pts1, n1, channels, 0)[:, :L], _plain(pts0, pts1, n1, channels, 1)[:, :L], c, fade, pts0)
    p = _object(pts0, pts1, n1, channels, hA)
    state, work = p.state_bytes(), p.workspace_bytes()
    gg.same(_faded(p, x, c, hB, fade, "odd", nblocks, host=True), want, "host push")
    # the second set is counted once it exists
    assert p.state_bytes() > state and p.workspace_bytes() > work
    gg.same(_faded(_object(pts0, pts1, n1, channels, hA), x, c, hB, fade, "one", nblocks), want, "device push")
    # rows on 16-byte boundaries take the kernels' other row form: the same bits
    for style in ("singles", "odd"):
        got = _faded(_object(pts0, pts1, n1, channels, hA), x, c, hB, fade, style, nblocks, run=_run_aligned)
        gg.same(got, want, "aligned rows, calls: " + style)


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_a_fade_from_a_to_a_gives_the_bits_of_no_push(pts0, pts1, n1):
    channels = 3
    hA, _, _, x = _signals(pts0, pts1, n1, channels)
    m = pts1 // pts0
    c, fade = _positions(m, n1)[5], 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    got = _faded(_object(pts0, pts1, n1, channels, hA), x, c, hA, fade, "odd", nblocks)
    gg.same(got, _plain(pts0, pts1, n1, channels, 0)[:, :nblocks * pts0], "a fade from A to A")


def test_after_the_fade_a_plain_push_at_phase_0_is_the_plain_objects():
    """the exchange: the faded object pushed at phase 0 after its fade equals the object that always held B, pushed at the
    same block"""
    pts0, pts1, n1, channels = 32, 256, 3, 3
    hA, hB, hC, x = _signals(pts0, pts1, n1, channels)
    m = pts1 // pts0
    c, fade = 2 * m + 1, m + 1
    c2 = 5 * m                                   # phase 0, after the fade's end
    nblocks = c2 + (n1 + 4) * m
    assert c + fade < c2 and nblocks * pts0 <= x.shape[1]
    ref = _object(pts0, pts1, n1, channels, hB)
    want = [_run(ref, x[:, :c2 * pts0], [c2])]
    assert ref.push_ir(hC) == 0
    want.append(_run(ref, x[:, c2 * pts0:nblocks * pts0], [nblocks - c2]))
    want = np.concatenate(want, axis=1)
    assert not np.array_equal(want[:, c2 * pts0:], _plain(pts0, pts1, n1, channels, 1)[:, c2 * pts0:nblocks * pts0])
    p = _object(pts0, pts1, n1, channels, hA)
    got = [_faded(p, x, c, hB, fade, "singles", c2)]
    assert p.position == c2 and p.position % m == 0
    assert p.push_ir(hC) == 0
    got.append(_run(p, x[:, c2 * pts0:nblocks * pts0], [3, nblocks - c2 - 3]))
    got = np.concatenate(got, axis=1)
    gg.same(got[:, (c + fade) * pts0:], want[:, (c + fade) * pts0:], "a plain push after the fade")


def test_a_second_fade():
    pts0, pts1, n1, channels = 32, 256, 3, 3
    hA, hB, hC, x = _signals(pts0, pts1, n1, channels)
    yA, yB, yC = (_plain(pts0, pts1, n1, channels, k) for k in range(3))
    m = pts1 // pts0
    c1, f1, f2 = 2 * m + 1, m + 1, 2 * m + 3
    c2 = c1 + f1 + m + 2                         # inside a period, a few blocks after the first fade's end
    nblocks = c2 + f2 + (n1 + 4) * m
    L = nblocks * pts0
    assert L <= x.shape[1]
    want = _mixed(_mixed(yA[:, :L], yB[:, :L], c1, f1, pts0), yC[:, :L], c2, f2, pts0)
    p = _object(pts0, pts1, n1, channels, hA)
    first = _faded(p, x, c1, hB, f1, "odd", c2 - 2)
    state = p.state_bytes()
    second = _faded(p, x, c2, hC, f2, "one", nblocks)
    assert p.state_bytes() == state              # the second set is kept for the next fade
    gg.same(np.concatenate([first, second], axis=1), want, "A to B, then B to C")
    assert not np.array_equal(yB[:, (c2 + f2) * pts0:L], yC[:, (c2 + f2) * pts0:L])


def test_refusals_leave_the_state_untouched():
    pts0, pts1, n1, channels = 32, 64, 1, 3
    hA, hB, hC, x = _signals(pts0, pts1, n1, channels)
    m = pts1 // pts0
    c, fade = 2 * m + 1, 2 * m + 3
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    want = _mixed(_plain(pts0, pts1, n1, channels, 0)[:, :L], _plain(pts0, pts1, n1, channels, 1)[:, :L], c, fade, pts0)
    need = 2 * pts1 + n1 * pts1
    p = _object(pts0, pts1, n1, channels, hA)
    got = [_run(p, x[:, :c * pts0], [c])]
    rows = _device_rows(hC, need)
    stream = torch.cuda.current_stream().cuda_stream
    # the arguments: the fade length, then those of push_ir_dev
    for blocks in (0, -1, (2 ** 31 - 1) // pts0 + 1):
        assert p.push_ir_fade_device(rows.data, blocks) == CL_INVALID_VALUE
        assert p.push_ir_fade(hC, blocks) == CL_INVALID_VALUE
    assert p.push_ir_fade_device(rows.data[:, :need - 1], 3) == CL_INVALID_VALUE
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
        rc = p.push_ir_fade_device(rows.data, 3, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert p.fade_remaining() == 0 and p.position == c
    # the fade, and one block of it
    rowsB = _device_rows(hB, need)
    assert p.push_ir_fade_device(rowsB.data, fade) == 0
    got.append(_run(p, x[:, c * pts0:(c + 1) * pts0], [1]))
    # while it is pending: no other push, no reset
    assert p.push_ir_fade_device(rows.data, 3) == CL_INVALID_OPERATION
    assert p.push_ir_fade(hC, 3) == CL_INVALID_OPERATION
    assert p.push_ir_device(rows.data) == CL_INVALID_OPERATION
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


@pytest.mark.parametrize("pts0,pts1,n1", GEOMS)
def test_against_float64(pts0, pts1, n1):
    """the float64 model of the schedule (tests/nupconv_fade_model.py) over the whole signal at the project's parity
    criterion, tests/util.TOL; the fade segment's figures are printed"""
    channels = 3
    hA, hB, _, x = _signals(pts0, pts1, n1, channels)
    m = pts1 // pts0
    c, fade = 2 * m + m - 1, m + 1
    nblocks = c + fade + (n1 + 4) * m
    L = nblocks * pts0
    got = _faded(_object(pts0, pts1, n1, channels, hA), x, c, hB, fade, "one", nblocks)
    model = NupFadeModel(_cvs(pts1, n1), pts0, pts1, channels)
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
