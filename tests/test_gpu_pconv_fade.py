"""Timed crossfade of the convolution matrix (PconvMatrix.push_ir_fade / push_ir_fade_device): equality with the
definition (two objects fed alike, mixed by g) and with the float64 model, the bits of a plain push after the fade, a fade
to the same responses, bit identity across splits / sub-batch caps / streams, the host form and layouts, the refusals, and
a graph captured before a fade replayed after it."""
import numpy as np
import pytest

import opencl_fft_amd as fa
from tests.pconv_fade_model import FadeModel, ramp
from tests.util import assert_parity

pytestmark = pytest.mark.gpu

CTOL = 1e-6   # this object's tolerance against its composition (tests/test_gpu_pconv_matrix.py); the mix is a convex
              # combination of two such outputs
CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
T_PUSH = 7    # blocks before the push: the ring has wrapped at nparts 5

GEOMS = [  # inputs, outputs, pts, nparts
    (1, 1, 32, 1),       # smallest everything; the prime reads one frame
    (3, 2, 64, 5),       # one segment
    (16, 2, 512, 20),    # 20 segments, tile 4
    (4, 4, 4096, 8),     # largest transform, tile 16
    (3, 5, 256, 12),     # the segments x tile sweep below
]
SWEEP = [(segs, tile) for segs in ("1", "3") for tile in ("4", "16")]


def _torch():
    import torch
    return torch


def _fades(nparts):
    return (1, 4, nparts + 3)


def _data(I, O, pts, nparts, nblocks, seed):
    rng = np.random.default_rng(seed)
    ha = rng.random((O, I, pts * nparts), dtype=np.float32) - 0.5
    hb = rng.random((O, I, pts * nparts), dtype=np.float32) - 0.5
    x = _torch().from_numpy(rng.random((I, nblocks * pts), dtype=np.float32) - 0.5).cuda()
    return ha, hb, x


def _matrix(I, O, pts, nparts, ir):
    m = fa.PconvMatrix(0, pts * nparts, pts, I, O)
    assert m.get_error() == 0, m.get_log()
    assert m.push_ir(ir) == 0
    return m


def _calls(m, out, x, pts, j, splits, stream=None):
    for n in splits:
        sl = slice(j * pts, (j + n) * pts)
        assert m.process_device(out[:, sl], x[:, sl], stream=stream) == 0
        j += n
    return j


def _plain(geom, ir, x):
    """an object holding ir for the whole signal"""
    torch = _torch()
    I, O, pts, nparts = geom
    m = _matrix(I, O, pts, nparts, ir)
    out = torch.empty((O, x.shape[1]), device="cuda")
    assert m.process_device(out, x) == 0
    torch.cuda.synchronize()
    return out


def _faded(geom, ha, hb, x, fade_blocks, splits, stream=None, host=False):
    """A for T_PUSH blocks, the fade push of hb, the rest of x in calls of `splits` blocks"""
    torch = _torch()
    I, O, pts, nparts = geom
    torch.cuda.synchronize()
    m = _matrix(I, O, pts, nparts, ha)
    out = torch.empty((O, x.shape[1]), device="cuda")
    _calls(m, out, x, pts, 0, [T_PUSH], stream)
    if host:
        torch.cuda.synchronize()
        assert m.push_ir_fade(hb, fade_blocks) == 0
    else:
        assert m.push_ir_fade_device(torch.from_numpy(hb).cuda(), fade_blocks, stream=stream) == 0
    assert m.fade_remaining() == fade_blocks
    j = _calls(m, out, x, pts, T_PUSH, splits, stream)
    assert j * pts == x.shape[1]
    torch.cuda.synchronize()
    assert m.fade_remaining() == 0
    return out


def _two_calls(fade_blocks):
    """the rest in two calls: the second one starts inside the fade and ends after it (a one-block fade lies inside the
    first call, which is then cut in the middle)"""
    k1 = 3 if fade_blocks == 1 else fade_blocks // 2
    return [k1, fade_blocks + 6 - k1]


def _check_definition(geom, fade_blocks, seed):
    I, O, pts, nparts = geom
    nblocks = T_PUSH + fade_blocks + 6
    ha, hb, x = _data(I, O, pts, nparts, nblocks, seed)
    got = _faded(geom, ha, hb, x, fade_blocks, _two_calls(fade_blocks)).cpu().numpy()
    ya = _plain(geom, ha, x).cpu().numpy().astype(np.float64)
    yb = _plain(geom, hb, x).cpu().numpy().astype(np.float64)
    n0, N = T_PUSH * pts, fade_blocks * pts
    want = ya.copy()
    want[:, n0:n0 + N] = ya[:, n0:n0 + N] + ramp(0, N, N) * (yb[:, n0:n0 + N] - ya[:, n0:n0 + N])
    want[:, n0 + N:] = yb[:, n0 + N:]
    model = FadeModel(nparts, pts, I, O, cap=nblocks)
    model.push_ir(ha.astype(np.float64))
    xn = x.cpu().numpy().astype(np.float64)
    ym = [model.process(xn[:, :n0])]
    model.push_ir_fade(hb.astype(np.float64), fade_blocks)
    ym.append(model.process(xn[:, n0:]))
    ym = np.concatenate(ym, axis=1)
    for o in range(O):
        for name, ref in (("objects mixed by g", want), ("float64 model", ym)):
            for part, sl in (("before", slice(0, n0)), ("fade", slice(n0, n0 + N)), ("after", slice(n0 + N, None))):
                l2, mx = assert_parity(got[o, sl], ref[o, sl], tol=CTOL * I, what="output %d %s, %s" % (o, part, name))
                print("%s fade %d output %d %s vs %s: relL2 %.3g max %.3g" % (geom, fade_blocks, o, part, name, l2, mx))
    # outside the fade the bits are those of the object that holds A, then of the one that holds B
    assert np.array_equal(got[:, :n0], ya[:, :n0].astype(np.float32))
    assert np.array_equal(got[:, n0 + N:], yb[:, n0 + N:].astype(np.float32))


@pytest.mark.parametrize("geom", GEOMS[:4])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_equals_the_definition(geom, which):
    _check_definition(geom, _fades(geom[3])[which], seed=sum(geom) + which)


@pytest.mark.parametrize("segs,tile", SWEEP)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_equals_the_definition_every_instantiation(monkeypatch, segs, tile, which):
    monkeypatch.setenv("CLFA_PCONV_MATRIX_SEGS", segs)
    monkeypatch.setenv("CLFA_PCONV_MATRIX_TILE", tile)
    _check_definition(GEOMS[4], _fades(GEOMS[4][3])[which], seed=int(segs) * 10 + int(tile) + which)


@pytest.mark.parametrize("geom", GEOMS)
def test_after_the_fade_the_bits_of_a_plain_push(geom):
    torch = _torch()
    I, O, pts, nparts = geom
    for fade_blocks in (1, nparts + 3):
        nblocks = T_PUSH + fade_blocks + 6
        ha, hb, x = _data(I, O, pts, nparts, nblocks, seed=sum(geom) + fade_blocks)
        hd = torch.from_numpy(hb).cuda()
        m, q = _matrix(I, O, pts, nparts, ha), _matrix(I, O, pts, nparts, ha)
        om, oq = torch.empty((O, nblocks * pts), device="cuda"), torch.empty((O, nblocks * pts), device="cuda")
        for obj, out in ((m, om), (q, oq)):
            _calls(obj, out, x, pts, 0, [T_PUSH])
        assert q.push_ir_device(hd) == 0 and q.fade_remaining() == 0
        assert m.push_ir_fade_device(hd, fade_blocks) == 0
        state, work = m.state_bytes(), m.workspace_bytes()
        assert state > q.state_bytes()   # the second responses and tails are counted once they exist
        for k in range(fade_blocks):     # block by block: the count goes down to 0
            assert m.fade_remaining() == fade_blocks - k
            _calls(m, om, x, pts, T_PUSH + k, [1])
        assert m.fade_remaining() == 0
        _calls(m, om, x, pts, T_PUSH + fade_blocks, [6])
        _calls(q, oq, x, pts, T_PUSH, [fade_blocks + 6])
        torch.cuda.synchronize()
        first = (T_PUSH + fade_blocks) * pts
        assert torch.equal(om[:, first:], oq[:, first:]), "fade of %d blocks" % fade_blocks
        assert torch.equal(om[:, :T_PUSH * pts], oq[:, :T_PUSH * pts])
        assert not torch.equal(om[:, T_PUSH * pts:first], oq[:, T_PUSH * pts:first])
        assert (m.state_bytes(), m.workspace_bytes()) == (state, work)
        # a second fade on the same object allocates nothing more
        assert m.push_ir_fade_device(torch.from_numpy(ha).cuda(), 2) == 0
        assert (m.state_bytes(), m.workspace_bytes()) == (state, work)


def _check_same_responses(geom, seed):
    torch = _torch()
    I, O, pts, nparts = geom
    fade_blocks = nparts + 3
    nblocks = T_PUSH + fade_blocks + 6
    ha, _, x = _data(I, O, pts, nparts, nblocks, seed)
    got = _faded(geom, ha, ha, x, fade_blocks, _two_calls(fade_blocks))
    assert torch.equal(got, _plain(geom, ha, x))


@pytest.mark.parametrize("geom", GEOMS[:4])
def test_a_fade_to_the_same_responses_changes_nothing(geom):
    _check_same_responses(geom, seed=sum(geom))


@pytest.mark.parametrize("segs,tile", SWEEP)
def test_a_fade_to_the_same_responses_every_instantiation(monkeypatch, segs, tile):
    monkeypatch.setenv("CLFA_PCONV_MATRIX_SEGS", segs)
    monkeypatch.setenv("CLFA_PCONV_MATRIX_TILE", tile)
    _check_same_responses(GEOMS[4], seed=int(segs) + int(tile))


@pytest.mark.parametrize("geom", [GEOMS[4], GEOMS[2]])
def test_bit_identity_inside_the_fade(monkeypatch, geom):
    torch = _torch()
    I, O, pts, nparts = geom
    fade_blocks = nparts + 3
    rest = fade_blocks + 6
    ha, hb, x = _data(I, O, pts, nparts, T_PUSH + rest, seed=sum(geom))
    ref = _faded(geom, ha, hb, x, fade_blocks, [rest])
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(1, rest), size=4, replace=False))
    for sp in ([1] * rest, [int(v) for v in np.diff(np.concatenate([[0], cuts, [rest]]))]):
        assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, sp), ref), "split %s" % (sp[:8],)
    for cap in ("1", "3"):
        monkeypatch.setenv("CLFA_PCONV_MATRIX_BLOCKS_MAX", cap)
        assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, [rest]), ref), "cap %s" % cap
        assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, [5, rest - 5]), ref), "cap %s split" % cap
    monkeypatch.delenv("CLFA_PCONV_MATRIX_BLOCKS_MAX")
    side = torch.cuda.Stream()
    assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, [4, rest - 4], stream=side.cuda_stream), ref), "second stream"
    # the two-launch form of the fade's multiply-accumulate (tuning switch) sums in the same order
    monkeypatch.setenv("CLFA_PCONV_MATRIX_FADE_MAC", "two")
    assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, [rest]), ref), "two MAC launches"


def test_host_form_and_layouts():
    torch = _torch()
    geom = I, O, pts, nparts = GEOMS[1]
    fade_blocks = 4
    rest = fade_blocks + 6
    ha, hb, x = _data(I, O, pts, nparts, T_PUSH + rest, seed=5)
    ref = _faded(geom, ha, hb, x, fade_blocks, _two_calls(fade_blocks))
    assert torch.equal(_faded(geom, ha, hb, x, fade_blocks, _two_calls(fade_blocks), host=True), ref)
    # rows at a longer stride, one float off the 8-byte grid
    big = torch.zeros((O, I, pts * nparts + 5), device="cuda")
    big[:, :, 1:1 + pts * nparts] = torch.from_numpy(hb).cuda()
    view = big[:, :, 1:1 + pts * nparts]
    assert view.data_ptr() % 8 == 4
    m = _matrix(I, O, pts, nparts, ha)
    out = torch.empty_like(ref)
    _calls(m, out, x, pts, 0, [T_PUSH])
    assert m.push_ir_fade_device(view, fade_blocks) == 0
    _calls(m, out, x, pts, T_PUSH, [rest])
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    # the shape checks of push_ir / push_ir_device
    assert m.push_ir_fade(hb[:, :, :-1], 2) == CL_INVALID_VALUE
    assert m.push_ir_fade(hb[:1], 2) == CL_INVALID_VALUE
    assert m.push_ir_fade_device(torch.from_numpy(hb).cuda()[:, :, :-1], 2) == CL_INVALID_VALUE
    assert m.push_ir_fade_device(torch.from_numpy(hb).cuda().double(), 2) == CL_INVALID_VALUE
    assert m.fade_remaining() == 0


def test_refusals_leave_the_state_untouched():
    torch = _torch()
    I, O, pts, nparts = GEOMS[1]
    fade_blocks, rest = 4, 10
    ha, hb, x = _data(I, O, pts, nparts, T_PUSH + rest, seed=6)
    hd = torch.from_numpy(hb).cuda()
    other = torch.from_numpy(ha[::-1].copy()).cuda()
    m, q = _matrix(I, O, pts, nparts, ha), _matrix(I, O, pts, nparts, ha)   # q: the undisturbed run
    om, oq = torch.empty((O, x.shape[1]), device="cuda"), torch.empty((O, x.shape[1]), device="cuda")
    for obj, out in ((m, om), (q, oq)):
        _calls(obj, out, x, pts, 0, [T_PUSH])
    # bad arguments: nothing pending afterwards
    assert m.push_ir_fade_device(hd, 0) == CL_INVALID_VALUE
    assert m.push_ir_fade_device(hd, -3) == CL_INVALID_VALUE
    assert m.push_ir_fade(hb, 0) == CL_INVALID_VALUE
    assert m.fade_remaining() == 0
    # a fade push under capture allocates: refused, the capture ends normally
    dummy = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = m.push_ir_fade_device(hd, fade_blocks, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION and m.fade_remaining() == 0
    torch.cuda.synchronize()
    state = m.state_bytes()
    assert state == q.state_bytes()
    # the fade, two blocks of it, then every push is refused
    for obj, out in ((m, om), (q, oq)):
        assert obj.push_ir_fade_device(hd, fade_blocks) == 0
        _calls(obj, out, x, pts, T_PUSH, [2])
    assert m.push_ir_fade_device(other, 3) == CL_INVALID_OPERATION
    assert m.push_ir_fade(ha, 3) == CL_INVALID_OPERATION
    assert m.push_ir_device(other) == CL_INVALID_OPERATION
    assert m.push_ir(ha) == CL_INVALID_OPERATION
    assert m.fade_remaining() == fade_blocks - 2
    # process under capture inside the fade: its progress is host state
    sl = slice((T_PUSH + 2) * pts, None)
    xs = x[:, sl].contiguous()
    scratch = torch.full((O, xs.shape[1]), 3.0, device="cuda")
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        rc = m.process_device(scratch, xs, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION and m.fade_remaining() == fade_blocks - 2
    torch.cuda.synchronize()
    assert bool((scratch == 3.0).all())
    # the remaining blocks equal the undisturbed run's
    for obj, out in ((m, om), (q, oq)):
        _calls(obj, out, x, pts, T_PUSH + 2, [rest - 2])
    torch.cuda.synchronize()
    assert torch.equal(om, oq)
    assert m.fade_remaining() == 0 and m.push_ir_device(other) == 0   # a plain push with no fade pending: as ever


def test_a_graph_captured_before_a_fade_is_valid_after_it():
    """every call is a multiple of nparts blocks, so the ring position a captured call carries stays the object's"""
    torch = _torch()
    I, O, pts, nparts = GEOMS[1]
    K = nparts
    ha, hb, x = _data(I, O, pts, nparts, 5 * K, seed=8)
    hd = torch.from_numpy(hb).cuda()
    m, q = _matrix(I, O, pts, nparts, ha), _matrix(I, O, pts, nparts, ha)
    blk = lambda k: x[:, k * K * pts:(k + 1) * K * pts]
    xg = blk(1).clone()
    og, oq, tmp = (torch.empty((O, K * pts), device="cuda") for _ in range(3))
    for obj in (m, q):
        assert obj.process_device(tmp, blk(0)) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert m.process_device(og, xg, stream=torch.cuda.current_stream().cuda_stream) == 0
    g.replay()
    assert q.process_device(oq, blk(1)) == 0
    torch.cuda.synchronize()
    assert torch.equal(og, oq)
    addresses = (m.state_bytes(), m.workspace_bytes())
    for obj in (m, q):   # a whole fade outside the graph
        assert obj.push_ir_fade_device(hd, K) == 0
        assert obj.process_device(tmp, blk(2)) == 0
        assert obj.fade_remaining() == 0
    assert m.workspace_bytes() > addresses[1]
    for k in (3, 4):     # the old graph, new input: the responses, rings and tails it reads are the object's still
        xg.copy_(blk(k))
        g.replay()
        assert q.process_device(oq, blk(k)) == 0
        torch.cuda.synchronize()
        assert torch.equal(og, oq), "replay %d after the fade" % k
    want = _plain((I, O, pts, nparts), hb, x)
    assert torch.equal(og, want[:, 4 * K * pts:])   # and they are B's: two calls after the fade nothing of A is left
