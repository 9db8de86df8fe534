"""Convolution matrix (PconvMatrix, clfa_pconv_matrix): equality with the Clpconv composition, accuracy against float64,
bit identity across splits / sub-batches / streams / graph replay, state across pushes, layouts and errors."""
import ctypes as C

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from tests import util
from tests.util import assert_parity
from tests.pconv_matrix_model import truth_with_push

pytestmark = pytest.mark.gpu

CTOL = 1e-6   # the single-block parity tolerance (tests/test_gpu_conv.py)
CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59


def _torch():
    import torch
    return torch


def _sig(rng, rows, n):
    return _torch().from_numpy((rng.random((rows, n), dtype=np.float32) - 0.5)).cuda()


def _ir(rng, O, I, n):
    return rng.random((O, I, n), dtype=np.float32) - 0.5


def _matrix(pts, nparts, I, O, ir):
    m = fa.PconvMatrix(0, pts * nparts, pts, I, O)
    assert m.get_error() == 0, m.get_log()
    assert m.nparts == nparts and m.kernel_name() == "k_pconvm_mac"
    assert m.push_ir(ir) == 0
    return m


def _composition(pts, nparts, I, O, ir):
    """Clpconv(channels = O*I), channel o*I + i holding h_{o,i}"""
    p = fa.Clpconv(0, pts * nparts, pts, channels=O * I)
    assert p.get_cl_err() == 0 and p.push_ir(ir.reshape(O * I, -1)) == 0
    return p


def _compose_blocks(p, x, O, I):
    """every input copied O times -> process_blocks_device -> (O*I, L) float32 per-pair outputs"""
    torch = _torch()
    xin = x.unsqueeze(0).expand(O, I, x.shape[1]).reshape(O * I, x.shape[1]).contiguous()
    y = torch.empty_like(xin)
    assert p.process_blocks_device(y, xin) == 0
    return y


CASES = [  # inputs, outputs, pts, nparts
    (1, 1, 32, 1), (1, 1, 64, 3), (1, 1, 1024, 94),
    (16, 2, 512, 94), (16, 2, 64, 3), (16, 2, 4096, 3),
    (2, 16, 32, 3), (2, 16, 1024, 1), (2, 16, 4096, 94),
    (4, 4, 64, 94), (4, 4, 512, 1), (4, 4, 1024, 3),
    (3, 5, 32, 94), (3, 5, 4096, 1), (3, 5, 512, 3),
]


@pytest.mark.parametrize("I,O,pts,nparts", CASES)
def test_equals_the_composition(I, O, pts, nparts):
    torch = _torch()
    rng = np.random.default_rng(I * 1000 + O * 100 + pts + nparts)
    ir = _ir(rng, O, I, pts * nparts)
    m, p = _matrix(pts, nparts, I, O, ir), _composition(pts, nparts, I, O, ir)
    assert m.workspace_bytes() == 0
    for nb in (2, nparts + 3):   # two calls; the second wraps the rings
        x = _sig(rng, I, nb * pts)
        got = torch.empty((O, nb * pts), device="cuda")
        assert m.process_device(got, x) == 0
        pairs = _compose_blocks(p, x, O, I)
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        want = pairs.cpu().numpy().astype(np.float64).reshape(O, I, -1).sum(axis=1)
        for o in range(O):
            assert_parity(g[o], want[o], tol=CTOL * I, what="output %d, %d blocks" % (o, nb))
        if I == 1 and O == 1:
            w32 = pairs.cpu().numpy()
            assert_parity(g, w32, tol=CTOL, what="one pair vs Clpconv")
            print("(1,1) pts %d nparts %d: bit-identical to Clpconv blocks: %s" % (pts, nparts, np.array_equal(g, w32)))
    assert m.workspace_bytes() > 0
    assert m.state_bytes() >= 8 * pts * nparts * (O * I + I)


def test_accuracy_config4_geometry():
    """16 -> 2 at pts 1024, 94 partitions, 110 blocks: against sum_i pconv_f64, relL2 and max error within 1.2 x those of
    the float32 composition (Clpconv per pair, then a float32 sum over the inputs)"""
    torch = _torch()
    I, O, pts, nparts, nb = 16, 2, 1024, 94, 110
    rng = np.random.default_rng(11)
    ir = _ir(rng, O, I, pts * nparts)
    m, p = _matrix(pts, nparts, I, O, ir), _composition(pts, nparts, I, O, ir)
    x = _sig(rng, I, nb * pts)
    got = torch.empty((O, nb * pts), device="cuda")
    assert m.process_device(got, x) == 0
    comp = _compose_blocks(p, x, O, I).reshape(O, I, -1).sum(dim=1)
    torch.cuda.synchronize()
    xn, g, c = x.cpu().numpy().astype(np.float64), got.cpu().numpy(), comp.cpu().numpy()
    for o in range(O):
        truth = sum(util.pconv_f64(ir[o, i].astype(np.float64), xn[i], pts) for i in range(I))
        em, ec = util.rel_err(g[o], truth), util.rel_err(c[o], truth)
        print("output %d: matrix relL2 %.3g max %.3g; composition relL2 %.3g max %.3g" % (o, em[0], em[1], ec[0], ec[1]))
        assert em[0] <= 1.2 * ec[0] and em[1] <= 1.2 * ec[1], (em, ec)


def _run(pts, nparts, I, O, ir, x, splits, stream=None):
    torch = _torch()
    torch.cuda.synchronize()
    m = _matrix(pts, nparts, I, O, ir)
    out = torch.empty((O, x.shape[1]), device="cuda")
    j = 0
    for n in splits:
        sl = slice(j * pts, (j + n) * pts)
        assert m.process_device(out[:, sl], x[:, sl], stream=stream) == 0
        j += n
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("I,O,pts,nparts", [(3, 5, 256, 12), (16, 2, 512, 20), (4, 4, 64, 3)])
def test_bit_identity(monkeypatch, I, O, pts, nparts):
    torch = _torch()
    rng = np.random.default_rng(I + O + pts + nparts)
    ir = _ir(rng, O, I, pts * nparts)
    N = 100
    x = _sig(rng, I, N * pts)
    ref = _run(pts, nparts, I, O, ir, x, [N])
    cuts = np.sort(rng.choice(np.arange(1, N), size=6, replace=False))
    for sp in ([1] * N, [37, 63], [1, 99], list(np.diff(np.concatenate([[0], cuts, [N]])))):
        got = _run(pts, nparts, I, O, ir, x, [int(v) for v in sp])
        assert torch.equal(got, ref), "split %s" % (sp[:8],)
    for cap in ("1", "3"):
        monkeypatch.setenv("CLFA_PCONV_MATRIX_BLOCKS_MAX", cap)
        assert torch.equal(_run(pts, nparts, I, O, ir, x, [N]), ref), "cap %s" % cap
        assert torch.equal(_run(pts, nparts, I, O, ir, x, [5, N - 5]), ref), "cap %s split" % cap
    monkeypatch.delenv("CLFA_PCONV_MATRIX_BLOCKS_MAX")
    side = torch.cuda.Stream()
    assert torch.equal(_run(pts, nparts, I, O, ir, x, [50, 50], stream=side.cuda_stream), ref), "second stream"
    # graph replay: two objects warmed alike, the second's next call captured and replayed
    n0 = 40
    objs = []
    for _ in range(2):
        m = _matrix(pts, nparts, I, O, ir)
        warm = torch.empty((O, n0 * pts), device="cuda")
        assert m.process_device(warm, x[:, :n0 * pts]) == 0
        objs.append(m)
    torch.cuda.synchronize()
    sl = slice(n0 * pts, N * pts)
    direct = torch.empty((O, (N - n0) * pts), device="cuda")
    assert objs[0].process_device(direct, x[:, sl]) == 0
    torch.cuda.synchronize()
    x1 = x[:, sl].contiguous()
    replayed = torch.empty_like(direct)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert objs[1].process_device(replayed, x1, stream=torch.cuda.current_stream().cuda_stream) == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(direct, replayed)
    assert torch.equal(direct, ref[:, sl])


def test_push_between_calls_keeps_history():
    torch = _torch()
    I, O, pts, nparts = 3, 2, 64, 5
    rng = np.random.default_rng(21)
    h1, h2 = _ir(rng, O, I, pts * nparts), _ir(rng, O, I, pts * nparts)
    x = _sig(rng, I, 19 * pts)
    m = _matrix(pts, nparts, I, O, h1)
    out = torch.empty((O, 19 * pts), device="cuda")
    assert m.process_device(out[:, :7 * pts], x[:, :7 * pts]) == 0
    hd = torch.from_numpy(h2).cuda()
    assert m.push_ir_device(hd) == 0
    assert m.process_device(out[:, 7 * pts:], x[:, 7 * pts:]) == 0
    torch.cuda.synchronize()
    want = truth_with_push(h1, h2, 7, x.cpu().numpy(), pts)
    for o in range(O):
        assert_parity(out[o].cpu().numpy(), want[o], tol=CTOL * I, what="output %d" % o)
    # the host push gives the same bits as the device push
    m2 = _matrix(pts, nparts, I, O, h1)
    out2 = torch.empty_like(out)
    assert m2.process_device(out2[:, :7 * pts], x[:, :7 * pts]) == 0
    torch.cuda.synchronize()
    assert m2.push_ir(h2) == 0
    assert m2.process_device(out2[:, 7 * pts:], x[:, 7 * pts:]) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out2)


@pytest.mark.parametrize("pts", [32, 1024])
def test_layouts_strides_offsets_and_host_form(pts):
    torch = _torch()
    I, O, nparts, nb = 3, 2, 5, 13
    L = nb * pts
    rng = np.random.default_rng(pts)
    ir = _ir(rng, O, I, pts * nparts)
    x = _sig(rng, I, L)
    ref = _run(pts, nparts, I, O, ir, x, [nb])
    for off, extra in ((0, 6), (1, 7), (1, 0)):
        big_x = torch.zeros((I, L + extra + off), device="cuda")
        big_x[:, off:off + L] = x
        vx = big_x[:, off:off + L]
        big_o = torch.full((O, L + extra + 3), 7.0, device="cuda")
        o_off = 1 if off else 2
        vo = big_o[:, o_off:o_off + L]
        m = _matrix(pts, nparts, I, O, ir)
        assert m.process_device(vo, vx) == 0
        torch.cuda.synchronize()
        assert torch.equal(vo, ref), "offset %d extra %d" % (off, extra)
        rest = big_o.clone()
        rest[:, o_off:o_off + L] = 7.0
        assert bool((rest == 7.0).all()), "wrote outside the rows"
    # responses at a longer row stride, one float off the 8-byte grid
    big_h = torch.zeros((O, I, pts * nparts + 5), device="cuda")
    big_h[:, :, 1:1 + pts * nparts] = torch.from_numpy(ir).cuda()
    m = fa.PconvMatrix(0, pts * nparts, pts, I, O)
    assert m.push_ir_device(big_h[:, :, 1:1 + pts * nparts]) == 0
    o2 = torch.empty((O, L), device="cuda")
    assert m.process_device(o2, x) == 0
    torch.cuda.synchronize()
    assert torch.equal(o2, ref)
    # host form
    m = _matrix(pts, nparts, I, O, ir)
    out = np.zeros((O, L), np.float32)
    assert m.convolution(out, x.cpu().numpy()) == 0
    assert np.array_equal(out, ref.cpu().numpy())


def test_errors_leave_the_state_untouched():
    torch = _torch()
    I, O, pts, nparts, nb = 2, 3, 64, 4, 6
    rng = np.random.default_rng(5)
    ir = _ir(rng, O, I, pts * nparts)
    m, q = _matrix(pts, nparts, I, O, ir), _matrix(pts, nparts, I, O, ir)
    row = 3 * nb * pts
    buf = _sig(rng, 4, row)
    keep = buf.clone()
    L = C.c_long
    f = lib().clfa_pconv_matrix_process_dev
    s = torch.cuda.current_stream().cuda_stream
    base = buf.data_ptr()
    n = nb * pts
    cases = [
        # out overlaps in: whole, one float at the end of in's last row, one float of out's last row in in's first row
        (base, row, base, row, nb),
        (base + 4 * (row + n - 1), row, base, row, nb),
        (base - 4 * (2 * row + n - 1), row, base, row, nb),
        (base + 4 * (n - 1), row, base, row, nb),    # out's first float = in's last float of row 0
        # short strides, negative counts, misaligned, NULL
        (base + 4 * n, n - 1, base, row, nb),
        (base + 4 * n, row, base, n - 1, nb),
        (base + 4 * n, row, base, row, -1),
        (base + 4 * n + 2, row, base, row, nb),
        (base + 4 * n, row, base + 2, row, nb),
        (None, row, base, row, nb),
        (base + 4 * n, row, None, row, nb),
    ]
    for o, os_, i, is_, k in cases:
        assert f(m._h, o, L(os_), i, L(is_), L(k), s) == CL_INVALID_VALUE, (o, os_, i, is_, k)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    assert m.workspace_bytes() == 0
    assert f(m._h, base, L(row), base, L(row), L(0), s) == 0   # nblocks == 0: nothing happens
    # bad shapes and sizes through Python
    x = _sig(rng, I, nb * pts)
    assert m.process_device(torch.empty((O, nb * pts - 1), device="cuda"), x) == CL_INVALID_VALUE
    assert m.process_device(torch.empty((O, 5), device="cuda"), x[:, :5]) == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        m.process_device(torch.empty((O + 1, nb * pts), device="cuda"), x)
    assert m.push_ir(ir[:, :, :-1]) == CL_INVALID_VALUE
    assert m.push_ir(ir[:1]) == CL_INVALID_VALUE
    assert m.convolution(np.zeros((O, nb * pts + 1), np.float32), x.cpu().numpy()) == CL_INVALID_VALUE
    assert lib().clfa_pconv_matrix_push_ir_dev(m._h, base, L(pts * nparts - 1), s) == CL_INVALID_VALUE
    # allocation under capture: CL_INVALID_OPERATION, nothing moves
    out = torch.full((O, nb * pts), 3.0, device="cuda")
    dummy = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = m.process_device(out, x, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and m.workspace_bytes() == 0
    # the next call equals the one of an object that never saw the bad calls
    o1, o2 = torch.empty((O, nb * pts), device="cuda"), torch.empty((O, nb * pts), device="cuda")
    assert m.process_device(o1, x) == 0 and q.process_device(o2, x) == 0
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)
    # creation outside 32..4096, and a failed object returns its error
    for bad_pts in (16, 8192):
        b = fa.PconvMatrix(0, 4 * bad_pts, bad_pts, 2, 2)
        assert b.get_error() == CL_INVALID_VALUE
        assert f(b._h, base, L(row), base, L(row), L(1), s) == CL_INVALID_VALUE
