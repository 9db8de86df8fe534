"""Multi-block partitioned convolution (clfa_pconv_process_blocks_dev): equivalence to the single-block calls and the
oracle, bit-identity across splits / streams / graph replay / sub-batches, layouts, errors and accuracy."""
import ctypes as C

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from oracle import oracle
from tests import util
from tests.util import assert_parity

pytestmark = pytest.mark.gpu

CTOL = 1e-6   # the single-block parity tolerance (tests/test_gpu_conv.py)
CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59


def _torch():
    import torch
    return torch


def _sig(rng, ch, n):
    return _torch().from_numpy((rng.random((ch, n), dtype=np.float32) - 0.5)).cuda()


def _loop(p, out, in1, in2, nblocks, pts):
    """nblocks single-block process_device calls: the definition of a multi-block call"""
    torch = _torch()
    for j in range(nblocks):
        o = torch.empty((p.channels, pts), device="cuda")
        a = in1[:, j * pts:(j + 1) * pts].contiguous()
        b = in2[:, j * pts:(j + 1) * pts].contiguous() if in2 is not None else None
        assert p.process_device(o, a, b) == 0
        out[:, j * pts:(j + 1) * pts] = o


def _pair(pts, nparts, ch, rng):
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    p, q = fa.Clpconv(0, pts * nparts, pts, channels=ch), fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.get_cl_err() == 0 and q.get_cl_err() == 0
    assert p.push_ir(ir) == 0 and q.push_ir(ir) == 0
    return p, q, ir


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("nparts", [1, 3, 94])
@pytest.mark.parametrize("pts,ch", [(8, 3), (32, 1), (64, 3), (128, 3), (256, 1), (512, 1), (1024, 3), (2048, 3), (4096, 1),
                                    (8192, 1)])
def test_blocks_equal_the_single_block_loop(pts, ch, nparts, tv):
    torch = _torch()
    rng = np.random.default_rng(pts * 1000 + nparts * 10 + tv)
    p, q, ir = _pair(pts, nparts, ch, rng)
    assert p.blocks_kernel_name() == ("k_pconvb_mac" if 32 <= pts <= 4096 else "loop")
    assert p.blocks_workspace_bytes() == 0
    orc = []
    for c in range(ch):
        o = oracle.Pconv(pts * nparts, pts)
        o.push_ir(ir[c])
        orc.append(o)
    counts = [n for n in (1, nparts - 1, nparts, 3 * nparts + 5) if n > 0]
    for step, nb in enumerate(counts):
        if step == 2:   # a new response between calls: push_ir mixes with multi-block calls
            ir2 = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
            assert p.push_ir(ir2) == 0 and q.push_ir(ir2) == 0
            for c in range(ch):
                orc[c].push_ir(ir2[c])
        a = _sig(rng, ch, nb * pts)
        b = _sig(rng, ch, nb * pts) if tv else None
        got = torch.empty_like(a)
        want = torch.empty_like(a)
        assert p.process_blocks_device(got, a, b) == 0
        _loop(q, want, a, b, nb, pts)
        torch.cuda.synchronize()
        assert (p.wp, p.wp2) == (q.wp, q.wp2)
        g, w = got.cpu().numpy(), want.cpu().numpy()
        assert_parity(g, w, tol=CTOL, what="blocks vs loop, %d blocks" % nb)
        an, bn = a.cpu().numpy(), (b.cpu().numpy() if tv else None)
        for c in range(ch):
            ref = np.concatenate([orc[c].convolution(an[c, j * pts:(j + 1) * pts],
                                                     None if bn is None else bn[c, j * pts:(j + 1) * pts])
                                  for j in range(nb)])
            assert_parity(g[c], ref, tol=CTOL, what="blocks vs oracle, channel %d, %d blocks" % (c, nb))
        assert (p.wp, p.wp2) == (orc[0].wp, orc[0].wp2)
    assert p.blocks_workspace_bytes() > 0
    # the state left behind carries on in single-block calls
    for j in range(5):
        a = _sig(rng, ch, pts)
        b = _sig(rng, ch, pts) if tv else None
        o1, o2 = torch.empty_like(a), torch.empty_like(a)
        assert p.process_device(o1, a, b) == 0 and q.process_device(o2, a, b) == 0
        torch.cuda.synchronize()
        assert_parity(o1.cpu().numpy(), o2.cpu().numpy(), tol=CTOL, what="single block %d after" % j)
    assert (p.wp, p.wp2) == (q.wp, q.wp2)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
def test_blocks_config4_shape_equal_the_loop(tv):
    """256 channels, pts 1024, 94 partitions: the one-launch-per-block route of the benchmark (k_pconv_fused)"""
    torch = _torch()
    pts, nparts, ch = 1024, 94, 256
    rng = np.random.default_rng(4 + tv)
    p, q, _ = _pair(pts, nparts, ch, rng)
    for nb in (nparts - 1, 3 * nparts + 5):
        a = _sig(rng, ch, nb * pts)
        b = _sig(rng, ch, nb * pts) if tv else None
        got, want = torch.empty_like(a), torch.empty_like(a)
        assert p.process_blocks_device(got, a, b) == 0
        _loop(q, want, a, b, nb, pts)
        torch.cuda.synchronize()
        assert (p.wp, p.wp2) == (q.wp, q.wp2)
        g, w = got.cpu().numpy(), want.cpu().numpy()
        assert_parity(g, w, tol=CTOL, what="config 4 shape, %d blocks" % nb)
        print("config 4 shape %s, %d blocks: bit-identical to the loop: %s (max |d| %.3g)"
              % ("tv" if tv else "static", nb, np.array_equal(g, w), float(np.max(np.abs(g - w)))))


def _run_split(pts, nparts, ch, ir, a, b, splits, stream=None):
    torch = _torch()
    torch.cuda.synchronize()   # inputs made on the default stream
    p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.get_cl_err() == 0 and p.push_ir(ir) == 0
    out = torch.empty_like(a)
    j = 0
    for n in splits:
        sl = slice(j * pts, (j + n) * pts)
        assert p.process_blocks_device(out[:, sl], a[:, sl], b[:, sl] if b is not None else None, stream=stream) == 0
        j += n
    torch.cuda.synchronize()
    return out, (p.wp, p.wp2)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("pts,nparts,ch", [(64, 3, 2), (512, 128, 1), (1024, 94, 4)])
def test_split_invariance_bit_exact(pts, nparts, ch, tv):
    torch = _torch()
    rng = np.random.default_rng(pts + nparts + ch)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    N = 100
    a = _sig(rng, ch, N * pts)
    b = _sig(rng, ch, N * pts) if tv else None
    ref, st = _run_split(pts, nparts, ch, ir, a, b, [N])
    splits = [[37, 63], [1, 99], [1] * 10 + [90]]
    cuts = np.sort(rng.choice(np.arange(1, N), size=6, replace=False))
    splits.append(list(np.diff(np.concatenate([[0], cuts, [N]]))))
    for sp in splits:
        got, st2 = _run_split(pts, nparts, ch, ir, a, b, [int(x) for x in sp])
        assert st2 == st
        assert torch.equal(got, ref), "split %s" % (sp,)
    side = torch.cuda.Stream()
    got, _ = _run_split(pts, nparts, ch, ir, a, b, [50, 50], stream=side.cuda_stream)
    assert torch.equal(got, ref), "second stream"
    again, _ = _run_split(pts, nparts, ch, ir, a, b, [N])
    assert torch.equal(again, ref), "repeated call"


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
def test_graph_replay_bit_exact(tv):
    torch = _torch()
    pts, nparts, ch, n0, n1 = 256, 12, 3, 20, 17
    rng = np.random.default_rng(77 + tv)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    a = _sig(rng, ch, (n0 + n1) * pts)
    b = _sig(rng, ch, (n0 + n1) * pts) if tv else None
    objs = []
    for _ in range(2):
        p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
        assert p.push_ir(ir) == 0
        warm = torch.empty((ch, n0 * pts), device="cuda")
        assert p.process_blocks_device(warm, a[:, :n0 * pts], b[:, :n0 * pts] if tv else None) == 0   # warms the workspace
        objs.append(p)
    torch.cuda.synchronize()
    sl = slice(n0 * pts, (n0 + n1) * pts)
    direct = torch.empty((ch, n1 * pts), device="cuda")
    assert objs[0].process_blocks_device(direct, a[:, sl], b[:, sl] if tv else None) == 0
    torch.cuda.synchronize()
    a1 = a[:, sl].contiguous()
    b1 = b[:, sl].contiguous() if tv else None
    replayed = torch.empty((ch, n1 * pts), device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        assert objs[1].process_blocks_device(replayed, a1, b1, stream=s) == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(direct, replayed)
    assert (objs[0].wp, objs[0].wp2) == (objs[1].wp, objs[1].wp2)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("pts,nparts,ch,cap", [(64, 3, 2, 2), (1024, 94, 3, 5), (512, 16, 1, 7)])
def test_sub_batches_bit_exact(monkeypatch, pts, nparts, ch, cap, tv):
    """a small cap (CLFA_PCONV_BLOCKS_MAX, read at creation) makes one call cross many sub-batch boundaries; time-varying
    sub-batches are also capped at nparts"""
    rng = np.random.default_rng(cap * 31 + tv)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    N = 2 * nparts + 11
    a = _sig(rng, ch, N * pts)
    b = _sig(rng, ch, N * pts) if tv else None
    ref, st = _run_split(pts, nparts, ch, ir, a, b, [N])
    monkeypatch.setenv("CLFA_PCONV_BLOCKS_MAX", str(cap))
    got, st2 = _run_split(pts, nparts, ch, ir, a, b, [N])
    got2, st3 = _run_split(pts, nparts, ch, ir, a, b, [3, N - 3])
    assert st == st2 == st3
    assert _torch().equal(got, ref) and _torch().equal(got2, ref)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("pts", [64, 1024, 8])
def test_layouts_strides_offsets_and_host_form(pts, tv):
    torch = _torch()
    nparts, ch, nb = 5, 3, 13
    L = nb * pts
    rng = np.random.default_rng(pts + tv)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    a = _sig(rng, ch, L)
    b = _sig(rng, ch, L) if tv else None
    ref, st = _run_split(pts, nparts, ch, ir, a, b, [nb])
    # views into longer rows, one float off the 8-byte grid (in, in2 and out), odd row strides
    for off, extra in ((0, 6), (1, 7), (1, 0)):
        big_a = torch.zeros((ch, L + extra + off), device="cuda")
        big_a[:, off:off + L] = a
        va = big_a[:, off:off + L]
        vb = None
        if tv:
            big_b = torch.zeros((ch, L + extra + off), device="cuda")
            big_b[:, off:off + L] = b
            vb = big_b[:, off:off + L]
        big_o = torch.full((ch, L + extra + 3), 7.0, device="cuda")
        o_off = 1 if off else 2
        vo = big_o[:, o_off:o_off + L]
        p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
        assert p.push_ir(ir) == 0
        assert p.process_blocks_device(vo, va, vb) == 0
        torch.cuda.synchronize()
        assert torch.equal(vo, ref), "offset %d extra %d" % (off, extra)
        assert (p.wp, p.wp2) == st
        rest = big_o.clone()
        rest[:, o_off:o_off + L] = 7.0
        assert bool((rest == 7.0).all()), "wrote outside the rows"
    # host form
    p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.push_ir(ir) == 0
    out = np.zeros((ch, L), np.float32)
    assert p.convolution_blocks(out, a.cpu().numpy(), b.cpu().numpy() if tv else None) == 0
    assert np.array_equal(out, ref.cpu().numpy())
    assert (p.wp, p.wp2) == st
    # one channel, 1-D arrays
    p1 = fa.Clpconv(0, pts * nparts, pts)
    assert p1.push_ir(ir[0]) == 0
    o1 = np.zeros(L, np.float32)
    assert p1.convolution_blocks(o1, a[0].cpu().numpy(), b[0].cpu().numpy() if tv else None) == 0
    q1, _ = _run_split(pts, nparts, 1, ir[:1], a[:1].contiguous(), b[:1].contiguous() if tv else None, [nb])
    assert np.array_equal(o1, q1.cpu().numpy()[0])


def test_errors_leave_the_state_untouched():
    torch = _torch()
    pts, nparts, ch, nb = 64, 4, 2, 6
    rng = np.random.default_rng(5)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.push_ir(ir) == 0
    buf = _sig(rng, ch, 3 * nb * pts)
    a = buf[:, :nb * pts]
    keep = buf.clone()
    L = C.c_long
    h, f = p._h, lib().clfa_pconv_process_blocks_dev
    s = torch.cuda.current_stream().cuda_stream
    row = 3 * nb * pts
    base = buf.data_ptr()
    cases = [
        # out overlaps in1: whole, a one-float tail, a one-float head, the second row
        (base, row, base, None, row, nb),
        (base + 4 * (nb * pts - 1), row, base, None, row, nb),
        (base - 4 * (nb * pts - 1) + 4 * row, row, base + 4 * row, None, row, nb),
        (base + 4 * nb * pts, row, base, base + 4 * nb * pts, row, nb),   # in2 = out
        # short strides, negative counts
        (base + 4 * nb * pts, nb * pts - 1, base, None, row, nb),
        (base + 4 * nb * pts, row, base, None, nb * pts - 1, nb),
        (base + 4 * nb * pts, row, base, None, row, -1),
        # misaligned address, NULL
        (base + 4 * nb * pts + 2, row, base, None, row, nb),
        (None, row, base, None, row, nb),
    ]
    for o, os_, i1, i2, is_, n in cases:
        assert f(h, o, L(os_), i1, i2, L(is_), L(n), s) == CL_INVALID_VALUE, (o, os_, i1, i2, is_, n)
    torch.cuda.synchronize()
    assert torch.equal(buf, keep)
    assert (p.wp, p.wp2) == (0, nparts - 1)
    assert f(h, base, L(row), base, None, L(row), L(0), s) == 0      # nblocks == 0: nothing happens
    assert p.blocks_workspace_bytes() == 0
    # a failed object returns its error
    bad = fa.Clpconv(0, 100, 3)
    assert bad.get_cl_err() != 0
    assert lib().clfa_pconv_process_blocks_dev(bad._h, base, L(row), base, None, L(row), L(1), s) == bad.get_cl_err()
    # allocation under capture: CL_INVALID_OPERATION, nothing moves; the same call after a warm-up captures
    out = torch.full((ch, nb * pts), 3.0, device="cuda")
    dummy = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = p.process_blocks_device(out, a, None, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)   # (the graph is not empty)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and (p.wp, p.wp2) == (0, nparts - 1) and p.blocks_workspace_bytes() == 0


def _accuracy(ch, route_env, monkeypatch, seed):
    torch = _torch()
    pts, nparts, nb = 1024, 94, 110
    rng = np.random.default_rng(seed)
    ir = (rng.random((ch, pts * nparts), dtype=np.float32) - 0.5)
    p = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    for k, v in route_env.items():
        monkeypatch.setenv(k, v)
    q = fa.Clpconv(0, pts * nparts, pts, channels=ch)
    assert p.push_ir(ir) == 0 and q.push_ir(ir) == 0
    a = _sig(rng, ch, nb * pts)
    got, want = torch.empty_like(a), torch.empty_like(a)
    assert p.process_blocks_device(got, a, None) == 0
    _loop(q, want, a, None, nb, pts)
    torch.cuda.synchronize()
    an, g, w = a.cpu().numpy(), got.cpu().numpy(), want.cpu().numpy()
    eb, el = [], []
    for c in range(ch):
        truth = util.pconv_f64(ir[c].astype(np.float64), an[c].astype(np.float64), pts)
        eb.append(util.rel_err(g[c], truth))
        el.append(util.rel_err(w[c], truth))
    return q.kernel_name(), np.array(eb), np.array(el), np.array_equal(g, w)


def test_blocks_accuracy_config4_shape(monkeypatch):
    """config 4's geometry (pts 1024, 94 partitions, 110 blocks) with 160 of its 256 channels — still the single-block route
    k_pconv_fused, whose partition sums have the contract's order (one accumulator, ascending p): against float64 the
    multi-block route is no worse than 1.2 x that route: mean relL2 over the channels and worst sample of all of them
    (tests/test_gpu_conv_accuracy.py)"""
    name, eb, el, _ = _accuracy(160, {}, monkeypatch, 11)
    assert name == "k_pconv_fused"
    print("vs k_pconv_fused: blocks relL2 mean %.3g max %.3g; loop relL2 mean %.3g max %.3g; worst ratio relL2 %.3f max %.3f"
          % (eb[:, 0].mean(), eb[:, 1].max(), el[:, 0].mean(), el[:, 1].max(),
             float(np.max(eb[:, 0] / el[:, 0])), float(np.max(eb[:, 1] / el[:, 1]))))
    assert eb[:, 0].mean() <= 1.2 * el[:, 0].mean() and eb[:, 1].max() <= 1.2 * el[:, 1].max(), (eb, el)


def test_blocks_accuracy_against_the_cooperative_route(monkeypatch):
    """three channels: the single-block route is k_pconv_coop, which sums each bin's partitions in parallel rows and
    combines the rows, a shorter chain than one accumulator and so a little more accurate.  The multi-block route keeps
    the contract's order: its relL2 stays within 1.2 x (measured 1.14 x); its worst sample, one value of 110 K, within 1.5 x
    (measured 1.17-1.38 x)."""
    name, eb, el, _ = _accuracy(3, {}, monkeypatch, 11)
    assert name == "k_pconv_coop"
    for c in range(3):
        print("channel %d: blocks relL2 %.3g max %.3g, loop relL2 %.3g max %.3g" % (c, eb[c, 0], eb[c, 1], el[c, 0], el[c, 1]))
        assert eb[c, 0] <= 1.2 * el[c, 0] + 1e-9 and eb[c, 1] <= 1.5 * el[c, 1] + 1e-9, (eb[c], el[c])
