"""Multi-block, multi-channel direct convolution (clfa_dconv_process_blocks_dev) on the GPU: every case against
oracle.Dconv per channel, block by block; bit-identity across splits, sub-batches, streams, graph replay and the
single-block calls; the state a call leaves; the two-input "loop" route; errors; accuracy against float64.

The kernel's own constants (opencl_fft_amd/csrc/dconv_launch.hpp, dconv_blocks.hip): the tap chunk kDconvbChunk = 256 (taps
per staged window and per partial accumulator), R = 2 or 8 outputs per lane (CLFA_DCONV_BLOCKS_R forces one; the launcher
picks by the size of the launch), the tile 256 R = 512 or 2048 outputs per workgroup, and the segment length kDconvbSeg =
4096 taps (longer responses: partial sums per segment, k_dconvb_reduce)."""
import ctypes as C

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd._lib import lib
from oracle import oracle
from tests import util
from tests.dconv_blocks_model import DconvBlocksModel

pytestmark = pytest.mark.gpu

CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59


def dconv_tol(irsize):
    """tests/test_gpu_conv.py dconv_tol: two float32 sums of irsize products in different orders"""
    return max(1e-6, 2 * float(np.sqrt(irsize)) * 2.0 ** -24)


def _torch():
    import torch
    return torch


def _rows(data, extra=5, with_buffer=False):
    """device rows holding `data` (channels, L): row stride L + extra, base address 4 bytes off 16-byte alignment"""
    torch = _torch()
    ch, L = data.shape
    stride = L + extra
    buf = torch.full((ch * stride + 8,), 7.0, device="cuda")
    off = (1 - buf.data_ptr() // 4) % 4   # float offset that puts the view at 16 k + 4 bytes
    view = buf[off:off + ch * stride].view(ch, stride)[:, :L]
    assert view.data_ptr() % 16 == 4
    view.copy_(torch.from_numpy(np.array(data)))   # (a copy: the shared cases are read-only)
    if not with_buffer:
        return view
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[off:off + ch * stride].view(ch, stride)[:, :L] = False
    return view, lambda: bool((buf[outside] == 7.0).all())


_ORACLE = {}


def _case(irsize, vsize, nblocks, channels, seed=0):
    """seeded response and input of a geometry and the oracle's outputs, block by block per channel (computed once)"""
    key = (irsize, vsize, nblocks, channels, seed)
    if key not in _ORACLE:
        rng = np.random.default_rng([irsize, vsize, nblocks, channels, seed])
        ir = rng.random((channels, irsize), dtype=np.float32) - 0.5
        x = rng.random((channels, nblocks * vsize), dtype=np.float32) - 0.5
        want = np.empty_like(x)
        for c in range(channels):
            o = oracle.Dconv(irsize, vsize)
            o.push_ir(ir[c])
            for j in range(nblocks):
                want[c, j * vsize:(j + 1) * vsize] = o.convolution(x[c, j * vsize:(j + 1) * vsize])
        for a in (ir, x, want):
            a.setflags(write=False)
        _ORACLE[key] = (ir, x, want)
    return _ORACLE[key]


def _obj(irsize, vsize, channels, ir):
    d = fa.Cldconv(0, irsize, vsize, channels=channels)
    assert d.get_cl_err() == 0
    assert d.push_ir(ir if channels > 1 else ir[0]) == 0
    return d


def _run(irsize, vsize, channels, ir, x, splits, stream=None):
    """a fresh object, the signal in calls of `splits` blocks on strided, misaligned rows -> (outputs, wp)"""
    torch = _torch()
    d = _obj(irsize, vsize, channels, ir)
    xin = _rows(x)
    out, untouched = _rows(np.zeros_like(x), with_buffer=True)
    torch.cuda.synchronize()
    j = 0
    for n in splits:
        sl = slice(j * vsize, (j + n) * vsize)
        assert d.process_blocks_device(out[:, sl], xin[:, sl], None, stream=stream) == 0
        j += n
    torch.cuda.synchronize()
    assert j * vsize == x.shape[1]
    assert untouched(), "wrote outside the rows"
    return out.clone(), d.wp


def _check(got, want, irsize, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    err = float(np.max(np.abs(g - want))) / max(float(np.max(np.abs(want))), 1e-30)
    print("%s: max error / largest expected sample %.3g (bound %.3g)" % (what, err, dconv_tol(irsize)))
    assert err <= dconv_tol(irsize), (what, err)


# the issue's table, then irsize one below, at and one above: R = 2, R = 8, the tap chunk 256, the tiles 512 and 2048,
# the segment length 4096 (4097: in the table)
TABLE = [(1, 1, 5, 3), (7, 3, 9, 3), (5, 8, 6, 3), (65, 7, 30, 3), (1000, 64, 40, 3), (4097, 64, 3, 3), (9000, 500, 2, 3),
         (96000, 64, 4, 1)]
BOUNDS = [(n, 16, 40, 3) for n in (2, 3, 8, 9, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096)]


@pytest.mark.parametrize("irsize,vsize,nblocks,channels", TABLE + BOUNDS)
def test_blocks_vs_oracle(monkeypatch, irsize, vsize, nblocks, channels):
    """one call on 3 channels (strides longer than the rows, base 4 bytes off 16-byte alignment) against the oracle; run
    with R = 2 and with R = 8: the same bits"""
    ir, x, want = _case(irsize, vsize, nblocks, channels)
    outs = []
    for r in ("2", "8"):
        monkeypatch.setenv("CLFA_DCONV_BLOCKS_R", r)
        got, wp = _run(irsize, vsize, channels, ir, x, [nblocks])
        assert wp == (nblocks * vsize) % (irsize + vsize)
        _check(got, want, irsize, "irsize %d vsize %d x %d blocks, R = %s" % (irsize, vsize, nblocks, r))
        outs.append(got)
    assert _torch().equal(outs[0], outs[1]), "R = 2 and R = 8 differ"


def test_large_launch_picks_the_wide_tile_with_the_same_bits(monkeypatch):
    """400000 outputs per channel: the launcher's own choice (R = 8 from two workgroups per CU on) against forced R = 2,
    and against the oracle"""
    irsize, vsize, nblocks, channels = 9, 500, 800, 3
    ir, x, want = _case(irsize, vsize, nblocks, channels)
    got, _ = _run(irsize, vsize, channels, ir, x, [nblocks])
    _check(got, want, irsize, "400000 outputs x 3 channels")
    monkeypatch.setenv("CLFA_DCONV_BLOCKS_R", "2")
    narrow, _ = _run(irsize, vsize, channels, ir, x, [nblocks])
    assert _torch().equal(got, narrow)


@pytest.mark.parametrize("irsize,vsize,nblocks,channels", [(65, 7, 30, 3), (1000, 64, 40, 3), (96000, 64, 12, 1)])
def test_bit_identity_across_splits_caps_streams_and_replay(monkeypatch, irsize, vsize, nblocks, channels):
    torch = _torch()
    ir, x, want = _case(irsize, vsize, nblocks, channels)
    ref, wp = _run(irsize, vsize, channels, ir, x, [nblocks])
    _check(ref, want, irsize, "one call")
    assert wp == (nblocks * vsize) % (irsize + vsize)
    got, wp2 = _run(irsize, vsize, channels, ir, x, [1, 5, 0, nblocks - 6])
    assert wp2 == wp and torch.equal(got, ref), "split 1 + 5 + 0 + rest"
    side = torch.cuda.Stream()
    got, _ = _run(irsize, vsize, channels, ir, x, [nblocks // 2, nblocks - nblocks // 2], stream=side.cuda_stream)
    assert torch.equal(got, ref), "another stream"
    # a replay of a captured graph: the first half eagerly (it warms the segmented route's workspace), the second half
    # captured and replayed
    xc = torch.from_numpy(np.array(x)).cuda()
    replayed = torch.empty_like(xc)
    half = (nblocks // 2) * vsize
    d = _obj(irsize, vsize, channels, ir)
    assert d.process_blocks_device(replayed[:, :half], xc[:, :half], None) == 0   # eager: warms any workspace
    torch.cuda.synchronize()
    tail_in, tail_out = xc[:, half:].contiguous(), torch.empty_like(xc[:, half:].contiguous())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert d.process_blocks_device(tail_out, tail_in, None, stream=torch.cuda.current_stream().cuda_stream) == 0
    g.replay()
    torch.cuda.synchronize()
    assert d.wp == wp
    assert torch.equal(replayed[:, :half], ref[:, :half]) and torch.equal(tail_out, ref[:, half:]), "graph replay"
    # the sub-batch cap forced to 2 blocks (read per object)
    monkeypatch.setenv("CLFA_DCONV_BLOCKS_MAX", "2")
    got, wp3 = _run(irsize, vsize, channels, ir, x, [nblocks])
    assert wp3 == wp and torch.equal(got, ref), "sub-batches of 2 blocks"
    monkeypatch.delenv("CLFA_DCONV_BLOCKS_MAX")
    if channels > 1:   # process_device on a multi-channel object is the block call with nblocks = 1
        d = _obj(irsize, vsize, channels, ir)
        out = torch.empty_like(xc)
        for j in range(nblocks):
            o = torch.empty((channels, vsize), device="cuda")
            assert d.process_device(o, xc[:, j * vsize:(j + 1) * vsize].contiguous()) == 0
            out[:, j * vsize:(j + 1) * vsize] = o
        torch.cuda.synchronize()
        assert d.wp == wp and torch.equal(out, ref), "single-block calls"


@pytest.mark.parametrize("irsize,vsize,nblocks", [(65, 7, 30), (1000, 64, 5), (5, 8, 6)])
def test_state_after_a_block_call_equals_single_block_calls(irsize, vsize, nblocks):
    """one-channel objects on both sides: after the block call wp is the model's, and the next three single-block outputs
    (k_dconv_block on rings that are copies of the inputs) are bit for bit those of an object fed block by block"""
    torch = _torch()
    ir, x, _ = _case(irsize, vsize, nblocks + 3, 1)
    a, b = _obj(irsize, vsize, 1, ir), _obj(irsize, vsize, 1, ir)
    xd = torch.from_numpy(np.array(x[0])).cuda()
    L = nblocks * vsize
    out = torch.empty(L, device="cuda")
    assert a.process_blocks_device(out, xd[:L]) == 0
    for j in range(nblocks):
        o = torch.empty(vsize, device="cuda")
        assert b.process_device(o, xd[j * vsize:(j + 1) * vsize].contiguous()) == 0
    m = DconvBlocksModel(irsize, vsize)
    m.push_ir(ir)
    m.blocks(x[:, :L])
    assert a.wp == m.wp == b.wp
    for j in range(nblocks, nblocks + 3):
        blk = xd[j * vsize:(j + 1) * vsize].contiguous()
        oa, ob = torch.empty(vsize, device="cuda"), torch.empty(vsize, device="cuda")
        assert a.process_device(oa, blk) == 0 and b.process_device(ob, blk) == 0
        torch.cuda.synchronize()
        assert torch.equal(oa, ob), "single block %d after the block call" % j
    assert a.wp == b.wp


@pytest.mark.parametrize("irsize,vsize", [(16, 8), (256, 32), (65, 7), (7, 3)])
def test_time_varying_loop_route_vs_oracle(irsize, vsize):
    """two channels, the oracle's two-input call block by block; a static block call and a push_ir_device in between
    ((7, 3): end = 10, so the second channel's rings start off 16-byte alignment)"""
    torch = _torch()
    channels = 2
    rng = np.random.default_rng(irsize + vsize)
    d = fa.Cldconv(0, irsize, vsize, channels=channels)
    assert d.get_cl_err() == 0 and d.blocks_kernel_name(True) == "loop" and d.blocks_kernel_name() == "k_dconvb_fir"
    orcs = [oracle.Dconv(irsize, vsize) for _ in range(channels)]
    cycle = (irsize + vsize) // vsize + 1
    wp = 0
    for step, (nb, tv) in enumerate([(3, True), (cycle + 2, True), (4, False), (2, True), (cycle, False), (5, True)]):
        if step == 3:
            ir = rng.random((channels, irsize + 3), dtype=np.float32) - 0.5
            ird = _rows(ir)
            assert d.push_ir_device(ird) == 0
            for c in range(channels):
                orcs[c].push_ir(ir[c, :irsize])
        x1 = rng.random((channels, nb * vsize), dtype=np.float32) - 0.5
        x2 = rng.random((channels, nb * vsize), dtype=np.float32) - 0.5 if tv else None
        a = _rows(x1)
        b = _rows(x2) if tv else None
        out = _rows(np.zeros_like(x1))
        assert d.process_blocks_device(out, a, b) == 0
        torch.cuda.synchronize()
        wp = (wp + nb * vsize) % (irsize + vsize)
        assert d.wp == wp
        for c in range(channels):
            want = np.concatenate([orcs[c].convolution(x1[c, j * vsize:(j + 1) * vsize],
                                                       None if x2 is None else x2[c, j * vsize:(j + 1) * vsize])
                                   for j in range(nb)])
            _check(out[c], want, irsize, "step %d channel %d (%s)" % (step, c, "tv" if tv else "static"))


def test_errors_leave_the_state_untouched():
    torch = _torch()
    irsize, vsize, channels, nb = 40, 8, 2, 6
    ir, x, _ = _case(irsize, vsize, nb, channels)
    d = _obj(irsize, vsize, channels, ir)
    warm = torch.zeros((channels, vsize), device="cuda")
    assert d.process_blocks_device(torch.empty_like(warm), warm) == 0   # wp = 8
    L = nb * vsize
    row = 3 * L
    buf = torch.zeros((channels, row), device="cuda")
    buf[:, :L] = torch.from_numpy(np.array(x)).cuda()
    keep = buf.clone()
    torch.cuda.synchronize()
    cl, f, h = C.c_long, lib().clfa_dconv_process_blocks_dev, d._h
    s = torch.cuda.current_stream().cuda_stream
    base = buf.data_ptr()
    cases = [
        (base + 4 * (L - 1), row, base, None, row, nb),        # out overlaps in1 by one sample
        (base, row, base, None, row, nb),                      # in place
        (base + 4 * L, row, base, base + 4 * L, row, nb),      # in2 = out
        (base + 4 * L, L - 1, base, None, row, nb),            # strides below nblocks * vsize
        (base + 4 * L, row, base, None, L - 1, nb),
        (None, row, base, None, row, nb),                      # NULL pointers
        (base + 4 * L, row, None, None, row, nb),
        (base + 4 * L + 2, row, base, None, row, nb),          # misaligned
        (base + 4 * L, row, base, None, row, -1),
    ]
    for o, os_, i1, i2, is_, n in cases:
        assert f(h, o, cl(os_), i1, i2, cl(is_), cl(n), s) == CL_INVALID_VALUE, (o, os_, i1, i2, is_, n)
        assert d.wp == vsize
    assert lib().clfa_dconv_push_ir_dev(h, None, cl(irsize), s) == CL_INVALID_VALUE
    assert lib().clfa_dconv_push_ir_dev(h, base, cl(irsize - 1), s) == CL_INVALID_VALUE
    assert f(h, base, cl(row), base, None, cl(row), cl(0), s) == 0   # nblocks == 0: nothing happens
    torch.cuda.synchronize()
    assert torch.equal(buf, keep) and d.wp == vsize
    assert d.process_device(buf[:, :vsize].contiguous(), buf[0, :vsize].contiguous()) == CL_INVALID_VALUE   # one channel's block
    # the segmented route under capture before its workspace exists: CL_INVALID_OPERATION, nothing moves
    big = fa.Cldconv(0, 5000, 8, channels=2)
    assert big.get_cl_err() == 0 and big.blocks_workspace_bytes() == 0
    a = torch.zeros((2, 16), device="cuda")
    out = torch.full((2, 16), 3.0, device="cuda")
    dummy = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = big.process_blocks_device(out, a, None, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)   # (the graph is not empty)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and big.wp == 0 and big.blocks_workspace_bytes() == 0
    assert big.process_blocks_device(out, a, None) == 0 and big.blocks_workspace_bytes() > 0


def test_host_forms_and_one_dimensional_rows():
    ir, x, want = _case(1000, 64, 40, 3)
    d = _obj(1000, 64, 3, ir)
    out = np.zeros_like(x)
    assert d.convolution_blocks(out, x) == 0
    ref, wp = _run(1000, 64, 3, ir, x, [40])
    assert np.array_equal(out, ref.cpu().numpy()) and d.wp == wp
    blk = np.zeros((3, 64), np.float32)
    d2 = _obj(1000, 64, 3, ir)
    for j in range(3):
        assert d2.convolution(blk, np.ascontiguousarray(x[:, j * 64:(j + 1) * 64])) == 0
        assert np.array_equal(blk, out[:, j * 64:(j + 1) * 64])
    ir1, x1, want1 = _case(65, 7, 30, 1)
    d1 = _obj(65, 7, 1, ir1)
    o1 = np.zeros(x1.shape[1], np.float32)
    assert d1.convolution_blocks(o1, x1[0]) == 0
    _check(o1, want1[0], 65, "one channel, 1-D host rows")
    assert d1.state_bytes() == 2 * 4 * (65 + 7)


@pytest.mark.parametrize("irsize,vsize", [(1024, 64), (96000, 500)])
def test_blocks_at_least_as_accurate_as_the_oracles_serial_sum(irsize, vsize):
    """the outputs of the last block once the delay line is full, against float64 and against the oracle's arithmetic
    (float32 products added one by one in tap order, tests/util.py dconv_last_block): HIP relL2 and max error <= 1.2 x the
    oracle's + 1e-9 (tests/test_gpu_conv_accuracy.py)"""
    torch = _torch()
    blocks = irsize // vsize + 3
    rng = np.random.default_rng(irsize)
    ir = ((rng.random(irsize, dtype=np.float32) - 0.5) / np.float32(np.sqrt(irsize))).astype(np.float32)
    x = (rng.random(blocks * vsize, dtype=np.float32) * 2 - 1).astype(np.float32)
    d = fa.Cldconv(0, irsize, vsize)
    assert d.get_cl_err() == 0 and d.push_ir(ir) == 0
    out = torch.empty(blocks * vsize, device="cuda")
    assert d.process_blocks_device(out, torch.from_numpy(x).cuda()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()[(blocks - 1) * vsize:]
    pick = np.arange(vsize)
    truth, seq = util.dconv_last_block(ir, x, vsize, blocks - 1, pick)
    eh, eo, df = util.rel_err(got, truth), util.rel_err(seq, truth), util.rel_err(got, seq)
    print("ACCURACY %-44s HIP vs f64 relL2 %.3g max %.3g | oracle vs f64 relL2 %.3g max %.3g | HIP vs oracle relL2 %.3g max %.3g"
          % ("dconv blocks irsize %d" % irsize, eh[0], eh[1], eo[0], eo[1], df[0], df[1]))
    assert eh[0] <= 1.2 * eo[0] + 1e-9 and eh[1] <= 1.2 * eo[1] + 1e-9, (eh, eo)
    assert df[0] <= dconv_tol(irsize) and df[1] <= dconv_tol(irsize), df
