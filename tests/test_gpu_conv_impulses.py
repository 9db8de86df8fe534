"""Per-partition, per-bin GPU tests of every convolution route: block impulses against single-tap responses (exact float64,
tests/conv_exact.py), unit taps against noise for the direct convolution (==), a poisoned sample and its flush, and guard
bands around the single-block calls' buffers.

The noise tests (tests/test_gpu_conv.py, test_gpu_pconv_blocks.py, test_gpu_pconv_matrix.py, test_gpu_dconv_blocks.py)
accept relL2 <= 1e-6 over a channel: one entry of the per-bin tables (w2f, w2i, half) off by eps moves that norm by about
eps / sqrt(bins) (the entry serves every partition; measured with w2f[300] of pts 1024 scaled by 1 + 1e-4: they fail at relL2
5.7e-6, six times the bar, where the cases here fail by 100 times and name bin 300), one bin slice of one partition of the
multiply-accumulate by eps / sqrt(bins x partitions).  Here the rfft of a block pair is X H of
ONE partition with unit magnitude in every bin, so the same bar (TOL of SURVEY.md section 8d, which the reference's own
float32 arithmetic meets on these inputs: tests/test_conv_exact_cpu.py) holds per bin and per partition; every sample outside
the pairs must be exactly zero, so a partition that reaches a block it should not (ring index, segment boundary, stale
workspace) shows at any magnitude.  Each case prints `CONV-IMPULSE <route> ...`; the lines of one run are
profiles/conv_impulses.txt.
"""
import numpy as np
import pytest

import opencl_fft_amd as fa
from oracle import oracle
from tests import conv_exact as cx
from tests import gpu_guard
from tests.test_gpu_pconv_fade import SWEEP
from tests.util import TOL

pytestmark = pytest.mark.gpu

# Guard rows start off 16-byte alignment.  Cldconv's single-block kernel reads and writes single floats: 4 bytes off.
# Clpconv's single-block kernels move real samples in pairs, as 8-byte words (include/clfft_amd.h states 8 bytes for
# clfa_pconv_process_dev): 8 bytes off.
PCONV_MISALIGN, DCONV_MISALIGN = 2, 1


def _torch():
    import torch
    return torch


def _rows(nrows, rowlen, misalign):
    """nrows rows of rowlen floats inside a buffer of canaries: at least 4 canaries between rows, 64 at both ends; every
    row starts `misalign` floats past a 16-byte boundary"""
    g = gpu_guard.rows(nrows, rowlen, (rowlen + 4 + 3) // 4 * 4, misalign=misalign, before=64, after=64)
    assert all(r.data_ptr() % 16 == 4 * misalign for r in g.data[:2])
    return g


# ---- (a) per bin, per partition, every Clpconv route --------------------------------------------------------------------------------

def _assignments(pts, channels):
    """per run, per channel: a (parity, k, s) case or None (a channel with a response and no impulse: the last one of three
    channels and more)"""
    sl = cx.slots(pts, channels)
    usable = channels if channels < 3 else channels - 1
    for r in range(-(-len(sl) // usable)):
        yield [sl[(r * usable + j) % len(sl)] for j in range(usable)] + [None] * (channels - usable)


def _family(pts, nparts, b0, assign, tv):
    """(response or None, first input, second input or None), channels x samples, of one run"""
    nblocks = cx.nblocks_for(nparts, b0)
    ch = len(assign)
    x1 = np.zeros((ch, nblocks * pts), np.float32)
    h = np.zeros((ch, (nblocks if tv else nparts) * pts), np.float32)
    for c, slot in enumerate(assign):
        parity, k, s = slot if slot is not None else (c % 2, 1 % pts, None)
        if s is not None:
            x1[c] = cx.block_impulse(pts, nblocks, b0, s)
        h[c] = cx.tv_comb_input(pts, nparts, nblocks, parity, k) if tv else cx.comb_response(pts, nparts, parity, k)
    return (None, x1, h) if tv else (h, x1, None)


def _object(pts, nparts, channels, ir):
    p = fa.Clpconv(0, pts * nparts, pts, channels=channels)
    assert p.get_cl_err() == 0 and p.nparts == nparts
    if ir is not None:
        assert p.push_ir(ir) == 0
    return p


def _by_block(x, channels, pts):
    """(channels, nblocks * pts) -> (nblocks, channels * pts): the single-block calls' layout"""
    return np.ascontiguousarray(x.reshape(channels, -1, pts).transpose(1, 0, 2)).reshape(-1, channels * pts)


def _single_block_run(p, x1, x2):
    """every block through process_device, inputs and outputs as guarded rows -> (channels, nblocks * pts) on the host"""
    ch, pts = p.channels, p.pts
    nblocks = x1.shape[1] // pts
    a = _rows(nblocks, ch * pts, PCONV_MISALIGN).fill(_by_block(x1, ch, pts))
    b = _rows(nblocks, ch * pts, PCONV_MISALIGN).fill(_by_block(x2, ch, pts)) if x2 is not None else None
    o = _rows(nblocks, ch * pts, PCONV_MISALIGN)
    for j in range(nblocks):
        assert p.process_device(o.data[j], a.data[j], b.data[j] if b is not None else None) == 0
    _torch().cuda.synchronize()
    assert o.intact(), "wrote outside the output blocks"
    assert not o.unwritten(), "an output block was not written completely"
    assert a.unchanged() and (b is None or b.unchanged()), "an input buffer changed"
    return np.ascontiguousarray(o.host().reshape(nblocks, ch, pts).transpose(1, 0, 2)).reshape(ch, nblocks * pts)


def _blocks_run(p, x1, x2):
    """the whole signal through one process_blocks_device call"""
    torch = _torch()
    a = torch.from_numpy(x1).cuda()
    b = torch.from_numpy(x2).cuda() if x2 is not None else None
    out = torch.full_like(a, float("nan"))
    assert p.process_blocks_device(out, a, b) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(out, pts, nparts, b0, assign, what):
    """every channel of one run against its expectation -> (worst bin, worst sample) of the run"""
    wb = ws = 0.0
    bad = []
    for c, slot in enumerate(assign):
        if slot is None:
            n = int(np.count_nonzero(out[c]))
            if n:
                bad.append("channel %d got no impulse and has %d non-zero samples" % (c, n))
            continue
        parity, k, s = slot
        b, t, stray, at = cx.check_channel(out[c], pts, b0, cx.comb(nparts, parity), k, s)
        wb, ws = max(wb, b), max(ws, t)
        if stray:
            bad.append("channel %d (k %d s %d): %d non-zero samples outside the pairs" % (c, k, s, stray))
        if not (b <= TOL and t <= TOL):   # (a NaN fails too)
            bad.append("channel %d (k %d s %d): worst bin %.3g at partition %d bin %d, worst sample %.3g" % ((c, k, s, b) + at + (t,)))
    assert not bad, "%s: %s" % (what, "; ".join(bad[:8]))
    return wb, ws


def _impulse_case(name, pts, nparts, channels, b0, tv, make, run):
    wb = ws = 0.0
    for assign in _assignments(pts, channels):
        ir, x1, x2 = _family(pts, nparts, b0, assign, tv)
        p = make(ir)
        out = run(p, x1, x2)
        nblocks = x1.shape[1] // pts
        assert (p.wp, p.wp2) == (nblocks % nparts, (nparts - 1 - (nblocks if tv else 0)) % nparts)
        what = "%s %dx%dx%d %s" % (name, pts, nparts, channels, "tv" if tv else "static")
        b, t = _check(out, pts, nparts, b0, assign, what)
        wb, ws = max(wb, b), max(ws, t)
    print("CONV-IMPULSE %s %dx%dx%d %s b0=%d worst-bin %.3g worst-sample %.3g"
          % (name, pts, nparts, channels, "tv" if tv else "static", b0, wb, ws))


# Every route measured inside TOL on these families (profiles/conv_impulses.txt): no case carries a bound of its own.
@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("name,kernel,pts,nparts,channels,b0", cx.PCONV_ROUTES,
                         ids=["%s-%dx%dx%d" % (r[1], r[2], r[3], r[4]) for r in cx.PCONV_ROUTES])
def test_pconv_single_block_routes_per_bin(name, kernel, pts, nparts, channels, b0, tv):
    def make(ir):
        p = _object(pts, nparts, channels, ir)
        assert p.kernel_name() == kernel
        return p
    _impulse_case(name, pts, nparts, channels, b0, tv, make, _single_block_run)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
def test_pconv_unfused_160_channels_per_bin(monkeypatch, tv):
    """CLFA_PCONV_NO_FUSE: the route 160 channels take without k_pconv_fused"""
    monkeypatch.setenv("CLFA_PCONV_NO_FUSE", "1")
    names = set()

    def make(ir):
        p = _object(512, 5, 160, ir)
        names.add(p.kernel_name())
        return p
    _impulse_case("unfused", 512, 5, 160, 1, tv, make, _single_block_run)
    assert names and "k_pconv_fused" not in names and "" not in names, names


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
@pytest.mark.parametrize("kernel,pts,nparts,channels,b0", cx.PCONV_BLOCK_ROUTES)
def test_pconv_multi_block_route_per_bin(kernel, pts, nparts, channels, b0, tv):
    def make(ir):
        p = _object(pts, nparts, channels, ir)
        assert p.blocks_kernel_name() == kernel
        return p
    _impulse_case("multi-block " + kernel, pts, nparts, channels, b0, tv, make, _blocks_run)


@pytest.mark.parametrize("tv", [False, True], ids=["static", "tv"])
def test_pconv_multi_block_route_across_sub_batches_per_bin(monkeypatch, tv):
    """CLFA_PCONV_BLOCKS_MAX = 2 (read at creation): 9 blocks in five sub-batches, the pairs straddle their boundaries"""
    monkeypatch.setenv("CLFA_PCONV_BLOCKS_MAX", "2")

    def make(ir):
        p = _object(64, 3, 3, ir)
        assert p.blocks_kernel_name() == "k_pconvb_mac"
        return p
    _impulse_case("multi-block k_pconvb_mac, sub-batches of 2", 64, 3, 3, 4, tv, make, _blocks_run)


# ---- (b) the convolution matrix ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("segs,tile", SWEEP)
@pytest.mark.parametrize("inputs,outputs,pts,nparts", cx.MATRIX_GEOMS)
def test_matrix_entry_per_bin(monkeypatch, inputs, outputs, pts, nparts, segs, tile):
    """one input with an impulse, one (input, output) pair with a comb response: that output passes the per-bin check,
    every other output is exactly zero; with the impulse on the next input every output is"""
    torch = _torch()
    monkeypatch.setenv("CLFA_PCONV_MATRIX_SEGS", segs)
    monkeypatch.setenv("CLFA_PCONV_MATRIX_TILE", tile)
    i0, o0, b0 = 1, outputs - 2, nparts + 1
    nblocks = cx.nblocks_for(nparts, b0)
    wb = ws = 0.0
    for parity, k, s in cx.slots(pts, 1):
        parts = cx.comb(nparts, parity)
        x = np.zeros((inputs, nblocks * pts), np.float32)
        x[i0] = cx.block_impulse(pts, nblocks, b0, s)
        for swapped in (False, True):
            m = fa.PconvMatrix(0, pts * nparts, pts, inputs, outputs)
            assert m.get_error() == 0, m.get_log()
            assert m.kernel_name() == "k_pconvm_mac"
            assert m.push_ir(cx.matrix_entry(inputs, outputs, pts, nparts, i0, o0, parts, k)) == 0
            out = torch.full((outputs, nblocks * pts), float("nan"), device="cuda")
            assert m.process_device(out, torch.from_numpy(np.roll(x, 1, axis=0) if swapped else x).cuda()) == 0
            torch.cuda.synchronize()
            y = out.cpu().numpy()
            if swapped:
                assert not y.any(), "impulse on input %d, response on input %d: %d non-zero samples" % (i0 + 1, i0, np.count_nonzero(y))
                continue
            assert not np.delete(y, o0, axis=0).any(), "outputs without a response are not zero"
            b, t = _check(y[o0:o0 + 1], pts, nparts, b0, [(parity, k, s)], "matrix %dx%dx%dx%d" % (inputs, outputs, pts, nparts))
            wb, ws = max(wb, b), max(ws, t)
    print("CONV-IMPULSE matrix %dx%dx%dx%d segs=%s tile=%s b0=%d worst-bin %.3g worst-sample %.3g"
          % (inputs, outputs, pts, nparts, segs, tile, b0, wb, ws))


# ---- (c) direct convolution: a unit tap delays by exactly k + 1 ------------------------------------------------------------------------

def _dconv(irsize, vsize, channels, ir):
    d = fa.Cldconv(0, irsize, vsize, channels=channels)
    assert d.get_cl_err() == 0 and d.push_ir(ir) == 0
    return d


def _same_values(got, want, what):
    """== on values (the sign of a zero may differ)"""
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        raise AssertionError("%s: %d samples differ, the first at %s: got %r, expected %r"
                             % (what, at.shape[0], tuple(at[0]), got[tuple(at[0])], want[tuple(at[0])]))


@pytest.mark.parametrize("irsize,vsize", [(16, 8), (1000, 64)])
def test_dconv_single_block_kernel_exact_delay(irsize, vsize):
    """k_dconv_block: one-channel objects, block by block through process_device on guarded rows 4 bytes off alignment"""
    nblocks = cx.dconv_blocks_needed(irsize, vsize)
    x = cx.nonzero_noise([irsize, vsize], nblocks * vsize)
    a = _rows(nblocks, vsize, DCONV_MISALIGN).fill(x.reshape(nblocks, vsize))
    for k in cx.dconv_taps(irsize):
        d = _dconv(irsize, vsize, 1, cx.unit_tap(irsize, k))
        o = _rows(nblocks, vsize, DCONV_MISALIGN)
        for j in range(nblocks):
            assert d.process_device(o.data[j], a.data[j]) == 0
        _torch().cuda.synchronize()
        assert o.intact() and not o.unwritten() and a.unchanged(), "tap %d: guard bands" % k
        _same_values(o.host().reshape(-1), cx.dconv_delayed(x, k), "irsize %d vsize %d tap %d" % (irsize, vsize, k))


def _dconv_blocks_exact(irsize, vsize, nblocks, splits):
    """three channels, a different tap each, until every tap of the family has run; the signal in calls of `splits` blocks"""
    torch = _torch()
    taps = cx.dconv_taps(irsize)
    x = cx.nonzero_noise([irsize, vsize, 3], (3, nblocks * vsize))
    xd = torch.from_numpy(x).cuda()
    for lo in range(0, len(taps), 3):
        ks = [taps[(lo + c) % len(taps)] for c in range(3)]
        d = _dconv(irsize, vsize, 3, np.stack([cx.unit_tap(irsize, k) for k in ks]))
        assert d.blocks_kernel_name() == "k_dconvb_fir"
        out = torch.full_like(xd, float("nan"))
        j = 0
        for n in splits:
            sl = slice(j * vsize, (j + n) * vsize)
            assert d.process_blocks_device(out[:, sl], xd[:, sl]) == 0
            j += n
        assert j == nblocks
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for c, k in enumerate(ks):
            _same_values(got[c], cx.dconv_delayed(x[c], k), "irsize %d vsize %d tap %d (channel %d)" % (irsize, vsize, k, c))
    return d


@pytest.mark.parametrize("r", ["8", "2"])
@pytest.mark.parametrize("irsize,vsize", [(65, 7), (1000, 64)])
def test_dconv_blocks_kernel_exact_delay(monkeypatch, irsize, vsize, r):
    monkeypatch.setenv("CLFA_DCONV_BLOCKS_R", r)
    nblocks = cx.dconv_blocks_needed(irsize, vsize)
    d = _dconv_blocks_exact(irsize, vsize, nblocks, [nblocks])
    assert d.blocks_workspace_bytes() == 0


@pytest.mark.parametrize("irsize,vsize", [(4097, 32), (96000, 64)])
def test_dconv_blocks_segmented_route_exact_delay(irsize, vsize):
    """responses of more than 4096 taps: tap segments and k_dconvb_reduce; a call of 12 blocks, then the rest of two turns
    of the delay ring"""
    nblocks = cx.dconv_blocks_needed(irsize, vsize)
    d = _dconv_blocks_exact(irsize, vsize, nblocks, [12, nblocks - 12])
    assert d.blocks_workspace_bytes() > 0


def test_dconv_blocks_across_sub_batches_exact_delay(monkeypatch):
    monkeypatch.setenv("CLFA_DCONV_BLOCKS_MAX", "2")
    nblocks = cx.dconv_blocks_needed(65, 7)
    _dconv_blocks_exact(65, 7, nblocks, [nblocks])


@pytest.mark.parametrize("irsize,vsize", [(16, 8), (65, 7)])
def test_dconv_time_varying_loop_route_exact(irsize, vsize):
    """unit samples in the second input, one in the coefficient ring at a time: the oracle's output value for value, which
    is the contract's (tests/test_conv_exact_cpu.py)"""
    torch = _torch()
    channels = 2
    nblocks = cx.dconv_blocks_needed(irsize, vsize, wraps=3)
    x1 = cx.nonzero_noise([irsize, vsize, 2], (channels, nblocks * vsize))
    x2 = np.stack([cx.dconv_tv_impulses(irsize, vsize, nblocks), np.roll(cx.dconv_tv_impulses(irsize, vsize, nblocks), 5)])
    d = fa.Cldconv(0, irsize, vsize, channels=channels)
    assert d.get_cl_err() == 0 and d.blocks_kernel_name(True) == "loop"
    out = torch.full((channels, nblocks * vsize), float("nan"), device="cuda")
    assert d.process_blocks_device(out, torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for c in range(channels):
        o = oracle.Dconv(irsize, vsize)
        want = np.concatenate([o.convolution(x1[c, j * vsize:(j + 1) * vsize], x2[c, j * vsize:(j + 1) * vsize])
                               for j in range(nblocks)])
        assert np.count_nonzero(want) > irsize
        _same_values(got[c], want, "irsize %d vsize %d channel %d" % (irsize, vsize, c))
    _same_values(got, cx.dconv_tv_expected(irsize, vsize, x1, x2), "against the contract")


# ---- (d) a NaN reaches no other channel and leaves the state when the formula says so ----------------------------------------------------

def _bits(t):
    return t.contiguous().view(_torch().int32)


NAN_ROUTES = [("k_pconv_coop", 1024, 94, 2, {}), ("k_pconv_coop", 512, 600, 1, {}), ("k_pconv_coop", 512, 6, 100, {}),
              ("k_pconv_fused", 512, 5, 162, {}), ("k_pconv_fused", 1024, 40, 160, {}), ("chain", 16384, 2, 2, {}),
              ("chain", 8, 4, 3, {}), ("blocks:k_pconvb_mac", 64, 3, 3, {}), ("blocks:k_pconvb_mac", 1024, 94, 3, {"CLFA_PCONV_BLOCKS_MAX": "5"})]


@pytest.mark.parametrize("kernel,pts,nparts,channels,env", NAN_ROUTES, ids=["%s-%dx%dx%d" % r[:4] for r in NAN_ROUTES])
def test_pconv_nan_stays_in_its_channel_and_is_flushed(monkeypatch, kernel, pts, nparts, channels, env):
    """noise twice, the second time with one NaN sample in block 2 of one channel: every other channel keeps its bits, and
    the poisoned one has them back from block 2 + nparts + 1 on — spectrum 2 has left the ring after nparts blocks and the
    overlap-add tail one block later; a route that keeps the NaN longer has stale state"""
    torch = _torch()
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    b, c = 2, channels // 2
    nblocks = b + nparts + 4
    g = torch.Generator(device="cuda").manual_seed(pts + nparts + channels)
    ir = ((torch.rand((channels, pts * nparts), generator=g, device="cuda") - 0.5) / (pts * nparts) ** 0.5)
    x = torch.rand((nblocks, channels, pts), generator=g, device="cuda") * 2 - 1
    outs = []
    for poisoned in (False, True):
        xin = x.clone()
        if poisoned:
            xin[b, c, pts // 3] = float("nan")
        p = fa.Clpconv(0, pts * nparts, pts, channels=channels)
        assert p.get_cl_err() == 0 and p.push_ir_device(ir) == 0
        y = torch.empty_like(xin)
        if kernel.startswith("blocks:"):
            assert p.blocks_kernel_name() == kernel[7:]
            rows, yrows = xin.transpose(0, 1).reshape(channels, nblocks * pts).contiguous(), torch.empty((channels, nblocks * pts), device="cuda")
            assert p.process_blocks_device(yrows, rows) == 0
            y = yrows.view(channels, nblocks, pts).transpose(0, 1)
        else:
            assert p.kernel_name() == kernel
            for j in range(nblocks):
                assert p.process_device(y[j], xin[j]) == 0
        torch.cuda.synchronize()
        outs.append(y)
    clean, dirty = outs
    assert not bool(torch.isnan(clean).any())
    assert bool(torch.isnan(dirty[b, c]).any()), "the poisoned block came out without a NaN"
    others = [i for i in range(channels) if i != c]
    assert torch.equal(_bits(clean[:, others]), _bits(dirty[:, others])), "the NaN reached another channel"
    assert torch.equal(_bits(clean[:b, c]), _bits(dirty[:b, c])), "blocks before the NaN changed"
    late = dirty[b + nparts + 1:, c]
    assert torch.equal(_bits(clean[b + nparts + 1:, c]), _bits(late)), \
        "the poisoned channel differs after the flush: first block %d" % (b + nparts + 1 + int((_bits(clean[b + nparts + 1:, c]) != _bits(late)).any(dim=1).nonzero()[0]))


def test_matrix_nan_is_flushed(monkeypatch):
    """the matrix mixes every input into every output: all outputs have their bits back from block 2 + nparts + 1 on"""
    torch = _torch()
    inputs, outputs, pts, nparts = cx.MATRIX_GEOMS[0]
    monkeypatch.setenv("CLFA_PCONV_MATRIX_SEGS", "3")
    monkeypatch.setenv("CLFA_PCONV_MATRIX_BLOCKS_MAX", "5")
    b = 2
    nblocks = b + nparts + 4
    rng = np.random.default_rng(12)
    ir = rng.random((outputs, inputs, pts * nparts), dtype=np.float32) - 0.5
    x = torch.from_numpy(rng.random((inputs, nblocks * pts), dtype=np.float32) - 0.5).cuda()
    outs = []
    for poisoned in (False, True):
        xin = x.clone()
        if poisoned:
            xin[1, b * pts + pts // 3] = float("nan")
        m = fa.PconvMatrix(0, pts * nparts, pts, inputs, outputs)
        assert m.get_error() == 0 and m.push_ir(ir) == 0
        out = torch.empty((outputs, nblocks * pts), device="cuda")
        assert m.process_device(out, xin) == 0
        torch.cuda.synchronize()
        outs.append(out)
    clean, dirty = outs
    assert not bool(torch.isnan(clean).any()) and bool(torch.isnan(dirty[:, b * pts:(b + 1) * pts]).any())
    assert torch.equal(_bits(clean[:, :b * pts]), _bits(dirty[:, :b * pts]))
    n0 = (b + nparts + 1) * pts
    assert torch.equal(_bits(clean[:, n0:]), _bits(dirty[:, n0:])), "the NaN is still in the state after nparts + 1 blocks"


@pytest.mark.parametrize("irsize,vsize,cap", [(65, 7, None), (4097, 32, "3")])
def test_dconv_blocks_nan_stays_in_its_channel_and_is_flushed(monkeypatch, irsize, vsize, cap):
    """k_dconvb_fir (and the segmented route under a sub-batch cap): a NaN at sample n of one channel is in outputs
    n + 1 .. n + irsize of that channel and nowhere else"""
    torch = _torch()
    if cap:
        monkeypatch.setenv("CLFA_DCONV_BLOCKS_MAX", cap)
    channels, n = 3, 2 * vsize + 3
    nblocks = (n + irsize) // vsize + 4
    rng = np.random.default_rng(irsize)
    ir = rng.random((channels, irsize), dtype=np.float32) - 0.5
    x = torch.from_numpy(rng.random((channels, nblocks * vsize), dtype=np.float32) - 0.5).cuda()
    outs = []
    for poisoned in (False, True):
        xin = x.clone()
        if poisoned:
            xin[1, n] = float("nan")
        d = _dconv(irsize, vsize, channels, ir)
        out = torch.empty_like(xin)
        half = (nblocks // 2) * vsize
        assert d.process_blocks_device(out[:, :half], xin[:, :half]) == 0
        assert d.process_blocks_device(out[:, half:], xin[:, half:]) == 0
        torch.cuda.synchronize()
        outs.append(out)
    clean, dirty = outs
    assert not bool(torch.isnan(clean).any()) and bool(torch.isnan(dirty[1, n + 1:n + 1 + irsize]).all())
    assert torch.equal(_bits(clean[[0, 2]]), _bits(dirty[[0, 2]])), "the NaN reached another channel"
    assert torch.equal(_bits(clean[1, :n + 1]), _bits(dirty[1, :n + 1]))
    assert torch.equal(_bits(clean[1, n + 1 + irsize:]), _bits(dirty[1, n + 1 + irsize:])), "the NaN outlived irsize samples"
