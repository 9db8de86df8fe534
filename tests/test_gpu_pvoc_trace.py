"""The N loudest bins of clfa_pvoc on the device (pvoc_trace.hip: k_pvoc_trace) against the numpy restatement of their
definition (tests/pvoc_trace_model.py).

Everything is compared bit for bit: the definition has no arithmetic in it, so there is no tolerance to choose.  Where
the model gives a NaN the device gives a NaN.  The inputs are tests/pvoc_inputs.py's frames and the model file's two
recipes (tests/test_pvoc_trace_cpu.py shows that the levels cases notice eight mutants of the model at every size run
here).  Both outputs lie in the guard bands of tests/gpu_guard.py: the frames 8-byte and not 16-byte aligned, the bin list
4-byte and not 8-byte aligned."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard
from tests import pvoc_trace_model as tm
from tests.gpu_guard import CANARY, DEV, bits, dev, same
from tests.pvoc_inputs import SR, analysed, make_pvoc, raw, raw_freq_first
from tests.test_pvoc_trace_cpu import gpu_cases

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
f32 = np.float32
SIZES = (64, 128, 512, 2048, 16384)


def make(size, channels=1, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert pv.trace_kernel_name() == "k_pvoc_trace"
    return pv


def run_guarded(pv, x, n, first=0, nbins=None, residual=False, list_n=0, stream=None):
    """one device call into guarded outputs: (frames, bins or None) as numpy, the guard bands checked, every element
    written; n: a number, or an array that goes to the device"""
    dx = dev(x)
    dn = n if np.isscalar(n) else dev(np.asarray(n, f32))
    out = gpu_guard.flat(x.shape, misalign=2)
    lst = gpu_guard.flat(x.shape[:2] + (list_n,), misalign=1) if list_n else None
    b = lst.data.view(torch.int32) if list_n else None
    assert out.data.data_ptr() % 16 == 8 and (b is None or b.data_ptr() % 8 == 4)
    if stream is not None:
        torch.cuda.synchronize()          # the arrays above were filled on the current stream
    assert pv.trace_device(dx, out.data, dn, first, nbins, residual, bins_out=b, stream=stream) == 0
    torch.cuda.synchronize()
    for g, what in ((out, "the frames"), (lst, "the bin list")):
        if g is not None:
            g.check_sides(what)
            assert not g.unwritten(), "an element of %s was not written" % what
    return out.data.cpu().numpy(), None if b is None else b.cpu().numpy()


def check(pv, x, n, first, nbins, residual, list_n, what, stream=None):
    got, lst = run_guarded(pv, x, n, first, nbins, residual, list_n, stream)
    row = np.full(x.shape[1], n, f32) if np.isscalar(n) else n
    want, wlst = tm.trace(x, row, first, nbins, residual, list_n)
    what = "%s range %d %s residual %d list %d" % (what, first, nbins, residual, list_n)
    same(got, want, what)
    assert np.array_equal(bits(got[..., 1]), bits(x[..., 1])), what + ": the freq column is the input's bits"
    if list_n:
        assert np.array_equal(lst, wlst), what + ": the bin list"


def list_lengths(nbins):
    """no list, one entry, a truncating list, a list padded with -1"""
    return (0, 1, 7, nbins + 3)


def inputs(size, C, F):
    """(name, frames): analysed frames, raw frames, raw frames with NaN amps and freqs, and the two near-key recipes"""
    return (("analysed", analysed(size, C, F, 3)), ("raw", raw(size, C, F, 4)), ("raw with NaNs", raw_freq_first(size, C, F, 5)),
            ("near keys", tm.near_keys(size, C, F, 6)), ("near exponents", tm.near_keys(size, C, F, 7, True)))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_one_call_is_the_models_bits(size, channels):
    """the levels recipe at 1, 5 and 37 frames over the four ranges with the planted n, both modes, every kind of list;
    the other inputs at 37 frames over everything and over the inner range; a scalar n"""
    pv = make(size, channels)
    B = size // 2 + 1
    turn = 0
    for F in (1, 5, 37):
        for name, x, first, nbins, n in gpu_cases(size, channels, F):
            for residual in (False, True):
                if F == 37:
                    lists = list_lengths(nbins)
                else:
                    turn += 1
                    lists = (list_lengths(nbins)[turn % 4],)
                for ln in lists:
                    check(pv, x, n, first, nbins, residual, ln, "size %d ch %d F %d %s" % (size, channels, F, name))
    for i, (name, x) in enumerate(inputs(size, channels, 37)):
        what = "size %d ch %d %s" % (size, channels, name)
        check(pv, x, tm.n_row(37, B, size + i), 0, None, bool(i & 1), B + 3, what)
        check(pv, x, tm.n_row(37, B - 5, size - i), 3, B - 5, not i & 1, 7, what)
        check(pv, x, 8, 0, None, False, 8, what + ", a scalar n")
    check(pv, analysed(size, channels, 37, 3), B // 8 + 0.5, 1, B - 1, True, 0, "size %d ch %d a scalar n" % (size, channels))


@pytest.mark.parametrize("size", [256, 1024])
def test_the_sizes_between(size):
    """W = 128, and W = 256 with two rows"""
    C, F = 2, 12
    pv = make(size, C)
    for name, x, first, nbins, n in gpu_cases(size, C, F):
        check(pv, x, n, first, nbins, first == 3, nbins + 3, "size %d %s" % (size, name))
    x = tm.near_keys(size, C, F, 9)
    check(pv, x, tm.n_row(F, size // 2 + 1, size), 0, None, False, 7, "size %d near keys" % size)


@pytest.mark.parametrize("grid_max", [1, 3])
@pytest.mark.parametrize("size", [64, 512, 2048])
def test_the_bits_do_not_depend_on_the_grid(size, grid_max, monkeypatch):
    C, F = 3, 37
    pv = make(size, C, grid_max=grid_max, monkeypatch=monkeypatch)
    for name, x, first, nbins, n in gpu_cases(size, C, F)[::2]:
        check(pv, x, n, first, nbins, grid_max == 3, nbins + 3, "size %d grid %d %s" % (size, grid_max, name))


@pytest.mark.parametrize("size", [64, 2048])
def test_a_stream_cut_into_calls_gives_the_uncut_bits(size):
    C, F = 3, 37
    pv = make(size, C)
    B = size // 2 + 1
    x = tm.levels(size, C, F, size)
    n = tm.n_row(F, B - 5, 1)
    whole, wlst = run_guarded(pv, x, n, 3, B - 5, False, 7)
    parts, lists, a = [], [], 0
    for cut in (1, 2, 5, 29):
        got, lst = run_guarded(pv, x[:, a:a + cut], n[a:a + cut], 3, B - 5, False, 7)
        parts.append(got)
        lists.append(lst)
        a += cut
    assert a == F
    same(np.concatenate(parts, axis=1), whole, "size %d cut" % size)
    assert np.array_equal(np.concatenate(lists, axis=1), wlst)


def test_a_call_on_another_stream():
    size, C, F = 512, 3, 12
    pv = make(size, C)
    name, x, first, nbins, n = gpu_cases(size, C, F)[2]
    check(pv, x, n, first, nbins, False, 7, "the current stream")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(pv, x, n, first, nbins, True, nbins + 3, "a second stream")
    check(pv, x, n, first, nbins, True, 1, "a second stream, named", stream=side)


def test_a_graph_replay_reads_the_n_of_its_time():
    size, C, F, LN = 1024, 2, 12, 9
    B = size // 2 + 1
    pv = make(size, C)
    x = tm.levels(size, C, F, 12)
    dx, out = dev(x), torch.zeros((C, F, B, 2), device=DEV)
    lst = torch.zeros((C, F, LN), dtype=torch.int32, device=DEV)
    rows = [tm.n_row(F, B, s) for s in (1, 2, 3)]
    dn = dev(rows[0])
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.trace_device(dx, out, dn, bins_out=lst) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.trace_device(dx, out, dn, bins_out=lst) == 0
    for row in rows[1:]:
        dn.copy_(torch.from_numpy(row))
        out.zero_()
        lst.zero_()
        g.replay()
        torch.cuda.synchronize()
        want, wlst = tm.trace(x, row, list_n=LN)
        same(out.cpu().numpy(), want, "replay")
        assert np.array_equal(lst.cpu().numpy(), wlst)
    assert not np.array_equal(tm.trace(x, rows[1])[0].view(np.uint32), tm.trace(x, rows[2])[0].view(np.uint32))


def _states(pv):
    return (pv.read_prev(), pv.read_phase(), pv.desc_state()) + tuple(pv.adsyn_state()) + \
        tuple(pv.time_state(op) for op in ("blur", "smooth", "freeze"))


def _equal_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_the_blocking_form_the_states_and_refused_calls():
    size, C, F = 64, 2, 9
    M = size // 2
    B = M + 1
    pv = make(size, C)
    assert pv.blur_setup(3) == 0
    # every state away from its initial value
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr, sp, sig = torch.zeros((C, F, B, 2), device=DEV), torch.zeros_like(spec), torch.zeros((C, F * pv.hop), device=DEV)
    fo, d8 = torch.zeros_like(fr), torch.zeros((C, F, 8), device=DEV)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0 and pv.adsyn_device(fr, sig) == 0
    assert pv.blur_device(fr, fo, 2.0) == 0 and pv.smooth_device(fr, fo) == 0 and pv.freeze_device(fr, fo) == 0
    assert pv.describe_device(fr, d8) == 0
    torch.cuda.synchronize()
    states = _states(pv)
    x = tm.levels(size, C, F, 21)
    n = tm.n_row(F, B - 5, 2)
    # the blocking form gives the device form's bits
    for residual in (False, True):
        got, lst = run_guarded(pv, x, n, 3, B - 5, residual, 7)
        hgot, hlst = pv.trace(x, n, 3, B - 5, residual, list_n=7)
        same(hgot, got, "host form")
        assert np.array_equal(hlst, lst) and hlst.dtype == np.int32
        same(pv.trace(x, n, 3, B - 5, residual), got, "host form without a list")
    same(pv.trace(x, 4)[0:1], tm.trace(x, np.full(F, 4, f32))[0][0:1], "host form, a scalar n")
    one = make(size, 1)
    h, hl = one.trace(x[0], n, list_n=3)
    w, wl = tm.trace(x[:1], n, list_n=3)
    same(h, w[0], "one channel, host form")
    assert np.array_equal(hl, wl[0])
    o, ol = torch.zeros((F, B, 2), device=DEV), torch.zeros((F, 3), dtype=torch.int32, device=DEV)
    assert one.trace_device(dev(x[0]), o, dev(n), bins_out=ol) == 0
    same(o.cpu().numpy(), w[0], "one channel, device form")
    assert np.array_equal(ol.cpu().numpy(), wl[0])
    assert _equal_bytes(_states(pv), states), "a trace call touched a state"
    # refused calls write nothing: overlaps by one pair or one word, bad ranges, flags through the C ABI, wrong tensors
    nf, nl = x.size, C * F * 7
    buf = torch.full((2 * nf + nl + F,), CANARY, dtype=torch.int32, device=DEV)
    fbuf = buf.view(torch.float32)
    gin, gout = fbuf[:nf].view(*x.shape), fbuf[nf:2 * nf].view(*x.shape)
    gl, gn = buf[2 * nf:2 * nf + nl].view(C, F, 7), fbuf[2 * nf + nl:]
    assert pv.trace_device(gin, fbuf[nf - 2:2 * nf - 2].view(*x.shape), gn) == CL_INVALID_VALUE
    assert pv.trace_device(fbuf[2:nf + 2].view(*x.shape), fbuf[:nf].view(*x.shape), gn) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn, bins_out=buf[2 * nf - 1:2 * nf - 1 + nl].view(C, F, 7)) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn, bins_out=buf[nf - 1:nf - 1 + nl].view(C, F, 7)) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, fbuf[2 * nf - 1:2 * nf - 1 + F]) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, fbuf[2 * nf + nl - 1:2 * nf + nl - 1 + F], bins_out=gl) == CL_INVALID_VALUE
    for first, nbins in ((0, 0), (1, M + 1), (-1, 3), (M + 1, 1), (M, 2)):
        assert pv.trace_device(gin, gout, gn, first, nbins, bins_out=gl) == CL_INVALID_VALUE, (first, nbins)
    L = fa._lib.lib()
    for flags in (2, 3, -1):
        assert L.clfa_pvoc_trace_dev(pv._h, gin.data_ptr(), gout.data_ptr(), gn.data_ptr(), gl.data_ptr(), 7, F, 0, B, flags,
                                     None) == CL_INVALID_VALUE
    assert L.clfa_pvoc_trace_dev(pv._h, gin.data_ptr(), gout.data_ptr(), gn.data_ptr(), gl.data_ptr(), 0, F, 0, B, 0,
                                 None) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout[:, :F - 1].contiguous(), gn) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn[:F - 1].contiguous()) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn.double()) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn, bins_out=gl[:, :F - 1].contiguous()) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn, bins_out=gl.float()) == CL_INVALID_VALUE
    assert pv.trace_device(gin, gout, gn, bins_out=gl[..., :0]) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, B, 2), device=DEV)
    assert pv.trace_device(e, torch.zeros_like(e), 3.0) == 0
    assert pv.trace(np.zeros((C, 0, B, 2), f32), 3).shape == (C, 0, B, 2)
    assert _equal_bytes(_states(pv), states)
    # an object without a device: a bad argument is still an invalid value, a good call the object's error
    none = fa.Pvoc(99, size, size // 4, SR, C)
    assert none.get_error() != 0 and none.trace_kernel_name() == ""
    assert none.trace_device(gin, gout, gn, 0, 0) == CL_INVALID_VALUE
    assert none.trace_device(gin, gout, gn) == none.get_error()

