"""The per-frame descriptors of clfa_pvoc on the device (pvoc_desc.hip: k_pvoc_desc, then k_pvoc_tail for the state) against
the numpy restatement of their definition (tests/pvoc_desc_model.py).

Everything is compared bit for bit with the float32 model: the sums are the header's tree of single correctly rounded
float32 additions, so there is no tolerance to choose.  Where the model gives a NaN the device gives a NaN; payloads are
not compared.  The inputs are tests/pvoc_desc_cases.py's (tests/test_pvoc_desc_cpu.py shows that they notice seven mutants
of the model) and tests/pvoc_inputs.py's analysed() frames; the outputs have the guard bands of tests/gpu_guard.py, 8-byte
and not 16-byte aligned."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import pvoc_desc_cases as dc
from tests import pvoc_desc_model as dm
from tests.gpu_guard import CANARY, DEV, bits, dev, run, same
from tests.pvoc_inputs import SR, analysed, make_pvoc

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
f32 = np.float32
assert SR == dc.SR


def make(size, channels=1, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert pv.desc_kernel_name() == "k_pvoc_desc"
    return pv


def run_guarded(pv, x, first_bin=0, nbins=None, rectify=False, stream=None):
    """one device call into a guarded output: the rows as numpy, the guard bands checked, every element written"""
    dx = dev(x)
    return run(lambda o: pv.describe_device(dx, o, first_bin, nbins, rectify, stream=stream), x.shape[:2] + (8,))


def run_cut(pv, x, cut, first_bin=0, nbins=None, rectify=False, stream=None):
    """the stream in calls of `cut` frames (the last one shorter): the rows put together"""
    F = x.shape[1]
    dx = dev(x)
    parts = []
    for a in range(0, F, cut):
        b = min(a + cut, F)
        o = torch.zeros((x.shape[0], b - a, 8), device=DEV)
        assert pv.describe_device(dx[:, a:b].contiguous(), o, first_bin, nbins, rectify, stream=stream) == 0
        parts.append(o)
    torch.cuda.synchronize()
    return torch.cat(parts, dim=1).cpu().numpy()


def check_case(pv, model, case, what):
    name, x, first, nbins, rectify = case
    what = "%s: %s" % (what, name)
    same(run_guarded(pv, x, first, nbins, rectify), model.run(x, first, nbins, rectify), what)
    assert np.array_equal(bits(pv.desc_state()), bits(x[:, -1, :, 0])), what + ": the state is the last frame's amps"
    same(pv.desc_state(), model.last, what + ": state")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", dc.SIZES + dc.MORE_SIZES)
def test_one_call_is_the_models_bits(size, channels):
    """every frame count and kind of frames over everything, every range at 37 frames; each call goes on from the state
    the one before left, ranged ones included (a ranged call stores all bins)"""
    pv = make(size, channels)
    M = size // 2
    assert pv.desc_state_bytes() >= channels * (M + 1) * 4
    assert not pv.desc_state().any()
    model = dm.Stream(channels, size, SR)
    counts = dc.FRAME_COUNTS if size in dc.SIZES else (5, 37)
    for case in dc.streams(size, channels, counts):
        check_case(pv, model, case, "size %d ch %d" % (size, channels))
    for n, F in enumerate(counts):
        x = analysed(size, channels, F, 3)
        check_case(pv, model, ("analysed F %d" % F, x, 0, None, bool(n & 1)), "size %d ch %d" % (size, channels))
    x = analysed(size, channels, counts[-1], 3)
    for name, first, nb in dc.ranges(M)[1:]:
        check_case(pv, model, ("analysed range " + name, x, first, nb, False), "size %d ch %d" % (size, channels))
    # the raw frames overflow pow and flux on purpose
    d = run_guarded(pv, dc.raw(size, channels, 5, 6))
    assert np.isinf(d[..., dm.POW]).any() and np.isinf(d[..., dm.FLUX]).any()


@pytest.mark.parametrize("size", dc.SIZES)
def test_planted_values(size):
    C = 3
    M = size // 2
    pv = make(size, C)
    model = dm.Stream(C, size, SR)
    got = {}
    for case in dc.planted(size, C):
        assert pv.reset() == 0
        model.reset()
        check_case(pv, model, case, "size %d" % size)
        assert pv.reset() == 0
        got[case[0]] = (run_guarded(pv, *case[1:]), case[1])
    sums = [dm.MAG, dm.POW, dm.MOM, dm.CENT, dm.FLUX]
    # one NaN amp, channel C - 1, frame 2: only that frame's sums and the next frame's flux are NaN; the peak ignores it
    d, x = got["one NaN amp"]
    want = np.zeros(d.shape, bool)
    want[C - 1, 2, sums] = True
    want[C - 1, 3, dm.FLUX] = True
    assert np.array_equal(np.isnan(d), want)
    # rectify drops it from the flux
    d, x = got["one NaN amp, rectified"]
    want[..., dm.FLUX] = False
    assert np.array_equal(np.isnan(d), want)
    for name in ("one NaN amp outside the range", "one NaN amp outside the range, rectified"):
        assert not np.isnan(got[name][0]).any(), name
    d, x = got["an all-NaN range"]
    assert np.array_equal(bits(d[C - 1, 1, 5:]), bits(np.array([0, 0, -1], f32))) and np.all(d[:C - 1, :, dm.PEAK_BIN] >= 3)
    d, x = got["a NaN Nyquist amp, alone in the range"]
    assert np.array_equal(bits(d[C - 1, 4, 5:]), bits(np.array([0, 0, -1], f32))) and np.isnan(d[C - 1, 4, sums]).all()
    assert np.all(np.delete(d[C - 1, :, dm.PEAK_BIN], 4) == M)
    # ties go to the lower bin
    assert got["equal maxima at M - 1 and M"][0][C - 1, 3, dm.PEAK_BIN] == M - 1
    assert got["the maximum at M alone"][0][C - 1, 3, dm.PEAK_BIN] == M
    assert np.all(got["equal maxima in one lane's neighbours"][0][:, 2, dm.PEAK_BIN] == 5)
    if M > dm.lanes(M):
        assert got["equal maxima at k and k + W"][0][C - 1, 3, dm.PEAK_BIN] == 9
        assert got["equal maxima at k + W and a higher lane's k"][0][C - 1, 3, dm.PEAK_BIN] == 11
    # zeros: cent is +0, the peak is the range's first bin with that bin's bits
    d, x = got["a frame of zeros"]
    assert not bits(d[:, 2, [dm.MAG, dm.POW, dm.MOM, dm.CENT, dm.PEAK_AMP, dm.PEAK_BIN]]).any()
    d, x = got["a frame of -0"]
    assert np.all(bits(d[:, 2, dm.MAG]) == 0x80000000) and not bits(d[:, 2, [dm.POW, dm.CENT]]).any()
    assert np.all(bits(d[:, 2, dm.PEAK_AMP]) == 0x80000000) and not d[:, 2, dm.PEAK_BIN].any()
    d, x = got["-0 below +0"]
    assert np.all(bits(d[:, 1, dm.PEAK_AMP]) == 0x80000000) and np.all(d[:, 1, dm.PEAK_BIN] == 4)
    d, x = got["+0 below -0"]
    assert np.all(bits(d[:, 1, dm.PEAK_AMP]) == 0) and np.all(d[:, 1, dm.PEAK_BIN] == 4)
    d, x = got["negative amps, the largest a -0"]
    assert bits(d[C - 1, 2, dm.PEAK_AMP]) == 0x80000000 and d[C - 1, 2, dm.PEAK_BIN] == M // 2


@pytest.mark.parametrize("grid_max", [None, 1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 256, 1024])
def test_the_bits_do_not_depend_on_how_the_stream_is_cut_or_on_the_grid(size, channels, grid_max, monkeypatch):
    F = 37
    M = size // 2
    pv = make(size, channels, grid_max=grid_max, monkeypatch=monkeypatch)
    x = dc.raw(size, channels, F, 4) if channels == 1 else analysed(size, channels, F, 3)
    for first, nbins, rectify in ((0, None, False), (M // 4, M // 2, True)):
        what = "size %d ch %d grid %s range %d %s" % (size, channels, grid_max, first, nbins)
        want = dm.Stream(channels, size, SR).run(x, first, nbins, rectify)
        for cut in (F, 1, 2, 5, F - 8):
            assert pv.reset() == 0
            same(run_cut(pv, x, cut, first, nbins, rectify), want, "%s cut %d" % (what, cut))
            assert np.array_equal(bits(pv.desc_state()), bits(x[:, -1, :, 0])), "%s cut %d: state" % (what, cut)


def test_a_call_on_another_stream_goes_on_from_the_first():
    size, C, F = 1024, 3, 11
    pv = make(size, C)
    x = analysed(size, C, 2 * F, 3)
    want = dm.Stream(C, size, SR).run(x)
    side = torch.cuda.Stream()
    first = run_cut(pv, x[:, :F], F)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run_cut(pv, x[:, F:], F)
    same(np.concatenate([first, second], axis=1), want, "two streams")
    assert np.array_equal(bits(pv.desc_state()), bits(x[:, -1, :, 0]))


def test_a_graph_replay_advances_the_state():
    size, C, F = 1024, 2, 3
    pv = make(size, C)
    x = analysed(size, C, F, 3)
    dx = dev(x)
    out = torch.zeros((C, F, 8), device=DEV)
    model = dm.Stream(C, size, SR)
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.describe_device(dx, out) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fresh = model.run(x)
    same(out.cpu().numpy(), fresh, "warm-up")
    assert pv.reset() == 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.describe_device(dx, out) == 0
    torch.cuda.synchronize()
    assert not pv.desc_state().any(), "the capture itself ran nothing"
    model.reset()
    for i in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = model.run(x)
        same(out.cpu().numpy(), want, "replay %d" % i)
        assert np.array_equal(bits(pv.desc_state()), bits(x[:, -1, :, 0]))
    # the second replay's frame 0 took its flux against the input's last frame, not against the reset state
    assert not np.array_equal(bits(want[:, 0, dm.FLUX]), bits(fresh[:, 0, dm.FLUX]))
    assert np.array_equal(bits(want[:, 1:]), bits(fresh[:, 1:]))


def _other_states(pv):
    return (pv.read_prev(), pv.read_phase()) + tuple(pv.adsyn_state()) + tuple(pv.time_state(op) for op in ("blur", "smooth", "freeze"))


def _equal_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_failed_calls_reset_the_other_states_and_the_blocking_form():
    size, C, F = 64, 2, 9
    M = size // 2
    pv = make(size, C)
    assert pv.blur_setup(3) == 0
    fresh = _other_states(pv)
    # the other states away from their initial values
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr, sp, sig = torch.zeros((C, F, M + 1, 2), device=DEV), torch.zeros_like(spec), torch.zeros((C, F * pv.hop), device=DEV)
    fo = torch.zeros_like(fr)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0 and pv.adsyn_device(fr, sig) == 0
    assert pv.blur_device(fr, fo, 2.0) == 0 and pv.smooth_device(fr, fo) == 0 and pv.freeze_device(fr, fo) == 0
    torch.cuda.synchronize()
    other = _other_states(pv)
    assert not any(_equal_bytes([a], [b]) for a, b in zip(other, fresh))
    x = dc.plain(size, C, F, 2)
    model = dm.Stream(C, size, SR)
    same(run_guarded(pv, x, 2, 9, True), model.run(x, 2, 9, True), "a ranged call")
    assert _equal_bytes(_other_states(pv), other), "the call touched another state"
    # failed calls: an output that overlaps the input by one float from either side, bad ranges; nothing is written and
    # the state stays
    state = pv.desc_state()
    assert np.array_equal(bits(state), bits(x[:, -1, :, 0]))
    n, m = x.size, C * F * 8
    buf = torch.full((n + m,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    assert pv.describe_device(buf[:n].view(*x.shape), buf[n - 1:n - 1 + m].view(C, F, 8)) == CL_INVALID_VALUE
    assert pv.describe_device(buf[m:].view(*x.shape), buf[1:m + 1].view(C, F, 8)) == CL_INVALID_VALUE
    good_in, good_out = buf[:n].view(*x.shape), buf[n:].view(C, F, 8)
    for first, nbins in ((0, 0), (1, M + 1), (-1, 3), (M + 1, 1), (M, 2)):
        assert pv.describe_device(good_in, good_out, first, nbins) == CL_INVALID_VALUE, (first, nbins)
    assert pv.describe_device(good_in, good_out[:, :F - 1].contiguous()) == CL_INVALID_VALUE
    assert pv.describe_device(good_in[:, :, :M].contiguous(), good_out) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == CANARY).all())
    assert np.array_equal(bits(pv.desc_state()), bits(state))
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, M + 1, 2), device=DEV)
    assert pv.describe_device(e, torch.zeros((C, 0, 8), device=DEV)) == 0
    assert pv.describe(np.zeros((C, 0, M + 1, 2), f32)).shape == (C, 0, 8)
    assert np.array_equal(bits(pv.desc_state()), bits(state))
    # the blocking form is the device form, and goes on from the same state
    y = dc.raw(size, C, F, 8)
    same(pv.describe(y), model.run(y), "host form")
    same(pv.describe(x, first_bin=M, rectify=True), model.run(x, M, None, True), "host form, the Nyquist bin, rectified")
    with pytest.raises(fa.ClError):
        pv.describe(x, first_bin=3, nbins=M)
    assert np.array_equal(bits(pv.desc_state()), bits(x[:, -1, :, 0]))
    assert _equal_bytes(_other_states(pv), other)
    # one channel: (F, M + 1, 2) -> (F, 8)
    one = make(size, 1)
    same(one.describe(x[0]), dm.Stream(1, size, SR).run(x[:1])[0], "one channel, host form")
    o = torch.zeros((F, 8), device=DEV)
    assert one.reset() == 0 and one.describe_device(dev(x[0]), o) == 0
    same(o.cpu().numpy(), dm.Stream(1, size, SR).run(x[:1])[0], "one channel, device form")
    # reset: the EMPTY amps, and every other state as at creation
    assert pv.reset() == 0
    assert not bits(pv.desc_state()).any()
    assert _equal_bytes(_other_states(pv), fresh)
    model.reset()
    same(run_guarded(pv, x), model.run(x), "after the reset")
    # an object without a device: a bad argument is still an invalid value, a good call the object's error
    none = fa.Pvoc(99, size, size // 4, SR, C)
    assert none.get_error() != 0 and none.desc_kernel_name() == ""
    assert none.describe_device(good_in, good_out, 0, 0) == CL_INVALID_VALUE
    assert none.describe_device(good_in, good_out) == none.get_error()
    with pytest.raises(fa.ClError):
        none.desc_state()
