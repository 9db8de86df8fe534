"""The operations along the frames of clfa_pvoc on the device (pvoc_time.hip: k_pvoc_blur, k_pvoc_smooth, k_pvoc_freeze)
against the numpy restatement of their definitions (tests/pvoc_time_model.py).

Everything is compared bit for bit with the float32 model: an output value is a fixed sequence of single correctly rounded
float32 operations on the stream's values, so there is no tolerance to choose.  Where the model gives a NaN the device gives
a NaN; payloads are not compared.  The frames are tests/pvoc_inputs.py's analysed() and raw(), the guard bands those of
tests/gpu_guard.py."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import pvoc_model as pm
from tests import pvoc_time_model as tm
from tests import stft_model
from tests.gpu_guard import CANARY, DEV, bits, dev, flat, run, same
from tests.pvoc_inputs import SR, analysed, hann, make_pvoc, raw

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
CL_INVALID_OPERATION = -59
f32 = np.float32
OPS = (tm.BLUR, tm.SMOOTH, tm.FREEZE)
MAX_FRAMES = (1, 2, 7, 40)


def make(size, channels=1, max_frames=None, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert [pv.time_kernel_name(op) for op in OPS] == ["k_pvoc_blur", "k_pvoc_smooth", "k_pvoc_freeze"]
    if max_frames is not None:
        assert pv.blur_setup(max_frames) == 0 and pv.blur_max_frames() == max_frames
    return pv


def frames_of(kind, size, C, F, seed=3):
    return analysed(size, C, F, seed) if kind == "analysed" else raw(size, C, F, seed + 1)


def per_frame(op, F, max_frames=1, seed=0):
    """(p, q) of F frames for the device form, the awkward values among them as soon as F allows.  Blur: lengths below 1,
    fractional, a NaN and values above max_frames; smooth: weights 0, 1, outside [0, 1] and a NaN; freeze: flags that are
    0, -0, 1, a fraction, negative and a NaN, about half of them 0"""
    rng = np.random.default_rng(1000 * op + F + seed)
    if op == tm.BLUR:
        p = rng.uniform(0.0, max_frames + 3.0, F).astype(f32)
        pool = np.array([max_frames, np.nan, max_frames + 100.0, 1.0, 0.5, 2.7, np.inf, -4.0], f32)
        p[:min(F, pool.size)] = pool[:F]
        return p, None
    if op == tm.SMOOTH:
        pools = (np.array([0.6, 0.0, 1.0, -0.5, np.nan, 1.5, 0.25, 2.0 ** -20], f32), np.array([1.0, 0.3, 0.0, np.nan, 7.0, 0.5], f32))
        lo, hi = -0.3, 1.3
    else:
        pools = (np.array([0.0, 1.0, np.nan, -0.0, 0.5, 0.0, -2.0], f32), np.array([1.0, 0.0, 0.0, 1.0, np.nan, 1.0], f32))
        lo, hi = 0.0, 1.0
    out = []
    for pool in pools:
        v = rng.uniform(lo, hi, F).astype(f32)
        if op == tm.FREEZE:
            v = (v < 0.5).astype(f32)
        v[:min(F, pool.size)] = pool[:F]
        out.append(v)
    return tuple(out)


def call(pv, op, x, o, p, q, stream=None):
    if op == tm.BLUR:
        return pv.blur_device(x, o, p, stream=stream)
    return (pv.smooth_device if op == tm.SMOOTH else pv.freeze_device)(x, o, p, q, stream=stream)


def dev_pq(p, q):
    return dev(p), None if q is None else dev(q)


def run_guarded(pv, op, x, p, q):
    """one device call into a guarded output: the result as numpy, the guard bands checked, every element written"""
    dx, (dp, dq) = dev(x), dev_pq(p, q)
    return run(lambda o: call(pv, op, dx, o, dp, dq), x.shape)


def run_cut(pv, op, x, p, q, cut, stream=None):
    """the stream in calls of `cut` frames (the last one shorter): the outputs put together"""
    F = x.shape[1]
    out = torch.zeros(x.shape, device=DEV)
    dx = dev(x)
    for a in range(0, F, cut):
        b = min(a + cut, F)
        o = torch.zeros((x.shape[0], b - a) + x.shape[2:], device=DEV)
        dp, dq = dev_pq(p[a:b], None if q is None else q[a:b])
        assert call(pv, op, dx[:, a:b].contiguous(), o, dp, dq, stream=stream) == 0
        out[:, a:b] = o
    torch.cuda.synchronize()
    return out.cpu().numpy()


def variants():
    """(op, max_frames) of every case: the blur at each history length"""
    return [(tm.BLUR, m) for m in MAX_FRAMES] + [(tm.SMOOTH, None), (tm.FREEZE, None)]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_one_call_is_the_models_bits(size, channels):
    pv = make(size, channels)
    assert pv.time_state_bytes() == 2 * channels * (size // 2 + 1) * 8
    for F in (1, 5, 37, 200):
        for kind in ("analysed", "raw"):
            x = frames_of(kind, size, channels, F)
            for op, max_frames in variants():
                what = "size %d ch %d F %d %s %s max_frames %s" % (size, channels, F, kind, tm.NAMES[op], max_frames)
                if op == tm.BLUR:
                    assert pv.blur_setup(max_frames) == 0
                else:
                    assert pv.reset() == 0
                model = tm.Stream(channels, size, SR, max_frames)
                p, q = per_frame(op, F, max_frames or 1)
                same(run_guarded(pv, op, x, p, q), model.run(op, x, p, q), what)
                same(pv.time_state(op), model.state(op), what + ": state")
                # a second call goes on from the first one's state; plain numbers as per-frame values
                num = (3.0, None) if op == tm.BLUR else ((0.3, 0.6) if op == tm.SMOOTH else (1.0, 0.0))
                g = flat(x.shape)
                assert call(pv, op, dev(x), g.data, num[0], num[1]) == 0
                torch.cuda.synchronize()
                assert g.intact()
                same(g.data.cpu().numpy(), model.run(op, x, num[0], num[1]), what + ": second call")
                same(pv.time_state(op), model.state(op), what + ": state after the second call")
    assert pv.time_state_bytes() == 2 * channels * (size // 2 + 1) * 8 * (1 + 39)


@pytest.mark.parametrize("grid_max", [None, 1, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_the_bits_do_not_depend_on_how_the_stream_is_cut(size, channels, grid_max, monkeypatch):
    F = 37
    pv = make(size, channels, grid_max=grid_max, monkeypatch=monkeypatch)
    x = frames_of("raw" if channels == 1 else "analysed", size, channels, F)
    for op, max_frames in variants():
        what = "size %d ch %d grid %s %s max_frames %s" % (size, channels, grid_max, tm.NAMES[op], max_frames)
        p, q = per_frame(op, F, max_frames or 1)
        model = tm.Stream(channels, size, SR, max_frames)
        want = model.run(op, x, p, q)
        for cut in (F, 1, 2, 5, F - 8):
            if op == tm.BLUR:
                assert pv.blur_setup(max_frames) == 0
            else:
                assert pv.reset() == 0
            same(run_cut(pv, op, x, p, q, cut), want, "%s cut %d" % (what, cut))
            same(pv.time_state(op), model.state(op), "%s cut %d: state" % (what, cut))


def test_a_call_on_another_stream_goes_on_from_the_first():
    size, C, F = 1024, 3, 11
    pv = make(size, C, max_frames=7)
    x = frames_of("analysed", size, C, 2 * F)
    side = torch.cuda.Stream()
    for op in OPS:
        p, q = per_frame(op, 2 * F, 7)
        model = tm.Stream(C, size, SR, 7)
        want = model.run(op, x, p, q)
        first = run_cut(pv, op, x[:, :F], p[:F], None if q is None else q[:F], F)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            second = run_cut(pv, op, x[:, F:], p[F:], None if q is None else q[F:], F)
        same(np.concatenate([first, second], axis=1), want, tm.NAMES[op])
        same(pv.time_state(op), model.state(op), tm.NAMES[op] + ": state")


@pytest.mark.parametrize("op", OPS)
def test_a_graph_replay_advances_the_state(op):
    size, C, F, max_frames = 1024, 2, 3, 7
    pv = make(size, C, max_frames=max_frames)
    x = frames_of("analysed", size, C, F)
    p, q = per_frame(op, F, max_frames, seed=5)
    if op == tm.BLUR:
        p = np.array([7.0, 3.0, 5.5], f32)
    dx, (dp, dq) = dev(x), dev_pq(p, q)
    out = torch.zeros(x.shape, device=DEV)
    model = tm.Stream(C, size, SR, max_frames)
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert call(pv, op, dx, out, dp, dq) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same(out.cpu().numpy(), model.run(op, x, p, q), "warm-up")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call(pv, op, dx, out, dp, dq) == 0
    torch.cuda.synchronize()
    same(pv.time_state(op), model.state(op), "the capture itself ran nothing")
    for i in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        same(out.cpu().numpy(), model.run(op, x, p, q), "replay %d" % i)
        same(pv.time_state(op), model.state(op), "state after replay %d" % i)
    # the setup is refused while the object's stream is being captured
    if op == tm.BLUR:
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2):
            assert call(pv, op, dx, out, dp, dq) == 0
            assert pv.blur_setup(9) == CL_INVALID_OPERATION
        assert pv.blur_max_frames() == max_frames


def test_nans_stay_where_the_definitions_put_them():
    size, C, F = 64, 2, 12
    M = size // 2
    pv = make(size, C, max_frames=7)
    x = np.array(frames_of("analysed", size, C, F))
    clean = tm.Stream(C, size, SR, 7)
    # blur: a NaN in the history that no window of the call reaches (windows of 3 frames look 2 frames back; the NaN is
    # 4 frames back), then windows of 7 frames, which reach it
    bad = x.copy()
    bad[1, F - 4, M // 3, 0] = np.nan
    lengths = np.full(F, 3.0, f32)
    model = tm.Stream(C, size, SR, 7)
    same(run_guarded(pv, tm.BLUR, bad, lengths, None), model.run(tm.BLUR, bad, lengths), "blur: the NaN's own call")
    clean.run(tm.BLUR, x, lengths)
    got = run_guarded(pv, tm.BLUR, x, lengths, None)
    assert not np.isnan(got).any()
    assert np.isnan(pv.time_state("blur")).sum() == 0 and np.isnan(model.run(tm.BLUR, x, lengths)).sum() == 0
    same(got, clean.run(tm.BLUR, x, lengths), "blur: the NaN is outside every window")
    assert pv.blur_setup(7) == 0
    model = tm.Stream(C, size, SR, 7)
    for fr, n in ((bad, 3.0), (x, 7.0)):
        got, want = run_guarded(pv, tm.BLUR, fr, np.full(F, n, f32), None), model.run(tm.BLUR, fr, np.full(F, n, f32))
        same(got, want, "blur: windows of %g" % n)
    hit = np.zeros(x.shape, bool)
    hit[1, :3, M // 3, 0] = True          # the NaN is frame -4 of the second call: inside the windows of frames 0, 1, 2
    assert np.array_equal(np.isnan(got), hit)
    # freeze: a NaN in a frozen frame's input stays out
    flag = np.zeros(F, f32)
    flag[5] = 1
    bad = x.copy()
    bad[:, 5] = np.nan
    got = run_guarded(pv, tm.FREEZE, bad, flag, flag)
    assert not np.isnan(got).any() and np.array_equal(bits(got[:, 5]), bits(x[:, 4]))
    want = x.copy()
    want[:, 5] = x[:, 4]
    assert np.array_equal(bits(got), bits(want))
    # smooth: weight 1 after a NaN state returns the input's bits
    nan_frame = np.full((C, 1, M + 1, 2), np.nan, f32)
    run_guarded(pv, tm.SMOOTH, nan_frame, np.ones(1, f32), np.ones(1, f32))
    assert np.isnan(pv.time_state("smooth")).all()
    w = np.full(F, 0.5, f32)
    w[0] = 1.0
    got = run_guarded(pv, tm.SMOOTH, x, w, np.ones(F, f32))
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got[..., 1]), bits(x[..., 1])) and np.array_equal(bits(got[:, 0]), bits(x[:, 0]))
    # ... and weight 0 keeps it: a NaN state that no frame replaces stays a NaN
    run_guarded(pv, tm.SMOOTH, nan_frame, np.ones(1, f32), np.ones(1, f32))
    got = run_guarded(pv, tm.SMOOTH, x, np.zeros(F, f32), np.ones(F, f32))
    assert np.isnan(got[..., 0]).all() and np.array_equal(bits(got[..., 1]), bits(x[..., 1]))


def _older_states(pv):
    return (pv.read_prev(), pv.read_phase()) + tuple(pv.adsyn_state())


def _equal_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_failed_calls_reset_and_the_older_states():
    size, C, F = 64, 2, 9
    M = size // 2
    fresh = _older_states(make(size, C))
    pv = make(size, C, max_frames=5)
    # the older states away from their initial values
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr, sp, sig = torch.zeros((C, F, M + 1, 2), device=DEV), torch.zeros_like(spec), torch.zeros((C, F * pv.hop), device=DEV)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0 and pv.adsyn_device(fr, sig) == 0
    torch.cuda.synchronize()
    older = _older_states(pv)
    assert not _equal_bytes(older, fresh)
    x = frames_of("analysed", size, C, F)
    model = tm.Stream(C, size, SR, 5)
    for op in OPS:
        p, q = per_frame(op, F, 5)
        same(run_guarded(pv, op, x, p, q), model.run(op, x, p, q), tm.NAMES[op])
    assert _equal_bytes(_older_states(pv), older), "the new calls touched an older state"
    # a failed call (an output that overlaps the input by one pair) leaves every state as it was, and writes nothing
    states = [pv.time_state(op) for op in OPS]
    n = x.size
    buf = torch.full((2 * n,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    lo, hi = buf[:n].view(*x.shape), buf[n - 2:2 * n - 2].view(*x.shape)
    s = dev(np.full(F, 1.0, f32))
    for op in OPS:
        assert call(pv, op, lo, hi, s, None if op == tm.BLUR else s) == CL_INVALID_VALUE
        assert call(pv, op, hi, lo, s, None if op == tm.BLUR else s) == CL_INVALID_VALUE
        assert call(pv, op, lo, lo, s, None if op == tm.BLUR else s) == CL_INVALID_VALUE
        assert call(pv, op, dev(x)[:, :4].contiguous(), hi, s, None if op == tm.BLUR else s) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == CANARY).all())
    for op, st in zip(OPS, states):
        assert np.array_equal(bits(pv.time_state(op)), bits(st)), tm.NAMES[op]
        same(st, model.state(op), tm.NAMES[op])
    with pytest.raises(fa.ClError):
        pv.blur(x, 6.0)                       # the blocking form checks the lengths against max_frames
    assert all(np.array_equal(bits(pv.time_state(op)), bits(st)) for op, st in zip(OPS, states))
    # the blocking forms are the device forms
    for op, host in ((tm.BLUR, lambda: pv.blur(x, 4.0)), (tm.SMOOTH, lambda: pv.smooth(x, 0.25, 1.0)), (tm.FREEZE, lambda: pv.freeze(x, 1.0, 0.0))):
        args = {tm.BLUR: (4.0, None), tm.SMOOTH: (0.25, 1.0), tm.FREEZE: (1.0, 0.0)}[op]
        same(host(), model.run(op, x, *args), "host form of " + tm.NAMES[op])
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, M + 1, 2), device=DEV)
    for op in OPS:
        assert call(pv, op, e, e.clone(), s[:0].contiguous(), None if op == tm.BLUR else s[:0].contiguous()) == 0
    # reset: EMPTY everywhere, and the analysis / synthesis / oscillator states as at creation
    assert pv.reset() == 0
    model.reset()
    for op in OPS:
        assert np.array_equal(bits(pv.time_state(op)), bits(model.state(op))), tm.NAMES[op]
    assert pv.blur_max_frames() == 5 and pv.time_state("blur").shape == (C, 4, M + 1, 2)
    assert _equal_bytes(_older_states(pv), fresh)
    # a blur before its setup
    other = make(size, C)
    assert other.blur_device(dev(x), torch.zeros(x.shape, device=DEV), 2.0) == CL_INVALID_OPERATION
    with pytest.raises(fa.ClError) as err:
        other.time_state("blur")
    assert err.value.code == CL_INVALID_OPERATION


def _tone_db(y, lo, nfft, k0):
    """the tone's energy (bin k0 of an nfft-point transform and its two neighbours) over the rest, in dB"""
    X = np.abs(np.fft.rfft(np.asarray(y[lo:lo + nfft], np.float64) * np.hanning(nfft))) ** 2
    tone = np.zeros(X.size, bool)
    tone[k0 - 2:k0 + 3] = True
    return 10 * np.log10(X[tone].sum() / X[~tone].sum())


def test_end_to_end_blur_of_a_steady_tone_in_noise():
    """a sanity check, not a contract: Stft -> Pvoc.analyze -> blur(n = 8) -> synthesize -> Stft synthesis of a steady tone
    in noise, the tone-to-noise ratio printed beside the numpy chain's and the unblurred signal's"""
    size, hop, F, nfft, n = 1024, 256, 64, 8192, 8
    N = size + (F - 1) * hop
    k0 = 40 * 8                                             # bin 40 of a 1024-point frame
    rng = np.random.default_rng(31)
    x = (0.5 * np.cos(2 * np.pi * k0 / nfft * np.arange(N) + 0.4) + 0.1 * rng.standard_normal(N)).astype(f32)
    w, lo = hann(size), 4 * size
    # the numpy chain
    fr = stft_model.windowed_frames_f32(x[None], size, hop, w)
    P = fa.onesided_to_packed(np.fft.rfft(fr.astype(np.float64), axis=-1)).astype(np.complex64)
    frames = pm.analyze32(P, pm.initial_prev(1, size), size, hop, SR)
    blurred, _ = tm.blur32(frames, float(n), tm.empty(1, size, SR, n - 1), n)
    th, _ = pm.phases(blurred[..., 1], pm.initial_phase(1, size), hop, SR)
    r = np.fft.irfft(fa.packed_to_onesided(pm.synth32(blurred, th).astype(np.complex128)), n=size, axis=-1)
    want_db = _tone_db(stft_model.overlap_add(r, w, hop, normalize=True)[0][0], lo, nfft, k0)
    # the device chain
    an, sy = fa.Stft(0, size, hop, window=w), fa.Stft(0, size, hop, window=w, fwd=False)
    pv = make(size, 1, max_frames=n)
    y = sy.synthesize(pv.synthesize(pv.blur(pv.analyze(an.analyze(x[None])), float(n))), normalize=True)[0]
    got_db, in_db = _tone_db(y, lo, nfft, k0), _tone_db(x, lo, nfft, k0)
    print("PVOCTIME end to end: tone over rest %.2f dB (numpy chain %.2f dB, the input %.2f dB)" % (got_db, want_db, in_db))
    assert np.isfinite(got_db) and np.isfinite(want_db)
