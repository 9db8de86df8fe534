"""The operations along the frames of clfa_pvoc (blur, smooth, freeze) without a GPU: the library's new symbols and
argument checks — which come before any device lookup, so they answer on a machine without a device too — and properties
of the numpy model of their definitions (tests/pvoc_time_model.py)."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_ops_model as om
from tests import pvoc_time_model as tm

CL_INVALID_VALUE = -30
CL_INVALID_OPERATION = -59
SR = 48000.0
f32 = np.float32
OPS = (tm.BLUR, tm.SMOOTH, tm.FREEZE)


def _frames(rng, C, F, size):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    return np.stack([amp, freq], axis=-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_time_symbols():
    names = ["clfa_pvoc_blur_setup", "clfa_pvoc_time_dev", "clfa_pvoc_time", "clfa_pvoc_time_read_state",
             "clfa_pvoc_time_state_bytes", "clfa_pvoc_blur_max_frames", "clfa_pvoc_time_kernel_name"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.time_kernel_name("blur") == "" and bad.time_kernel_name(2) == ""
    assert bad.blur_max_frames() == 0 and bad.blur_setup(4) == CL_INVALID_VALUE
    pv = fa.Pvoc(0, 64, 16, SR)
    if pv.get_error() == 0:
        assert [pv.time_kernel_name(op) for op in ("blur", "smooth", "freeze", "nothing", 0, 1, 2, 3, -1)] == \
            ["k_pvoc_blur", "k_pvoc_smooth", "k_pvoc_freeze", "", "k_pvoc_blur", "k_pvoc_smooth", "k_pvoc_freeze", "", ""]
    else:
        assert pv.time_kernel_name("blur") == ""
    assert pv.blur_max_frames() == 0
    for m in ("blur", "smooth", "freeze"):
        assert callable(getattr(pv, m)) and callable(getattr(pv, m + "_device"))
    for m in ("blur_setup", "time_state", "time_state_bytes", "time_kernel_name", "smooth_weight"):
        assert callable(getattr(pv, m))


def test_smooth_weight_is_csounds_map():
    for cutoff in (0.01, 0.1, 0.5, 1.0):
        g = 2.0 - np.cos(np.pi * cutoff)
        assert fa.Pvoc.smooth_weight(cutoff) == 1.0 + np.sqrt(g * g - 1.0) - g
    assert fa.Pvoc.smooth_weight(0.0) == 0.0
    w = [fa.Pvoc.smooth_weight(c) for c in np.linspace(0, 1, 11)]
    assert all(a < b for a, b in zip(w, w[1:])) and 0.0 <= w[0] and w[-1] < 1.0


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    rng = np.random.default_rng(5)
    a = _frames(rng, C, F, size)
    out = np.full_like(a, 7.0)
    par, par2 = np.full(F, 0.5, f32), np.full(F, 0.25, f32)
    length = np.full(F, 2.0, f32)
    ptr = lambda x: None if x is None else x.ctypes.data

    def defaults(op, p, q):
        return (length if op == tm.BLUR else par) if p is ... else p, par2 if q is ... else q

    def host(op, a=a, o=out, F=F, p=..., q=..., h=pv._h):
        p, q = defaults(op, p, q)
        return L.clfa_pvoc_time(h, op, ptr(a), ptr(o), F, ptr(p), ptr(q))

    def devf(op, a=a, o=out, F=F, p=..., q=...):      # the device form's checks, on host addresses
        p, q = defaults(op, p, q)
        return L.clfa_pvoc_time_dev(pv._h, op, ptr(a), ptr(o), F, ptr(p), ptr(q), None)

    # the blur before its setup: every argument error first, then CL_INVALID_OPERATION, with or without a device
    assert pv.blur_max_frames() == 0
    assert host(tm.BLUR) == CL_INVALID_OPERATION and devf(tm.BLUR) == CL_INVALID_OPERATION
    assert host(tm.BLUR, q=None) == CL_INVALID_OPERATION and devf(tm.BLUR, q=None) == CL_INVALID_OPERATION
    assert host(tm.BLUR, F=-1) == CL_INVALID_VALUE and host(tm.BLUR, a=None) == CL_INVALID_VALUE
    assert host(tm.BLUR, o=a) == CL_INVALID_VALUE and devf(tm.BLUR, p=None) == CL_INVALID_VALUE
    assert host(tm.BLUR, p=np.array([1.0, 0.5, 1.0], f32)) == CL_INVALID_VALUE      # the values come before it as well
    assert host(tm.BLUR, p=np.array([1.0, np.nan, 1.0], f32)) == CL_INVALID_VALUE
    assert host(tm.BLUR, F=0) == good and devf(tm.BLUR, F=0) == good                # nothing to do: no history needed
    with pytest.raises(fa.ClError) as e:
        pv.time_state("blur")
    assert e.value.code == (CL_INVALID_OPERATION if good == 0 else good)
    # the setup's range, before the device lookup
    for bad_max in (0, 4097, -1):
        assert pv.blur_setup(bad_max) == CL_INVALID_VALUE
        assert L.clfa_pvoc_blur_setup(pv._h, bad_max) == CL_INVALID_VALUE
    assert L.clfa_pvoc_blur_setup(None, 4) == CL_INVALID_VALUE
    assert pv.blur_max_frames() == 0
    assert pv.blur_setup(4) == good and pv.blur_setup(1) == good and pv.blur_setup(4096 if good == 0 else 4) == good
    assert pv.blur_setup(4) == good
    assert pv.blur_max_frames() == (4 if good == 0 else 0)
    ops = OPS if good == 0 else (tm.SMOOTH, tm.FREEZE)      # without a device the blur cannot be set up
    for op in ops:
        assert host(op) == good, op
        assert host(op, F=0) == good and devf(op, F=0) == good
        assert host(op, F=-1) == CL_INVALID_VALUE and devf(op, F=-1) == CL_INVALID_VALUE
        for name in ("a", "o", "p"):
            assert host(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
            assert devf(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
        # an output overlapping the input by one element, or being it
        both = np.zeros(2 * a.size, f32)
        lo, hi = both[:a.size].reshape(a.shape), both[a.size - 1:2 * a.size - 1].reshape(a.shape)
        lo[...] = a
        assert host(op, a=lo, o=hi) == CL_INVALID_VALUE and host(op, a=hi, o=lo) == CL_INVALID_VALUE
        assert devf(op, a=lo, o=hi) == CL_INVALID_VALUE and host(op, a=a, o=a) == CL_INVALID_VALUE
        # an output overlapping p or q by one element
        buf = np.zeros(a.size + F, f32)
        o2, tail = buf[:a.size].reshape(a.shape), buf[a.size - 1:a.size - 1 + F]
        assert host(op, o=o2, p=tail) == CL_INVALID_VALUE and devf(op, o=o2, p=tail) == CL_INVALID_VALUE
        if op != tm.BLUR:
            assert host(op, o=o2, q=tail) == CL_INVALID_VALUE and devf(op, o=o2, q=tail) == CL_INVALID_VALUE
            assert host(op, q=None) == CL_INVALID_VALUE and devf(op, q=None) == CL_INVALID_VALUE
            assert host(op, p=par, q=par) == good                   # p and q may be the same array
            buf[a.size:] = 0.5
            assert host(op, o=o2, p=buf[a.size:], q=buf[a.size:]) == good
    for bad_op in (-1, 3, 99):
        assert host(bad_op) == CL_INVALID_VALUE and devf(bad_op) == CL_INVALID_VALUE
        assert L.clfa_pvoc_time_read_state(pv._h, bad_op, ptr(out)) == CL_INVALID_VALUE
    assert L.clfa_pvoc_time_read_state(pv._h, tm.SMOOTH, None) == CL_INVALID_VALUE
    # BLUR does not look at q: NULL, or an array that overlaps the output
    if good == 0:
        buf = np.zeros(a.size + F, f32)
        o2, tail = buf[:a.size].reshape(a.shape), buf[a.size - 1:a.size - 1 + F]
        assert host(tm.BLUR, q=None) == good and host(tm.BLUR, o=o2, q=tail) == good
    # the blocking form checks the values
    nan_, inf_, wide = np.array([0.5, np.nan, 1.0], f32), np.array([np.inf, 0, 0], f32), np.array([0.0, 1.5, 1.0], f32)
    for op in (tm.SMOOTH, tm.FREEZE):
        assert host(op, p=nan_) == CL_INVALID_VALUE and host(op, q=nan_) == CL_INVALID_VALUE, op
        assert host(op, p=inf_) == CL_INVALID_VALUE and host(op, q=-inf_) == CL_INVALID_VALUE, op
    assert host(tm.SMOOTH, p=wide) == CL_INVALID_VALUE and host(tm.SMOOTH, q=wide) == CL_INVALID_VALUE
    assert host(tm.SMOOTH, q=-wide) == CL_INVALID_VALUE
    assert host(tm.SMOOTH, p=np.array([0, 1, 0.5], f32), q=np.array([1, 0, 1], f32)) == good
    assert host(tm.FREEZE, p=wide, q=-wide) == good                 # any finite flag
    if good == 0:
        assert host(tm.BLUR, p=np.array([1.0, 4.0, 2.5], f32)) == good
        for bad_len in (np.array([1.0, 4.5, 1.0], f32), np.array([0.99, 1, 1], f32), np.array([1, 1, 5], f32), nan_ * 4, inf_):
            assert host(tm.BLUR, p=bad_len) == CL_INVALID_VALUE
    assert L.clfa_pvoc_time(None, 1, ptr(a), ptr(out), F, ptr(par), ptr(par2)) == CL_INVALID_VALUE
    if good != 0:
        assert (out == 7.0).all()          # nothing was computed anywhere
    # an object whose creation arguments were bad keeps answering with that error
    assert host(tm.SMOOTH, h=fa.Pvoc(0, 48, 16, SR)._h) == CL_INVALID_VALUE
    # the Python forms: plain numbers for the per-frame arrays; the status raised as ClError
    if good != 0:
        with pytest.raises(fa.ClError):
            pv.smooth(a, 0.5, 0.5)
    for call in (lambda: pv.smooth(a, amp=1.5), lambda: pv.smooth(a, freq=-0.1), lambda: pv.freeze(a, np.nan, 0),
                 lambda: pv.freeze(a, 0, np.inf), lambda: pv.blur(a, 0.5), lambda: pv.blur(a, np.nan)):
        with pytest.raises(fa.ClError) as e:
            call()
        assert e.value.code == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        pv.smooth(a[:, :, :5])


# ---- the model's own properties ----

F_ALL = 37
CUTS = (1, 2, 5, F_ALL - 8)


def _stream_inputs(seed=3, size=64, C=2, F=F_ALL):
    rng = np.random.default_rng(seed)
    fr = _frames(rng, C, F, size)
    length = rng.uniform(0.0, 45.0, F).astype(f32)
    length[[3, 11]] = np.nan, 1000.0
    w1, w2 = rng.uniform(-0.2, 1.2, F).astype(f32), rng.uniform(-0.2, 1.2, F).astype(f32)
    w1[[0, 4, 9]], w2[[1, 4, 20]] = (0.0, 1.0, np.nan), (1.0, 0.0, 0.0)
    z1, z2 = (rng.random(F) < 0.5).astype(f32), (rng.random(F) < 0.5).astype(f32)
    z1[7] = np.nan
    return fr, size, C, {tm.BLUR: (length, None), tm.SMOOTH: (w1, w2), tm.FREEZE: (z1, z2)}


def _pieces(F, cut):
    edges = list(range(0, F, cut)) + [F]
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("max_frames", [1, 2, 7, 40])
def test_the_model_gives_the_same_bits_however_the_stream_is_cut(max_frames):
    fr, size, C, pq = _stream_inputs()
    for op in OPS:
        p, q = pq[op]
        whole = tm.Stream(C, size, SR, max_frames)
        want = whole.run(op, fr, p, q)
        for cut in CUTS:
            st = tm.Stream(C, size, SR, max_frames)
            got = np.concatenate([st.run(op, fr[:, a:b], p[a:b], None if q is None else q[a:b])
                                  for a, b in _pieces(F_ALL, cut)], axis=1)
            assert np.array_equal(bits(got), bits(want)), (op, cut)
            assert np.array_equal(bits(st.state(op)), bits(whole.state(op))), (op, cut)


def test_blur_of_one_frame_returns_the_inputs_bits():
    fr, size, C, _ = _stream_inputs(4)
    fr = fr.copy()
    fr[0, 2, 3, 0], fr[1, 5, 7, 1] = -0.0, np.inf
    for max_frames in (1, 7):
        for length in (1.0, 1.9, 0.0, -3.0, np.nan):
            out, hist = tm.blur32(fr, length, tm.empty(C, size, SR, max_frames - 1), max_frames)
            assert np.array_equal(bits(out), bits(fr)), (max_frames, length)
            assert np.array_equal(bits(hist), bits(fr[:, F_ALL - (max_frames - 1):])), max_frames
    # a window never reaches past max_frames, and the history before the stream is EMPTY
    out, _ = tm.blur32(fr, 1000.0, tm.empty(C, size, SR, 2), 3)
    e = tm.empty(C, size, SR)
    assert np.array_equal(out[:, 0], ((e + e) + fr[:, 0]) * f32(1.0 / 3))
    assert np.array_equal(out[:, 5], ((fr[:, 3] + fr[:, 4]) + fr[:, 5]) * f32(1.0 / 3))


def test_freeze_is_the_gather_of_the_last_unfrozen_frame():
    fr, size, C, pq = _stream_inputs(5)
    z1, z2 = pq[tm.FREEZE]
    start = tm.empty(C, size, SR)
    for a, b in ((z1, z2), (z2, z1), (np.ones(F_ALL, f32), np.zeros(F_ALL, f32)), (z1, z1)):
        out, held = tm.freeze32(fr, a, b, start)
        assert np.array_equal(bits(out), bits(tm.freeze_gather(fr, a, b, start)))
        assert np.array_equal(bits(held), bits(out[:, -1]))
    out, _ = tm.freeze32(fr, 1.0, 0.0, start)
    assert np.array_equal(bits(out[..., 0]), bits(np.broadcast_to(start[:, None, :, 0], out.shape[:3])))
    assert np.array_equal(bits(out[..., 1]), bits(fr[..., 1]))
    # a NaN in a frozen frame's input stays out
    bad = fr.copy()
    bad[:, 6] = np.nan
    flag = np.zeros(F_ALL, f32)
    flag[6] = 1
    out, _ = tm.freeze32(bad, flag, flag, start)
    assert not np.isnan(out).any() and np.array_equal(bits(out[:, 6]), bits(fr[:, 5]))


def test_smooth_with_weights_one_and_zero_copies_and_holds():
    fr, size, C, _ = _stream_inputs(6)
    y0 = tm.empty(C, size, SR)
    out, y = tm.smooth32(fr, 1.0, 7.0, y0)
    assert np.array_equal(bits(out), bits(fr)) and np.array_equal(bits(y), bits(fr[:, -1]))
    for w in (0.0, -1.0, np.nan):
        out, y = tm.smooth32(fr, w, w, y0)
        assert np.array_equal(bits(out), bits(np.broadcast_to(y0[:, None], fr.shape))) and np.array_equal(bits(y), bits(y0))
    # weight 1 after a NaN state returns the input's bits
    out, _ = tm.smooth32(fr, 1.0, 1.0, np.full_like(y0, np.nan))
    assert np.array_equal(bits(out), bits(fr))
    out, _ = tm.smooth32(fr, 0.25, 0.5, y0)
    assert np.array_equal(out[:, 0, :, 0], y0[..., 0] + f32(0.25) * (fr[:, 0, :, 0] - y0[..., 0]))
    assert np.array_equal(out[:, 1, :, 1], out[:, 0, :, 1] + f32(0.5) * (fr[:, 1, :, 1] - out[:, 0, :, 1]))


def test_float32_and_float64_models_agree():
    fr, size, C, pq = _stream_inputs(7)
    length = pq[tm.BLUR][0]
    o32, h32 = tm.blur32(fr, length, tm.empty(C, size, SR, 39), 40)
    o64, h64 = tm.blur64(fr, length, tm.empty(C, size, SR, 39), 40)
    assert om.rel_l2(o32, o64) < 1e-5 and np.array_equal(h32.astype(np.float64), h64)
    w1, w2 = pq[tm.SMOOTH]
    o32, y32 = tm.smooth32(fr, w1, w2, tm.empty(C, size, SR))
    o64, y64 = tm.smooth64(fr, w1, w2, tm.empty(C, size, SR))
    assert om.rel_l2(o32, o64) < 1e-5 and om.rel_l2(y32, y64) < 1e-5
    z1, z2 = pq[tm.FREEZE]
    o32, _ = tm.freeze32(fr, z1, z2, tm.empty(C, size, SR))
    o64, _ = tm.freeze64(fr, z1, z2, tm.empty(C, size, SR))
    assert np.array_equal(o32.astype(np.float64), o64)
