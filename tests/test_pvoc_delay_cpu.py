"""The per-bin delay with feedback of clfa_pvoc without a GPU: properties of the numpy model of its definition
(tests/pvoc_delay_model.py), all exact, and the library's new symbols and argument checks — which come before any device
lookup, so they answer on a machine without a device too."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_delay_model as dm
from tests.pvoc_time_model import empty

CL_INVALID_VALUE = -30
CL_INVALID_OPERATION = -59
SR = 48000.0
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frames(rng, C, F, size):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    fr = np.stack([amp, freq], axis=-1)
    fr[0, F // 2, 3] = (np.nan, 7.0)
    fr[C - 1, 1, 5] = (np.inf, np.nan)
    fr[0, 2, 6, 0] = -0.0
    return fr


def _tables(rng, B, L):
    d = rng.integers(0, L + 1, B).astype(np.int32)
    pool = [0, 1, L, 3, 7, 9, L + 5, -3]
    d[:len(pool)] = pool
    g = rng.uniform(-1, 1, B).astype(f32)
    pool = np.array([0.5, 0.0, -0.0, 1.0, -1.0, -0.7, 2.0 ** -20, np.nan, 1.5], f32)
    g[1:1 + pool.size] = pool
    return d, g


# ---- the model's own properties ----

@pytest.mark.parametrize("d,g", [(1, 0.5), (3, -0.7), (8, 1.0), (5, f32(2.0 ** -20)), (2, 0.3)])
def test_an_impulse_echoes_every_d_frames_with_the_powers_of_g(d, g):
    size, C, F, L, b = 64, 2, 41, 9, 11
    B = size // 2 + 1
    phi = f32(1234.5)
    fr = np.zeros((C, F, B, 2), f32)
    fr[..., 1] = empty(C, size, SR, F)[..., 1]
    fr[:, 0, b] = (1.0, phi)
    delays = np.zeros(B, np.int32)
    delays[b] = d
    st = dm.Stream(C, size, SR, L)
    out = st.run(fr, delays, np.full(B, g, f32))
    want_amp = np.zeros(F, f32)
    gk = f32(1.0)
    for k in range(F):
        if d * (k + 1) >= F:
            break
        want_amp[d * (k + 1)] = gk
        gk = f32(f32(g) * gk)
    for c in range(C):
        assert np.array_equal(bits(out[c, :, b, 0]), bits(want_amp)), c       # the echoes, and +0 everywhere else
        echoes = want_amp != 0
        assert np.array_equal(bits(out[c, echoes, b, 1]), bits(np.full(echoes.sum(), phi, f32)))
    # the other bins have d == 0: the input's bits
    other = np.arange(B) != b
    assert np.array_equal(bits(out[:, :, other]), bits(fr[:, :, other]))


def test_without_feedback_it_is_a_take_along_the_frames_of_the_padded_input():
    size, C, F, L = 64, 2, 23, 9
    rng = np.random.default_rng(2)
    fr = _frames(rng, C, F, size)
    d, _ = _tables(rng, size // 2 + 1, L)
    st = dm.Stream(C, size, SR, L)
    out = st.run(fr, d)
    padded = np.concatenate([empty(C, size, SR, L), fr], axis=1)
    dd = np.clip(d, 0, L)
    for b in range(size // 2 + 1):
        assert np.array_equal(bits(out[:, :, b]), bits(np.take(padded[:, :, b], L - dd[b] + np.arange(F), axis=1))), b
    assert np.array_equal(bits(out), bits(dm.delay_take(fr, d, empty(C, size, SR, L))))
    # the histories: the last L frames of the input and of the output
    assert np.array_equal(bits(st.xhist), bits(fr[:, F - L:])) and np.array_equal(bits(st.yhist), bits(out[:, F - L:]))
    # a second call reads the first one's frames
    out2 = st.run(fr[:, :4], d)
    both = np.concatenate([padded, fr[:, :4]], axis=1)
    for b in (0, 1, 2, 3, 20):
        assert np.array_equal(bits(out2[:, :, b]), bits(both[:, L + F - dd[b]:L + F - dd[b] + 4, b])), b


def test_a_delay_of_zero_returns_the_inputs_bits_with_any_feedback():
    size, C, F, L = 64, 2, 12, 5
    rng = np.random.default_rng(3)
    fr = _frames(rng, C, F, size)
    B = size // 2 + 1
    for g in (None, 0.0, 1.0, -0.7, np.nan, np.inf, 1.5):
        for d in (0, -4, np.zeros(B, np.int32)):
            st = dm.Stream(C, size, SR, L)
            assert np.array_equal(bits(st.run(fr, d, g)), bits(fr)), (g, d)
            assert np.array_equal(bits(st.yhist), bits(fr[:, F - L:]))
    st = dm.Stream(C, size, SR, 0)          # no history at all: every delay is 0
    assert np.array_equal(bits(st.run(fr, 7, 0.5)), bits(fr)) and st.xhist.shape == (C, 0, B, 2)


def test_the_rule_rounds_every_step_and_takes_the_louder_sides_freq():
    size, C, L = 64, 1, 2
    B = size // 2 + 1
    fr = np.zeros((C, 3, B, 2), f32)
    fr[0, 0, :, 0], fr[0, 0, :, 1] = 0.1, 100.0          # x[0]
    fr[0, 1, :, 0], fr[0, 1, :, 1] = 3.0, 200.0          # x[1]
    g = f32(0.3)
    out = dm.Stream(C, size, SR, L).run(fr, 1, np.full(B, g, f32))
    # frame 1: x[0] + g y[0], y[0] = x[-1] + g y[-1] = EMPTY (amp 0): the input is louder
    assert np.array_equal(bits(out[0, 1, :, 0]), bits(np.full(B, f32(0.1) + f32(g * f32(0.0)), f32)))
    assert (out[0, 1, :, 1] == 100.0).all()
    # frame 2: x[1] + g y[1] = 3 + 0.3 * 0.1
    assert np.array_equal(bits(out[0, 2, :, 0]), bits(np.full(B, f32(3.0) + f32(g * out[0, 1, 0, 0]), f32)))
    assert (out[0, 2, :, 1] == 200.0).all()
    # an echo louder than the delayed input brings its freq; a NaN on either side takes the input's freq
    yh = np.zeros((C, L, B, 2), f32)
    yh[0, 1, :, 0], yh[0, 1, :, 1] = 5.0, 777.0
    yh[0, 1, 4, 0] = np.nan
    xh = np.zeros((C, L, B, 2), f32)
    xh[0, 1, :, 0], xh[0, 1, :, 1] = 1.0, 55.0
    o, _, _ = dm.delay32(fr[:, :1], 1, np.full(B, -0.5, f32), xh, yh)
    assert np.array_equal(o[0, 0, :4, 0], np.full(4, f32(1.0) + f32(f32(-0.5) * f32(5.0)), f32)) and (o[0, 0, :4, 1] == 777.0).all()
    assert np.isnan(o[0, 0, 4, 0]) and o[0, 0, 4, 1] == 55.0


F_ALL = 37
CUTS = (1, 2, 5, F_ALL - 8)


@pytest.mark.parametrize("L", [0, 1, 6, 39])
def test_the_model_gives_the_same_bits_however_the_stream_is_cut(L):
    size, C = 64, 2
    rng = np.random.default_rng(4)
    fr = _frames(rng, C, F_ALL, size)
    d, g = _tables(rng, size // 2 + 1, L)
    for fb in (None, g):
        whole = dm.Stream(C, size, SR, L)
        want = whole.run(fr, d, fb)
        for cut in CUTS:
            st = dm.Stream(C, size, SR, L)
            edges = list(range(0, F_ALL, cut)) + [F_ALL]
            got = np.concatenate([st.run(fr[:, a:b], d, fb) for a, b in zip(edges[:-1], edges[1:])], axis=1)
            assert np.array_equal(bits(got), bits(want)), (fb is None, cut)
            for h, w in zip(st.state(), whole.state()):
                assert np.array_equal(bits(h), bits(w)), (fb is None, cut)
    # a call without feedback leaves both histories as a call with feedback wants them: yhist holds what it put out
    st = dm.Stream(C, size, SR, L)
    first = st.run(fr[:, :20], d)
    assert np.array_equal(bits(st.yhist), bits(np.concatenate([empty(C, size, SR, L), first], axis=1)[:, 20:]))
    assert np.array_equal(bits(st.xhist), bits(np.concatenate([empty(C, size, SR, L), fr[:, :20]], axis=1)[:, 20:]))


def test_delay_frames_is_the_nearest_whole_number_of_frames():
    assert fa.Pvoc.delay_frames(0.5, 48000.0, 512) == 47          # 46.875
    assert fa.Pvoc.delay_frames(0.0, 48000.0, 512) == 0
    assert fa.Pvoc.delay_frames(1.0, 48000.0, 256) == 188         # 187.5 rounds to the even neighbour
    assert fa.Pvoc.delay_frames(0.004, 44100.0, 128) == 1         # 1.378
    assert isinstance(fa.Pvoc.delay_frames(0.1, 48000.0, 512), int)


# ---- the library without a device ----

NAMES = ["clfa_pvoc_delay_setup", "clfa_pvoc_delay_dev", "clfa_pvoc_delay", "clfa_pvoc_delay_read_state",
         "clfa_pvoc_delay_state_bytes", "clfa_pvoc_delay_max_frames", "clfa_pvoc_delay_kernel_name"]


def test_library_exports_the_delay_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in NAMES:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.delay_kernel_name() == "" and bad.delay_kernel_name(True) == ""
    assert bad.delay_max_frames() == -1 and bad.delay_setup(4) == CL_INVALID_VALUE and bad.delay_state_bytes() == 0
    pv = fa.Pvoc(0, 64, 16, SR)
    if pv.get_error() == 0:
        assert [pv.delay_kernel_name(f) for f in (False, True)] == ["k_pvoc_delay", "k_pvoc_delay_fb"]
    else:
        assert pv.delay_kernel_name() == "" and pv.delay_kernel_name(True) == ""
    assert pv.delay_max_frames() == -1 and pv.delay_state_bytes() == 0
    for m in ("delay", "delay_device", "delay_setup", "delay_max_frames", "delay_state", "delay_state_bytes",
              "delay_kernel_name", "delay_frames"):
        assert callable(getattr(pv, m)), m


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    B = size // 2 + 1
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    rng = np.random.default_rng(5)
    a = _frames(rng, C, F, size)
    out = np.full_like(a, 7.0)
    delays, gains = np.full(B, 2, np.int32), np.full(B, 0.5, f32)
    ptr = lambda x: None if x is None else x.ctypes.data

    def host(a=a, o=out, F=F, d=delays, g=gains, h=pv._h):
        return L.clfa_pvoc_delay(h, ptr(a), ptr(o), F, ptr(d), ptr(g))

    def devf(a=a, o=out, F=F, d=delays, g=gains):          # the device form's checks, on host addresses
        return L.clfa_pvoc_delay_dev(pv._h, ptr(a), ptr(o), F, ptr(d), ptr(g), None)

    def bad_arguments():
        """every argument error, whatever the setup's state"""
        for f in (host, devf):
            assert f(F=-1) == CL_INVALID_VALUE
            for name in ("a", "o", "d"):
                assert f(**{name: None}) == CL_INVALID_VALUE, name
            # an output overlapping the input by one element, or being it
            both = np.zeros(2 * a.size, f32)
            lo, hi = both[:a.size].reshape(a.shape), both[a.size - 1:2 * a.size - 1].reshape(a.shape)
            lo[...] = a
            assert f(a=lo, o=hi) == CL_INVALID_VALUE and f(a=hi, o=lo) == CL_INVALID_VALUE and f(a=a, o=a) == CL_INVALID_VALUE
            # an output overlapping a table by one element
            buf = np.zeros(a.size + B, f32)
            o2, tail = buf[:a.size].reshape(a.shape), buf[a.size - 1:a.size - 1 + B]
            assert f(o=o2, g=tail) == CL_INVALID_VALUE and f(o=o2, d=tail.view(np.int32)) == CL_INVALID_VALUE
        # misaligned tables and frames: the device form alone looks at the alignment
        def off_by(nbytes, dtype, align, by):
            raw = np.zeros(nbytes + 2 * align, np.uint8)
            lo = (by - raw.ctypes.data) % align
            return raw[lo:lo + nbytes].view(dtype)

        assert devf(d=off_by(4 * B, np.int32, 4, 1)) == CL_INVALID_VALUE
        assert devf(g=off_by(4 * B, f32, 4, 2)) == CL_INVALID_VALUE
        assert devf(a=off_by(a.nbytes, f32, 8, 4).reshape(a.shape)) == CL_INVALID_VALUE
        assert devf(o=off_by(a.nbytes, f32, 8, 4).reshape(a.shape)) == CL_INVALID_VALUE
        # the blocking form checks the tables' values
        for bad_d in (-1, 4097, np.iinfo(np.int32).min):
            d = delays.copy()
            d[B - 1] = bad_d
            assert host(d=d) == CL_INVALID_VALUE, bad_d
        for bad_g in (1.5, -1.0000001, np.nan, np.inf, -np.inf):
            g = gains.copy()
            g[B // 2] = bad_g
            assert host(g=g) == CL_INVALID_VALUE, bad_g
        assert L.clfa_pvoc_delay(None, ptr(a), ptr(out), F, ptr(delays), ptr(gains)) == CL_INVALID_VALUE
        assert L.clfa_pvoc_delay_dev(None, ptr(a), ptr(out), F, ptr(delays), ptr(gains), None) == CL_INVALID_VALUE

    # before the setup: every argument error first, then CL_INVALID_OPERATION, with or without a device
    assert pv.delay_max_frames() == -1
    bad_arguments()
    assert host() == CL_INVALID_OPERATION and devf() == CL_INVALID_OPERATION
    assert host(g=None) == CL_INVALID_OPERATION and devf(g=None) == CL_INVALID_OPERATION
    assert host(F=0) == good and devf(F=0) == good                 # nothing to do: no history needed
    with pytest.raises(fa.ClError) as e:
        pv.delay_state()
    assert e.value.code == (CL_INVALID_OPERATION if good == 0 else good)
    assert (out == 7.0).all()
    # the setup's range, before the device lookup
    for bad_max in (-1, 4097, -4096):
        assert pv.delay_setup(bad_max) == CL_INVALID_VALUE and L.clfa_pvoc_delay_setup(pv._h, bad_max) == CL_INVALID_VALUE
    assert L.clfa_pvoc_delay_setup(None, 4) == CL_INVALID_VALUE
    assert pv.delay_max_frames() == -1
    assert L.clfa_pvoc_delay_read_state(pv._h, 2, ptr(out)) == CL_INVALID_VALUE
    assert L.clfa_pvoc_delay_read_state(pv._h, -1, ptr(out)) == CL_INVALID_VALUE
    assert L.clfa_pvoc_delay_read_state(pv._h, 0, None) == CL_INVALID_VALUE
    assert L.clfa_pvoc_delay_read_state(None, 0, ptr(out)) == CL_INVALID_VALUE
    assert L.clfa_pvoc_delay_max_frames(None) == -1 and L.clfa_pvoc_delay_state_bytes(None) == 0
    # a good setup returns the object's error; with a device the calls then go through
    assert pv.delay_setup(0) == good and pv.delay_setup(4096 if good == 0 else 4) == good and pv.delay_setup(4) == good
    assert pv.delay_max_frames() == (4 if good == 0 else -1)
    assert pv.delay_state_bytes() == (3 * C * 4 * B * 8 if good == 0 else 0)
    if good == 0:
        bad_arguments()
        d5 = delays.copy()
        d5[0] = 5                                                  # above max_delay: the blocking form alone refuses it
        assert host(d=d5) == CL_INVALID_VALUE
        assert host() == 0 and host(g=None) == 0 and host(F=0) == 0
        assert host(d=np.array([0, 4] * B, np.int32)[:B], g=np.array([1.0, -1.0, 0.0] * B, f32)[:B]) == 0
    else:
        assert host() == CL_INVALID_OPERATION                      # without a device the delay cannot be set up
        assert (out == 7.0).all()                                  # nothing was computed anywhere
    # an object whose creation arguments were bad keeps answering with that error
    assert host(h=fa.Pvoc(0, 48, 16, SR)._h) == CL_INVALID_VALUE
    # the Python forms: the status raised as ClError, the shapes as ValueError
    for call, code in ((lambda: pv.delay(a, -1), CL_INVALID_VALUE), (lambda: pv.delay(a, 1, 1.5), CL_INVALID_VALUE),
                       (lambda: pv.delay(a, 1, np.nan), CL_INVALID_VALUE),
                       (lambda: pv.delay(a, 9), CL_INVALID_VALUE if good == 0 else CL_INVALID_OPERATION)):
        with pytest.raises(fa.ClError) as e:
            call()
        assert e.value.code == code
    with pytest.raises(ValueError):
        pv.delay(a[:, :, :5], 1)
    with pytest.raises(ValueError):
        pv.delay(a, np.zeros(B - 1, np.int32))
