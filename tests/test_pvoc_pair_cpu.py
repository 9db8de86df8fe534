"""The two-input frame operations of clfa_pvoc (cross, morph, filter, mix, vocode) without a GPU: the library's new
symbols and argument checks — which come before any device lookup, so they answer on a machine without a device too —
and identities of the numpy model of their definitions (tests/pvoc_pair_model.py)."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_ops_model as om
from tests import pvoc_pair_model as pp

CL_INVALID_VALUE = -30
SR = 48000.0
f32 = np.float32


def _frames(rng, C, F, size):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    return np.stack([amp, freq], axis=-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_pair_symbols():
    names = ["clfa_pvoc_pair_dev", "clfa_pvoc_pair", "clfa_pvoc_pair_kernel_name"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.pair_kernel_name("cross") == "" and bad.pair_kernel_name(4) == ""
    pv = fa.Pvoc(0, 64, 16, SR)
    if pv.get_error() == 0:
        assert [pv.pair_kernel_name(op) for op in ("cross", "morph", "filter", "mix", "vocode", "nothing", 5, -1)] == \
            ["k_pvoc_pair"] * 4 + ["k_pvoc_vocode", "", "", ""]
    for m in ("cross", "morph", "filter", "mix", "vocode"):
        assert callable(getattr(pv, m)) and callable(getattr(pv, m + "_device"))


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    rng = np.random.default_rng(5)
    a, b = _frames(rng, C, F, size), _frames(rng, C, F, size)
    out = np.full_like(a, 7.0)
    par, par2 = np.full(F, 0.5, f32), np.full(F, 0.25, f32)
    ptr = lambda x: None if x is None else x.ctypes.data

    def host(op, a=a, b=b, o=out, F=F, p=par, q=par2, coefs=10, h=pv._h):
        return L.clfa_pvoc_pair(h, op, ptr(a), ptr(b), ptr(o), F, ptr(p), ptr(q), coefs)

    def devf(op, a=a, b=b, o=out, F=F, p=par, q=par2, coefs=10):      # the device form's checks, on host addresses
        return L.clfa_pvoc_pair_dev(pv._h, op, ptr(a), ptr(b), ptr(o), F, ptr(p), ptr(q), coefs, None)

    for op in range(5):
        assert host(op) == good, op
        assert host(op, F=0) == good
        assert host(op, F=-1) == CL_INVALID_VALUE and devf(op, F=-1) == CL_INVALID_VALUE
        for name in ("a", "b", "o"):
            assert host(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
            assert devf(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
        # an output overlapping a or b by one element, or being one of them
        both = np.zeros(2 * a.size, f32)
        lo, hi = both[:a.size].reshape(a.shape), both[a.size - 1:2 * a.size - 1].reshape(a.shape)
        assert host(op, a=lo, o=hi) == CL_INVALID_VALUE and host(op, b=hi, o=lo) == CL_INVALID_VALUE
        assert devf(op, b=lo, o=hi) == CL_INVALID_VALUE
        assert host(op, a=a, o=a) == CL_INVALID_VALUE and host(op, b=b, o=b) == CL_INVALID_VALUE
        # the two inputs may be the same array; p and q may be the same array
        assert host(op, a=a, b=a) == good and host(op, p=par, q=par) == good
    for bad_op in (-1, 5, 99):
        assert host(bad_op) == CL_INVALID_VALUE and devf(bad_op) == CL_INVALID_VALUE
    # the per-frame arrays: NULL only for MIX; an output that overlaps one by one element
    assert host(pp.CROSS, p=None) == CL_INVALID_VALUE and devf(pp.CROSS, p=None) == CL_INVALID_VALUE
    buf = np.zeros(a.size + F, f32)
    o2, tail = buf[:a.size].reshape(a.shape), buf[a.size - 1:a.size - 1 + F]
    for op in (pp.CROSS, pp.MORPH, pp.FILTER, pp.VOCODE):
        assert host(op, q=None) == CL_INVALID_VALUE and host(op, p=None, q=None) == CL_INVALID_VALUE
        assert host(op, o=o2, p=tail) == CL_INVALID_VALUE and host(op, o=o2, q=tail) == CL_INVALID_VALUE
        assert devf(op, o=o2, p=tail) == CL_INVALID_VALUE and devf(op, o=o2, q=tail) == CL_INVALID_VALUE
        assert host(op, o=o2, p=buf[a.size:], q=buf[a.size:]) == good
    assert host(pp.MIX, p=None, q=None) == good and devf(pp.MIX, p=None, q=None, F=0) == good
    # coefs: VOCODE only
    assert host(pp.VOCODE, coefs=0) == CL_INVALID_VALUE and host(pp.VOCODE, coefs=M) == CL_INVALID_VALUE
    assert devf(pp.VOCODE, coefs=0) == CL_INVALID_VALUE and devf(pp.VOCODE, coefs=M) == CL_INVALID_VALUE
    assert host(pp.VOCODE, coefs=M - 1) == good and host(pp.VOCODE, coefs=1) == good and host(pp.CROSS, coefs=0) == good
    # the blocking form checks the values
    nan_gain, wide = np.array([1.0, np.nan, 1.0], f32), np.array([0.0, 1.5, 1.0], f32)
    for op in (pp.CROSS, pp.FILTER, pp.VOCODE):
        assert host(op, q=nan_gain) == CL_INVALID_VALUE, op
    assert host(pp.CROSS, p=np.array([np.inf, 0, 0], f32)) == CL_INVALID_VALUE
    assert host(pp.MORPH, p=wide) == CL_INVALID_VALUE and host(pp.MORPH, q=wide) == CL_INVALID_VALUE
    assert host(pp.MORPH, q=-wide) == CL_INVALID_VALUE
    assert host(pp.FILTER, p=wide) == CL_INVALID_VALUE and host(pp.VOCODE, p=wide) == CL_INVALID_VALUE
    assert host(pp.FILTER, q=wide) == good and host(pp.CROSS, p=-wide, q=wide) == good     # gains are free
    assert host(pp.MIX, p=nan_gain, q=wide) == good                                        # MIX reads neither
    assert L.clfa_pvoc_pair(None, 0, ptr(a), ptr(b), ptr(out), F, ptr(par), ptr(par2), 10) == CL_INVALID_VALUE
    if good != 0:
        assert (out == 7.0).all()          # nothing was computed anywhere
    # an object whose creation arguments were bad keeps answering with that error
    assert host(pp.CROSS, h=fa.Pvoc(0, 48, 16, SR)._h) == CL_INVALID_VALUE
    # the Python forms: plain numbers for the per-frame arrays; the status raised as ClError
    if good != 0:
        with pytest.raises(fa.ClError):
            pv.cross(a, b)
    for call in (lambda: pv.morph(a, b, amp=1.5), lambda: pv.morph(a, b, freq=-0.1), lambda: pv.filter(a, b, depth=2.0),
                 lambda: pv.vocode(a, b, depth=1.5, coefs=10), lambda: pv.vocode(a, b, coefs=M), lambda: pv.cross(a, b, np.nan)):
        with pytest.raises(fa.ClError) as e:
            call()
        assert e.value.code == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        pv.mix(a, b[:, :2])


def _pair_of_frames(seed=7, size=64, C=2, F=4):
    rng = np.random.default_rng(seed)
    return _frames(rng, C, F, size), _frames(rng, C, F, size), size


def test_morph_at_the_ends_returns_the_bits_of_one_side():
    a, b, size = _pair_of_frames()
    na, nb = a.copy(), b.copy()
    na[0, 1, 3], nb[1, 2, 5] = np.nan, (np.nan, np.inf)
    # weights 0: a, whatever b holds; weights 1 (and above, clamped): b, whatever a holds; a NaN weight is 0
    for w in (0.0, -3.0, np.nan):
        assert np.array_equal(bits(pp.pair32(pp.MORPH, a, nb, w, w, size, SR)), bits(a)), w
    for w in (1.0, 7.0):
        assert np.array_equal(bits(pp.pair32(pp.MORPH, na, b, w, w, size, SR)), bits(b)), w
    # per column: amps of a with the freqs of b, frame by frame
    wa, wf = np.array([0, 1, 0, 1], f32), np.array([1, 0, 0, 1], f32)
    out = pp.pair32(pp.MORPH, a, b, wa, wf, size, SR)
    for f in range(4):
        assert np.array_equal(bits(out[:, f, :, 0]), bits((b if wa[f] else a)[:, f, :, 0]))
        assert np.array_equal(bits(out[:, f, :, 1]), bits((b if wf[f] else a)[:, f, :, 1]))
    mid = pp.pair32(pp.MORPH, a, b, 0.5, 0.25, size, SR)
    assert np.array_equal(mid[..., 0], a[..., 0] + f32(0.5) * (b[..., 0] - a[..., 0]))
    assert np.array_equal(mid[..., 1], a[..., 1] + f32(0.25) * (b[..., 1] - a[..., 1]))


def test_cross_filter_and_mix_identities():
    a, b, size = _pair_of_frames(8)
    assert np.array_equal(bits(pp.pair32(pp.CROSS, a, b, 1.0, 0.0, size, SR)), bits(a))
    sw = pp.pair32(pp.CROSS, a, b, 0.0, 1.0, size, SR)
    assert np.array_equal(bits(sw[..., 0]), bits(b[..., 0])) and np.array_equal(bits(sw[..., 1]), bits(a[..., 1]))
    # a filter of depth 0 and gain 1 is a, whatever b holds
    nb = b.copy()
    nb[0, 0, 2, 0] = np.nan
    assert np.array_equal(bits(pp.pair32(pp.FILTER, a, nb, 0.0, 1.0, size, SR)), bits(a))
    full = pp.pair32(pp.FILTER, a, b, 1.0, 2.0, size, SR)
    assert np.array_equal(full[..., 0], f32(2) * (a[..., 0] * (f32(0) + b[..., 0])))
    # mix: idempotent, a on ties and on NaNs of either side
    m = pp.pair32(pp.MIX, a, b, None, None, size, SR)
    assert np.array_equal(bits(pp.pair32(pp.MIX, m, b, None, None, size, SR)), bits(m))
    assert np.array_equal(bits(pp.pair32(pp.MIX, a, m, None, None, size, SR)), bits(m))
    assert np.array_equal(m[..., 0], np.maximum(a[..., 0], b[..., 0]))
    tie = b.copy()
    tie[..., 0] = a[..., 0]
    assert np.array_equal(bits(pp.pair32(pp.MIX, a, tie, None, None, size, SR)), bits(a))
    na, nb = a.copy(), b.copy()
    na[1, 1, 4, 0] = nb[0, 2, 6, 0] = np.nan
    nb[0, 2, 6, 1] = 123.0
    m = pp.pair32(pp.MIX, na, nb, None, None, size, SR)
    assert np.array_equal(bits(m[1, 1, 4]), bits(na[1, 1, 4])) and np.array_equal(bits(m[0, 2, 6]), bits(a[0, 2, 6]))


@pytest.mark.parametrize("size,coefs", [(64, 1), (64, 31), (256, 24)])
def test_vocode_of_a_frame_with_itself_returns_its_amps(size, coefs):
    a, _, _ = _pair_of_frames(9, size)
    out = pp.pair32(pp.VOCODE, a, a, 1.0, 1.0, size, SR, coefs)
    assert np.array_equal(bits(out[..., 1]), bits(a[..., 1]))
    assert om.rel_l2(out[..., 0], a[..., 0]) <= 1e-5
    assert om.rel_l2(pp.vocode64_amps(a, a, 1.0, 1.0, size, SR, coefs), a[..., 0]) <= 1e-12


def test_vocode_models_agree_and_depth_zero_is_the_excitation():
    a, b, size = _pair_of_frames(10, 256)
    d = np.array([1.0, 0.6, 0.0, 0.3], f32)
    g = np.array([1.0, -0.5, 2.0, 1.0], f32)
    m32, m64 = pp.pair32(pp.VOCODE, a, b, d, g, size, SR, 20), pp.vocode64_amps(a, b, d, g, size, SR, 20)
    assert np.isfinite(m32).all() and np.isfinite(m64).all()
    assert om.rel_l2(m32[..., 0], m64) < 1e-5
    assert np.allclose(m64[:, 2], 2.0 * b[:, 2, :, 0].astype(np.float64), rtol=1e-12)
    # the formants of a: with depth 1 the envelope of the output is the envelope of a (the lifter is a linear projection)
    ea, eo = om.env64(a[..., 0], 20)[:, 0], om.env64(m64[:, :1], 20)[:, 0]
    assert np.abs(np.log(eo / ea)).max() < 1e-9
