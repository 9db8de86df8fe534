"""The one-stream shaping operations of clfa_pvoc (band, mask, stencil, arp, lock, warp) without a GPU: the library's new
symbols and argument checks — which come before any device lookup, so they answer on a machine without a device too —
and identities of the numpy model of their definitions (tests/pvoc_shape_model.py)."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_ops_model as om
from tests import pvoc_shape_model as sm

CL_INVALID_VALUE = -30
SR = 48000.0
f32 = np.float32
NAMES = ("band", "mask", "stencil", "arp", "lock", "warp")


def _frames(rng, C, F, size):
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    return np.stack([amp, freq], axis=-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_shape_symbols():
    names = ["clfa_pvoc_shape_dev", "clfa_pvoc_shape", "clfa_pvoc_shape_kernel_name"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.shape_kernel_name("band") == "" and bad.shape_kernel_name(5) == ""
    pv = fa.Pvoc(0, 64, 16, SR)
    if pv.get_error() == 0:
        assert [pv.shape_kernel_name(op) for op in NAMES + (0, 3, 4, 5, "nothing", 6, -1)] == \
            ["k_pvoc_shape"] * 4 + ["k_pvoc_lock", "k_pvoc_warp", "k_pvoc_shape", "k_pvoc_shape", "k_pvoc_lock",
                                    "k_pvoc_warp", "", "", ""]
    else:
        assert [pv.shape_kernel_name(op) for op in NAMES + ("nothing", 6, -1)] == [""] * 9
    for m in NAMES:
        assert callable(getattr(pv, m)) and callable(getattr(pv, m + "_device"))


# rows the blocking form accepts, per op
GOOD = {sm.BAND: (100.0, 200.0, 3000.0, 4000.0), sm.MASK: (0.5,), sm.STENCIL: (0.5, 1.0), sm.ARP: (0.3, 0.9, 2.0),
        sm.LOCK: (1.0, 0.01), sm.WARP: (1.5, 100.0, 1.0)}


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    rng = np.random.default_rng(5)
    a = _frames(rng, C, F, size)
    out = np.full_like(a, 7.0)
    table = np.linspace(0, 1, M + 1).astype(f32)
    ptr = lambda x: None if x is None else x.ctypes.data
    default = object()

    def host(op, a=a, o=out, F=F, par=default, t=table, flags=0, lowest=1, coefs=10, h=pv._h):
        par = sm.rows(3, *GOOD[op]) if par is default else par
        return L.clfa_pvoc_shape(h, op, ptr(a), ptr(o), F, ptr(par), ptr(t), flags, lowest, coefs)

    def devf(op, a=a, o=out, F=F, par=default, t=table, flags=0, lowest=1, coefs=10):   # the device form's checks, on host addresses
        par = sm.rows(3, *GOOD[op]) if par is default else par
        return L.clfa_pvoc_shape_dev(pv._h, op, ptr(a), ptr(o), F, ptr(par), ptr(t), flags, lowest, coefs, None)

    for op in range(6):
        assert host(op) == good, op
        assert host(op, F=0) == good and devf(op, F=0) == good      # the device form on host addresses: never a good call
        assert host(op, F=-1) == CL_INVALID_VALUE and devf(op, F=-1) == CL_INVALID_VALUE
        for name in ("a", "o", "par"):
            assert host(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
            assert devf(op, **{name: None}) == CL_INVALID_VALUE, (op, name)
        # the table: needed by MASK and STENCIL, not looked at by the others
        needs = op in (sm.MASK, sm.STENCIL)
        assert host(op, t=None) == (CL_INVALID_VALUE if needs else good), op
        assert not needs or devf(op, t=None) == CL_INVALID_VALUE, op
        assert devf(op, t=None, F=0) == good
        # flags: bit 0 for BAND alone, no other bit
        assert host(op, flags=1) == (good if op == sm.BAND else CL_INVALID_VALUE), op
        assert op == sm.BAND or devf(op, flags=1) == CL_INVALID_VALUE, op
        assert devf(sm.BAND, flags=1, F=0) == good
        for flags in (2, 3, 4, -1, 1 << 16):
            assert host(op, flags=flags) == CL_INVALID_VALUE and devf(op, flags=flags) == CL_INVALID_VALUE, (op, flags)
        # an output overlapping the input by one element, or being the input
        both = np.zeros(2 * a.size, f32)
        lo, hi = both[:a.size].reshape(a.shape), both[a.size - 1:2 * a.size - 1].reshape(a.shape)
        assert host(op, a=lo, o=hi) == CL_INVALID_VALUE and host(op, a=hi, o=lo) == CL_INVALID_VALUE
        assert devf(op, a=lo, o=hi) == CL_INVALID_VALUE and devf(op, a=hi, o=lo) == CL_INVALID_VALUE
        assert host(op, a=a, o=a) == CL_INVALID_VALUE and devf(op, a=a, o=a) == CL_INVALID_VALUE
        # an output overlapping par by one element, on either side
        buf = np.zeros(4 * F + a.size + 4 * F, f32)
        buf[:4 * F] = buf[-4 * F:] = sm.rows(F, *GOOD[op]).ravel()
        o2 = buf[4 * F:4 * F + a.size].reshape(a.shape)
        before, after = buf[1:4 * F + 1].reshape(F, 4), buf[4 * F + a.size - 1:-1].reshape(F, 4)
        for par in (before, after):
            assert host(op, o=o2, par=par) == CL_INVALID_VALUE and devf(op, o=o2, par=par) == CL_INVALID_VALUE, op
        assert host(op, o=o2, par=buf[:4 * F].reshape(F, 4)) == good and host(op, o=o2, par=buf[-4 * F:].reshape(F, 4)) == good
        # an output overlapping the table by one element: MASK and STENCIL; the others do not look at it
        tb = np.zeros(M + 1 + a.size, f32)
        o3, t3 = tb[M + 1:].reshape(a.shape), tb[1:M + 2]
        assert host(op, o=o3, t=t3) == (CL_INVALID_VALUE if needs else good), op
        assert not needs or devf(op, o=o3, t=t3) == CL_INVALID_VALUE, op
        assert host(op, o=o3, t=tb[:M + 1]) == good
    for bad_op in (-1, 6, 99):
        for call in (host, devf):
            assert call(bad_op, par=sm.rows(3, 0.5)) == CL_INVALID_VALUE
    # lowest_bin and coefs: WARP only
    for call in (host, devf):
        for kw in ({"lowest": 0}, {"lowest": M}, {"lowest": -2}, {"coefs": 0}, {"coefs": M}, {"coefs": -1}):
            assert call(sm.WARP, **kw) == CL_INVALID_VALUE, kw
            assert call(sm.WARP, F=0, **kw) == CL_INVALID_VALUE, kw
    assert host(sm.WARP, lowest=M - 1, coefs=M - 1) == good and host(sm.WARP, lowest=1, coefs=1) == good
    assert devf(sm.WARP, lowest=M - 1, coefs=M - 1, F=0) == good
    for op in range(5):
        assert host(op, lowest=0, coefs=0) == good and host(op, lowest=M, coefs=M) == good
        assert devf(op, lowest=0, coefs=M, F=0) == good
    # the blocking form checks the values the op names: finite ...
    for op in range(6):
        for col in range(4):
            for bad in (np.nan, np.inf, -np.inf):
                r = sm.rows(3, *GOOD[op])
                r[1, col] = bad
                assert host(op, par=r) == (CL_INVALID_VALUE if col < sm.COLS[op] else good), (op, col, bad)
    # ... BAND: 0 <= lc <= lf <= hf <= hc
    for row in ((-1, 200, 3000, 4000), (300, 200, 3000, 4000), (100, 3500, 3000, 4000), (100, 200, 5000, 4000)):
        assert host(sm.BAND, par=sm.rows(3, *row)) == CL_INVALID_VALUE, row
    for row in ((0, 0, 0, 0), (100, 100, 3000, 3000), (0, 200, 200, 1e9)):
        assert host(sm.BAND, par=sm.rows(3, *row)) == good and host(sm.BAND, par=sm.rows(3, *row), flags=1) == good, row
    # ... depths and pos in [0, 1]
    for v in (-0.25, 1.5):
        assert host(sm.MASK, par=sm.rows(3, v)) == CL_INVALID_VALUE
        assert host(sm.ARP, par=sm.rows(3, v, 0.5, 1.0)) == CL_INVALID_VALUE
        assert host(sm.ARP, par=sm.rows(3, 0.5, v, 1.0)) == CL_INVALID_VALUE
    for v in (0.0, 1.0):
        assert host(sm.MASK, par=sm.rows(3, v)) == good and host(sm.ARP, par=sm.rows(3, v, v, -7.0)) == good
    assert host(sm.STENCIL, par=sm.rows(3, -3.0, 1e20)) == good                    # gains and levels are free
    # ... tol >= 0
    assert host(sm.LOCK, par=sm.rows(3, 1.0, -0.01)) == CL_INVALID_VALUE
    assert host(sm.LOCK, par=sm.rows(3, -5.0, 0.0)) == good
    # ... s in [0.25, 4]
    for s in (0.2, 4.5, -1.0, 0.0):
        assert host(sm.WARP, par=sm.rows(3, s, 0.0, 1.0)) == CL_INVALID_VALUE, s
    assert host(sm.WARP, par=sm.rows(3, np.array([0.25, 4.0, 1.0], f32), -1e6, -2.0)) == good
    assert L.clfa_pvoc_shape(None, 0, ptr(a), ptr(out), F, ptr(sm.rows(3, *GOOD[0])), None, 0, 1, 1) == CL_INVALID_VALUE
    if good != 0:
        assert (out == 7.0).all()          # nothing was computed anywhere
    # an object whose creation arguments were bad keeps answering with that error
    assert host(sm.BAND, h=fa.Pvoc(0, 48, 16, SR)._h) == CL_INVALID_VALUE
    # the Python forms: plain numbers for the per-frame values; the status raised as ClError
    if good != 0:
        with pytest.raises(fa.ClError):
            pv.lock(a)
    for call in (lambda: pv.band(a, 300, 200, 3000, 4000), lambda: pv.mask(a, table, 1.5), lambda: pv.arp(a, -0.1),
                 lambda: pv.stencil(a, table, np.nan), lambda: pv.lock(a, tol=-1.0), lambda: pv.warp(a, 5.0, coefs=10),
                 lambda: pv.warp(a, 1.0, coefs=M), lambda: pv.warp(a, 1.0, lowest_bin=0, coefs=10)):
        with pytest.raises(fa.ClError) as e:
            call()
        assert e.value.code == CL_INVALID_VALUE
    with pytest.raises(ValueError):
        pv.mask(a, table[:-1])
    with pytest.raises(ValueError):
        pv.lock(a[:, :, :-1])


def _serial_lock(frame, tol):
    """one locked frame (M + 1, 2) by the definition: a loop over the peaks in ascending order, each handing its freq to
    the bin below and the bin above it where theirs lies within tol of it; written on its own, not from the gather.
    Returns (the frame, how often each bin was reached)"""
    B = frame.shape[0]
    M = B - 1
    amp, freq = frame[:, 0], frame[:, 1]
    out = frame.copy()
    reached = np.zeros(B, np.int64)
    with np.errstate(all="ignore"):
        for c in range(2, M - 1):
            if not all(amp[c] > amp[c + o] for o in (-2, -1, 1, 2)):
                continue
            d = f32(f32(tol) * np.abs(freq[c]))
            for nb in (c - 1, c + 1):
                reached[nb] += 1
                if np.abs(f32(freq[nb] - freq[c])) < d:
                    out.view(np.uint32)[nb, 1] = frame.view(np.uint32)[c, 1]
    return out, reached


@pytest.mark.parametrize("M", [32, 256])
def test_the_locks_gather_is_the_serial_loop_over_the_peaks(M):
    size, C, F = 2 * M, 2, 6
    rng = np.random.default_rng(M)
    fr = _frames(rng, C, F, size)
    fr[..., 0] = rng.integers(0, 6, (C, F, M + 1)).astype(f32)      # few levels: ties everywhere
    fr[1, :3, :, 0] = np.abs(rng.standard_normal((3, M + 1))).astype(f32)
    fr[..., 0][rng.random((C, F, M + 1)) < 0.05] = np.nan
    fr[0, 0, :5, 0], fr[0, 0, M - 4:, 0] = (1, 2, 50, 2, 1), (1, 2, 60, 2, 1)   # the first and the last bin that can be a peak
    fr[0, 1, 1, 0], fr[0, 1, M - 1, 0] = 50.0, 60.0                   # and the ones beside them, which cannot
    tol = np.array([0.01, 0.5, 0.0, 10.0, 0.3, 1e-3], f32)
    lock = np.array([1.0, -2.0, 1.0, np.nan, 0.0, 1.0], f32)
    got = sm.lock_gather(fr, lock, tol)
    moved = peaks_seen = 0
    for c in range(C):
        for f in range(F):
            want, reached = _serial_lock(fr[c, f], tol[f])
            assert reached.max() <= 1, "a bin next to two peaks"
            peaks_seen += int(reached.sum()) // 2
            if lock[f] == 0:
                want = fr[c, f]
            assert np.array_equal(bits(got[c, f]), bits(want)), (c, f)
            moved += int((bits(want[:, 1]) != bits(fr[c, f, :, 1])).sum())
    assert np.array_equal(bits(got[..., 0]), bits(fr[..., 0]))
    assert np.array_equal(bits(got[:, 4]), bits(fr[:, 4])) and np.array_equal(bits(got[:, 2]), bits(fr[:, 2]))   # lock 0; tol 0
    assert sm.peaks(fr[0, 0, :, 0])[2] and sm.peaks(fr[0, 0, :, 0])[M - 2] and not sm.peaks(fr[0, 1, :, 0])[[1, M - 1]].any()
    assert peaks_seen >= 10 and moved >= 10, (peaks_seen, moved)
    # the count again, over all frames at once: no bin has a peak on both sides
    pk = sm.peaks(fr[..., 0])
    assert int((pk[..., 2:] & pk[..., :-2]).sum()) == 0 and int((pk[..., 1:] & pk[..., :-1]).sum()) == 0
    assert int(pk.sum()) == peaks_seen


def test_band_mask_arp_and_stencil_identities():
    size, C, F = 64, 2, 4
    M = size // 2
    rng = np.random.default_rng(3)
    a = _frames(rng, C, F, size)
    a[0, 1, 5, 0] = np.nan
    a[1, 2, 7, 1] = -a[1, 2, 7, 1]
    big = 3e38
    # wide open: the input's bits; with reject: +0 everywhere, the NaN amp included
    got = sm.shape32(sm.BAND, a, sm.rows(F, 0, 0, big, big), size, SR)
    assert np.array_equal(bits(got), bits(a))
    got = sm.shape32(sm.BAND, a, sm.rows(F, 0, 0, big, big), size, SR, reject=True)
    assert np.array_equal(bits(got[..., 1]), bits(a[..., 1])) and (bits(got[..., 0]) == 0).all()
    # a NaN freq lies in no band: +0, or with reject the bits
    n = a.copy()
    n[0, 0, 3, 1] = np.nan
    assert bits(sm.shape32(sm.BAND, n, sm.rows(F, 0, 0, big, big), size, SR))[0, 0, 3, 0] == 0
    got = sm.shape32(sm.BAND, n, sm.rows(F, 0, 0, big, big), size, SR, reject=True)
    assert bits(got)[0, 0, 3, 0] == bits(n)[0, 0, 3, 0]
    # an invalid order or a NaN edge: the gain is 0
    for row in ((300, 200, 3000, 4000), (100, 200, np.nan, 4000)):
        assert (bits(sm.shape32(sm.BAND, a, sm.rows(F, *row), size, SR)[..., 0]) == 0).all()
    # the ramps: halfway up and halfway down
    g = sm.band_gain(np.array([100, 150, 200, 1000, 3000, 3500, 4000, 4001, 99], f32), 100, 200, 3000, 4000)
    assert np.array_equal(g, np.array([0, 0.5, 1, 1, 1, 0.5, 0, 0, 0], f32))
    assert np.array_equal(sm.band_gain(np.array([100, 3000], f32), 100, 100, 3000, 3000), np.array([1, 1], f32))
    # mask of depth 0, arp of depth 0 and gain 1, stencil of level 0 on non-negative amps: the bits
    table = rng.uniform(0, 2, M + 1).astype(f32)
    table[4] = np.nan
    for d in (0.0, -1.0, np.nan):
        assert np.array_equal(bits(sm.shape32(sm.MASK, a, sm.rows(F, d), size, SR, table)), bits(a))
    for pos in (0.0, 0.37, 1.0):
        assert np.array_equal(bits(sm.shape32(sm.ARP, a, sm.rows(F, pos, 0.0, 1.0), size, SR)), bits(a)), pos
    assert np.array_equal(bits(sm.shape32(sm.STENCIL, a, sm.rows(F, 0.0, 0.0), size, SR, table)), bits(a))
    # the arp's bin: pos 0 -> bin 0, pos 1 -> bin M, a NaN -> bin 0; everything else is silenced by depth 1
    pos = np.array([0.0, 1.0, np.nan, 0.5], f32)
    clean = np.abs(np.nan_to_num(a, nan=1.0))
    got = sm.shape32(sm.ARP, clean, sm.rows(F, pos, 1.0, 2.0), size, SR)
    for f, t in enumerate((0, M, 0, M // 2)):
        nz = np.nonzero(got[0, f, :, 0] != 0)[0]
        assert nz.tolist() == [t] and got[0, f, t, 0] == f32(2) * clean[0, f, t, 0]
    # the mask in full and the stencil's threshold
    got = sm.shape32(sm.MASK, a, sm.rows(F, 1.0), size, SR, table)
    ok = np.isfinite(got[..., 0])
    assert np.array_equal(got[..., 0][ok], (a[..., 0] * (f32(0) + table))[ok])
    t2 = np.full(M + 1, 1.0, f32)
    got = sm.shape32(sm.STENCIL, a, sm.rows(F, 0.0, 0.5), size, SR, t2)
    small = a[..., 0] < f32(0.5)
    assert (got[..., 0][small] == 0).all() and np.array_equal(bits(got[..., 0][~small]), bits(a[..., 0][~small]))


@pytest.mark.parametrize("size,coefs,lowest", [(64, 1, 1), (64, 31, 5), (256, 24, 1)])
def test_warp_by_nothing_divides_and_multiplies_by_the_same_envelope(size, coefs, lowest):
    M = size // 2
    a = _frames(np.random.default_rng(size + coefs), 2, 3, size)
    r = sm.rows(3, 1.0, 0.0, 1.0)
    assert (sm.warp_map(M, 1.0, 0.0, lowest, om.bpf_of(size, SR))[lowest:M] == np.arange(lowest, M)).all()
    got = sm.shape32(sm.WARP, a, r, size, SR, lowest=lowest, coefs=coefs)
    env = om.env32(a[..., 0], coefs)
    want = (a[..., 0] / env) * env
    assert want.dtype == f32
    assert np.array_equal(bits(got[..., 1]), bits(a[..., 1]))
    assert np.array_equal(bits(got[..., lowest:M, 0]), bits(want[..., lowest:M]))
    for k in list(range(lowest)) + [M]:
        assert np.array_equal(bits(got[..., k, :]), bits(a[..., k, :]))
    assert om.rel_l2(sm.warp64_amps(a, r, size, SR, lowest, coefs), a[..., 0]) <= 1e-12
    # a frame that is not warped takes the plain gain
    r = sm.rows(3, np.array([5.0, np.nan, 1.0], f32), np.array([0.0, 0.0, 1e9], f32), 0.5)
    got = sm.shape32(sm.WARP, a, r, size, SR, lowest=lowest, coefs=coefs)
    assert np.array_equal(got[..., lowest:M, 0], f32(0.5) * a[..., lowest:M, 0])


def test_warp_moves_the_envelope_and_the_models_agree():
    size, coefs = 256, 20
    M = size // 2
    a = _frames(np.random.default_rng(11), 2, 4, size)
    r = sm.rows(4, np.array([0.25, 1.37, 4.0, 0.8], f32), np.array([0.0, 3.4 * SR / size, -3.4 * SR / size, 700.0], f32),
                np.array([1.0, -0.5, 2.0, 1.0], f32))
    m32, m64 = sm.shape32(sm.WARP, a, r, size, SR, lowest=3, coefs=coefs), sm.warp64_amps(a, r, size, SR, 3, coefs)
    assert np.isfinite(m32).all() and np.isfinite(m64).all()
    assert om.rel_l2(m32[..., 0], m64) < 1e-5
    # the map of the second frame: output bin j looks at the scale map's bin j - 3
    src = sm.warp_map(M, r[1, 0], r[1, 1], 3, om.bpf_of(size, SR))
    smap = om.scale_map_serial(M, r[1, 0])
    assert (src[:3] == om.COPY).all() and src[M] == om.COPY and src[3] == om.EMPTY
    for j in range(4, M):
        assert src[j] == (smap[j - 3] if smap[j - 3] >= 0 else om.EMPTY)
    assert (src >= 0).sum() > M // 2
    # a flat frame has a flat envelope: every bin from lowest_bin up takes the gain and nothing else
    flat = a[:, :1].copy()
    flat[..., 0] = 0.7
    got = sm.warp64_amps(flat, sm.rows(1, 2.0, 500.0, -1.5), size, SR, 3, coefs)
    assert om.rel_l2(got[..., 3:M], np.full_like(got[..., 3:M], -1.5 * float(f32(0.7)))) < 1e-12
    assert np.array_equal(got[..., :3], flat[..., :3, 0].astype(np.float64))


def test_the_bands_division_is_the_correctly_rounded_one():
    """fl(fl(x - lc) / fl(lf - lc)) as numpy's float32 division against the float64 quotient rounded once: the double
    quotient of two float32 values rounds to the float32 quotient (53 >= 2 x 24 + 2 bits), denormal results included"""
    rng = np.random.default_rng(17)
    n = 100000
    lc = (10.0 ** rng.uniform(-3, 4, n)).astype(f32)
    lf = (lc * (1 + 10.0 ** rng.uniform(-6, 2, n))).astype(f32)
    x = (lc + (lf - lc) * rng.random(n)).astype(f32)
    lc[:1000] = 0                                         # tiny numerators over large widths: denormal quotients
    lf[:1000] = (10.0 ** rng.uniform(0, 4, 1000)).astype(f32)
    x[:1000] = (10.0 ** rng.uniform(-44, -30, 1000)).astype(f32)
    keep = lf > lc
    num, den = (x - lc)[keep], (lf - lc)[keep]
    assert num.dtype == f32 and den.dtype == f32 and keep.sum() > 0.9 * n
    q32 = num / den
    q64 = (num.astype(np.float64) / den.astype(np.float64)).astype(f32)
    assert q32.dtype == f32 and int((bits(q32) != bits(q64)).sum()) == 0
    ramp = x[keep] < lf[keep]
    assert ramp.sum() > 0.8 * n and int((q32[:1000] < f32(1.2e-38)).sum()) > 500
    assert np.array_equal(bits(sm.band_gain(x[keep], lc[keep], lf[keep], lf[keep], lf[keep] * f32(2))[ramp]), bits(q64[ramp]))
