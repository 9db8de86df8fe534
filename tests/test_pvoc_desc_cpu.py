"""The per-frame descriptors of clfa_pvoc without a GPU: the library's new symbols and argument checks — which come before
any device lookup, so they answer on a machine without a device too — and properties of the numpy model of the
definition (tests/pvoc_desc_model.py): its tree sums against float64, its peak against np.nanargmax, the identity after a
reset, cutting, and seven mutants of the model on the GPU test's own inputs (tests/pvoc_desc_cases.py)."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_desc_cases as dc
from tests import pvoc_desc_model as dm

CL_INVALID_VALUE = -30
SR = dc.SR
f32 = np.float32
ALL_SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differs(a, b):
    """some compared value differs: the test of tests/gpu_guard.py's same(), negated"""
    na, nb = np.isnan(a), np.isnan(b)
    return not np.array_equal(na, nb) or not np.array_equal(bits(a)[~na], bits(b)[~na])


def test_library_exports_the_desc_symbols():
    names = ["clfa_pvoc_desc_dev", "clfa_pvoc_desc", "clfa_pvoc_desc_read_state", "clfa_pvoc_desc_state_bytes",
             "clfa_pvoc_desc_kernel_name"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in names:
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.desc_kernel_name() == "" and bad.desc_state_bytes() == 0
    pv = fa.Pvoc(0, 64, 16, SR, 2)
    assert pv.desc_kernel_name() == ("k_pvoc_desc" if pv.get_error() == 0 else "")
    for m in ("describe", "describe_device", "desc_state", "desc_state_bytes", "desc_kernel_name"):
        assert callable(getattr(pv, m))
    cols = [fa.Pvoc.DESC_MAG, fa.Pvoc.DESC_POW, fa.Pvoc.DESC_MOM, fa.Pvoc.DESC_CENT, fa.Pvoc.DESC_FLUX,
            fa.Pvoc.DESC_PEAK_AMP, fa.Pvoc.DESC_PEAK_FREQ, fa.Pvoc.DESC_PEAK_BIN]
    assert cols == list(range(8)) == [dm.MAG, dm.POW, dm.MOM, dm.CENT, dm.FLUX, dm.PEAK_AMP, dm.PEAK_FREQ, dm.PEAK_BIN]
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/clfft_amd.h").read()
    for i, n in enumerate(("MAG", "POW", "MOM", "CENT", "FLUX", "PEAK_AMP", "PEAK_FREQ", "PEAK_BIN")):
        assert "CLFA_PVOC_DESC_%s = %d" % (n, i) in header


def test_argument_errors_come_before_the_device_lookup():
    size, C, F = 64, 2, 3
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    a = dc.plain(size, C, F, 5)
    out = np.full((C, F, 8), 7.0, f32)
    ptr = lambda x: None if x is None else x.ctypes.data

    def host(a=a, o=out, F=F, first=0, nbins=M + 1, rectify=0, h=pv._h):
        return L.clfa_pvoc_desc(h, ptr(a), ptr(o), F, first, nbins, rectify)

    def devf(a=a, o=out, F=F, first=0, nbins=M + 1, rectify=0, h=pv._h):      # the device form's checks, on host addresses
        return L.clfa_pvoc_desc_dev(h, ptr(a), ptr(o), F, first, nbins, rectify, None)

    for f in (host, devf):
        assert f(F=0) == good and f(F=-1) == CL_INVALID_VALUE
        assert f(a=None) == CL_INVALID_VALUE and f(o=None) == CL_INVALID_VALUE and f(h=None) == CL_INVALID_VALUE
        for first, nbins in ((0, 0), (0, M + 2), (1, M + 1), (-1, 2), (M + 1, 1), (M, 2), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(first=first, nbins=nbins) == CL_INVALID_VALUE, (first, nbins)
            assert f(first=first, nbins=nbins, F=0) == CL_INVALID_VALUE, (first, nbins)
        for rectify in (2, -1):
            assert f(rectify=rectify) == CL_INVALID_VALUE
        # an output overlapping the input by one element, from either side
        both = np.zeros(a.size + out.size, f32)
        lo, hi = both[:a.size].reshape(a.shape), both[a.size - 1:a.size - 1 + out.size].reshape(out.shape)
        assert f(a=lo, o=hi) == CL_INVALID_VALUE
        lo, hi = both[:out.size].reshape(out.shape), both[out.size - 1:out.size - 1 + a.size].reshape(a.shape)
        assert f(a=hi, o=lo) == CL_INVALID_VALUE
    assert host() == good and host(first=M, nbins=1, rectify=1) == good and host(first=0, nbins=1) == good
    if good != 0:
        assert np.all(out == 7.0)
    assert L.clfa_pvoc_desc_read_state(pv._h, None) == (CL_INVALID_VALUE if good == 0 else good)
    assert L.clfa_pvoc_desc_read_state(None, ptr(out)) == CL_INVALID_VALUE
    assert L.clfa_pvoc_desc_state_bytes(None) == 0 and L.clfa_pvoc_desc_kernel_name(None) == b""
    # the Python layer: shapes and ranges
    with pytest.raises(ValueError):
        pv.describe(a[:, :, :-1])
    for kw in (dict(first_bin=-1), dict(first_bin=M + 1), dict(nbins=0), dict(first_bin=2, nbins=M)):
        with pytest.raises(fa.ClError) as e:
            pv.describe(a, **kw)
        assert e.value.code == CL_INVALID_VALUE


@pytest.mark.parametrize("size", ALL_SIZES)
def test_the_models_sums_are_near_the_float64_sums(size):
    """|T - sum64| <= (M / W + log2 W + 1) 2^-24 sum|t|: a term passes through at most M / W - 1 additions of its lane,
    log2 W levels of the tree and the Nyquist addition, each with a relative error of at most 2^-24 of a partial sum that
    the sum of |t| bounds (first order; the measured ratios are printed)"""
    M = size // 2
    W = dm.lanes(M)
    C, F = 2, 6
    x = dc.plain(size, C, F, size)
    x[0, :, :, 0] *= np.where(np.arange(M + 1) % 3 == 0, -1, 1).astype(f32)     # mixed signs in one channel
    last = dc.plain(size, C, 1, size + 1)[:, 0, :, 0]
    bound = (M // W + np.log2(W) + 1) * 2.0 ** -24
    worst = 0.0
    for name, first, nbins in dc.ranges(M):
        for rectify in (False, True):
            desc, _ = dm.describe32(x, last, size, SR, first, nbins, rectify)
            s64, sabs = dm.sums64(x, last, size, SR, first, nbins, rectify)
            got = desc[..., [dm.MAG, dm.POW, dm.MOM, dm.FLUX]].astype(np.float64)
            err = np.abs(got - s64)
            assert np.all(err <= bound * sabs), (name, rectify)
            worst = max(worst, float(np.max(err / np.maximum(sabs, 1e-300))) / bound)
    print("PVOCDESC size %d: the model's largest error is %.3f of the bound" % (size, worst))


def _peak_by_nanargmax(a, lo, hi):
    """(amp index or -1) of one frame's amps"""
    r = a[lo:hi + 1]
    if np.isnan(r).all():
        return -1
    return lo + int(np.nanargmax(r))          # the first of equal maxima; -0 == +0


@pytest.mark.parametrize("size", (64, 512, 1024))
def test_the_models_peak_is_nanargmax_with_the_tie_rule(size):
    M = size // 2
    for C in (1, 3):
        for name, x, first, nbins, rectify in dc.planted(size, C) + dc.streams(size, C, counts=(5,)):
            lo, hi = dm.selection(M, first, nbins)
            desc, _ = dm.describe32(x, np.zeros((C, M + 1), f32), size, SR, first, nbins, rectify)
            for c in range(C):
                for f in range(x.shape[1]):
                    kp = _peak_by_nanargmax(x[c, f, :, 0], lo, hi)
                    row = desc[c, f]
                    assert row[dm.PEAK_BIN] == kp, (name, c, f)
                    want = x[c, f, kp] if kp >= 0 else np.zeros(2, f32)
                    assert np.array_equal(bits(row[[dm.PEAK_AMP, dm.PEAK_FREQ]]), bits(want)), (name, c, f)


def test_frame_0_after_a_reset_has_the_flux_of_its_pow():
    """d = fl(a - 0) = a, so the two columns are the same sums — without rectify; with it a negative amp drops out"""
    for size in (64, 1024):
        M = size // 2
        x = dc.plain(size, 2, 3, 3)
        for name, first, nbins in dc.ranges(M):
            s = dm.Stream(2, size, SR)
            d = s.run(x, first, nbins)
            assert np.array_equal(bits(d[:, 0, dm.FLUX]), bits(d[:, 0, dm.POW])), name
            assert not np.array_equal(bits(d[:, 1, dm.FLUX]), bits(d[:, 1, dm.POW]))
            s.reset()
            assert np.array_equal(bits(s.run(x, first, nbins)), bits(d))
            s.reset()
            assert np.array_equal(bits(s.run(x, first, nbins, True)[:, 0, dm.FLUX]), bits(d[:, 0, dm.POW]))


@pytest.mark.parametrize("size", (64, 1024))
def test_the_model_cut_at_any_frame_gives_the_same_rows_and_state(size):
    C, F = 2, 9
    M = size // 2
    x = dc.plain(size, C, F, 11)
    x[1, 4, M // 2, 0] = np.nan
    for first, nbins, rectify in ((0, None, False), (3, M // 2, True)):
        whole = dm.Stream(C, size, SR)
        want = whole.run(x, first, nbins, rectify)
        for cut in range(F + 1):
            s = dm.Stream(C, size, SR)
            got = np.concatenate([s.run(x[:, :cut], first, nbins, rectify), s.run(x[:, cut:], first, nbins, rectify)], axis=1)
            assert not differs(got, want), cut
            assert np.array_equal(bits(s.last), bits(whole.last)) and np.array_equal(bits(s.last), bits(x[:, -1, :, 0]))
    s = dm.Stream(C, size, SR)
    s.run(x)
    before = s.last.copy()
    assert s.run(x[:, :0]).shape == (C, 0, 8) and np.array_equal(bits(s.last), bits(before))


def _two_calls(size, C, case, mutant):
    """what the GPU test compares of a case: the rows of the call, the state after it, and the rows of a second call over
    everything that goes on from that state"""
    name, x, first, nbins, rectify = case
    s = dm.Stream(C, size, SR, mutant)
    rows = s.run(x, first, nbins, rectify)
    state = s.last.copy()
    return rows, state, s.run(x[:, :2], 0, None, rectify)


def _cases(size, C):
    return dc.planted(size, C) + dc.streams(size, C, counts=(5, 37))


@pytest.mark.parametrize("mutant", dm.MUTANTS)
def test_every_mutant_of_the_model_shows_in_a_compared_value(mutant):
    """on the GPU test's own inputs; W = 64 cannot show below M = 128, the others show at every size tried"""
    for size in (64, 256, 1024):
        C = 3
        hit = []
        for case in _cases(size, C):
            good, bad = _two_calls(size, C, case, None), _two_calls(size, C, case, mutant)
            if any(differs(g, b) for g, b in zip(good, bad)):
                hit.append(case[0])
        print("PVOCDESC mutant %s size %d: %d cases differ" % (mutant, size, len(hit)))
        assert hit or (mutant == "w64" and size == 64), "size %d: no case notices the mutant %s" % (size, mutant)


@pytest.mark.parametrize("size", ALL_SIZES)
def test_a_wrong_order_of_the_additions_changes_the_bits_at_every_size(size):
    x = dc.plain(size, 1, 40, size)
    last = np.zeros((1, size // 2 + 1), f32)
    good, _ = dm.describe32(x, last, size, SR)
    for mutant in ("serial", "halving", "nyquist_first"):
        bad, _ = dm.describe32(x, last, size, SR, mutant=mutant)
        rows = np.any(bits(good) != bits(bad), axis=-1).mean()
        print("PVOCDESC size %d mutant %s: %.0f %% of the rows differ" % (size, mutant, 100 * rows))
        assert rows > 0.1, mutant
