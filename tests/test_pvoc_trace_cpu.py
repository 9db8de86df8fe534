"""The N loudest bins of clfa_pvoc without a GPU: the numpy model (tests/pvoc_trace_model.py) against the definition taken
word for word (an O(B^2) count of louder candidates), the library's new symbols and device-free argument checks — which
answer on a machine without a device too — and eight mutants of the model on the GPU test's own inputs."""
import ctypes

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_trace_model as tm
from tests.pvoc_inputs import SR, raw, raw_freq_first

CL_INVALID_VALUE = -30
f32 = np.float32
GPU_SIZES = (64, 128, 512, 2048, 16384)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _recipes(size, C, F):
    return (("levels", tm.levels(size, C, F, 1)), ("near keys", tm.near_keys(size, C, F, 2)),
            ("near exponents", tm.near_keys(size, C, F, 3, True)), ("raw", raw(size, C, F, 4)),
            ("raw with NaNs", raw_freq_first(size, C, F, 5)))


@pytest.mark.parametrize("size", (64, 512))
def test_the_model_selects_what_the_definition_says(size):
    C, F = 2, 12
    B = size // 2 + 1
    for name, x in _recipes(size, C, F):
        for first, nbins in tm.ranges(B):
            n = tm.n_row(F, nbins, size + first)
            want = tm.brute_selected(x[..., 0], n, first, nbins)
            got = tm.selected(x[..., 0], n, first, nbins)
            assert np.array_equal(got, want), (name, first, nbins)
            N = tm.counts(n, nbins)
            ncand = (~np.isnan(x[:, :, first:first + nbins, 0])).sum(-1)
            assert np.array_equal(got.sum(-1), np.minimum(N[None], ncand)), (name, first, nbins)
            # the frames and the list follow the selection
            for residual in (False, True):
                y, lst = tm.trace(x, n, first, nbins, residual, nbins + 3)
                assert np.array_equal(bits(y[..., 1]), bits(x[..., 1]))
                inr = np.zeros(B, bool)
                inr[first:first + nbins] = True
                keep = ~inr | (got != residual)
                assert np.array_equal(bits(y[..., 0])[keep], bits(x[..., 0])[keep]) and not bits(y[..., 0])[~keep].any()
                for c in range(C):
                    for f in range(F):
                        k = np.nonzero(got[c, f])[0]
                        assert np.array_equal(lst[c, f, :len(k)], k) and np.all(lst[c, f, len(k):] == -1)
                for ln in (1, min(7, nbins + 3)):      # a shorter list is the longer one's head
                    assert np.array_equal(tm.trace(x, n, first, nbins, residual, ln)[1], lst[..., :ln])


def test_the_count_rule():
    n = np.array([0, 1, 2.5, 3.5, 3.999, 10, 15, np.inf, np.nan, -1, -0.0, -np.inf, 1e30], f32)
    assert list(tm.counts(n, 10)) == [0, 1, 2, 3, 3, 10, 10, 10, 0, 0, 0, 0, 10]
    assert list(tm.counts(np.array([2.5, 3.5], f32), 10, "n_rounded")) == [2, 4]


def test_library_exports_the_trace_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in ("clfa_pvoc_trace_dev", "clfa_pvoc_trace", "clfa_pvoc_trace_kernel_name"):
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.trace_kernel_name() == ""
    pv = fa.Pvoc(0, 64, 16, SR, 2)
    assert pv.trace_kernel_name() == ("k_pvoc_trace" if pv.get_error() == 0 else "")
    assert _lib.lib().clfa_pvoc_trace_kernel_name(None) == b""
    for m in ("trace", "trace_device", "trace_kernel_name"):
        assert callable(getattr(pv, m))
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/clfft_amd.h").read()
    assert "CLFA_PVOC_TRACE_RESIDUAL = 1" in header and fa.Pvoc.TRACE_RESIDUAL == 1


def test_argument_errors_come_before_the_device_lookup():
    size, C, F, LN = 64, 2, 3, 5
    M = size // 2
    pv = fa.Pvoc(0, size, 16, SR, C)
    good = pv.get_error()                  # 0 with a device, "Device not found" without: what a good call returns
    assert good == (0 if fa.device_count() > 0 else -1)
    L = _lib.lib()
    a = tm.levels(size, C, F, 5)
    nn = np.array([2, 3.5, 40], f32)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    # 8-byte aligned host arrays: numpy's allocations are, the views below start from them
    room = np.zeros(a.size + 2, f32)
    out = room[(-room.ctypes.data % 8) // 4:][:a.size].reshape(a.shape)
    out[:] = 7.0
    lst = np.full((C, F, LN), 9, np.int32)
    assert a.ctypes.data % 8 == 0 and out.ctypes.data % 8 == 0

    def host(a=a, o=out, n=nn, b=lst, ln=LN, F=F, first=0, nbins=M + 1, flags=0, h=pv._h):
        return L.clfa_pvoc_trace(h, ptr(a), ptr(o), ptr(n), ptr(b), ln, F, first, nbins, flags)

    def devf(a=a, o=out, n=nn, b=lst, ln=LN, F=F, first=0, nbins=M + 1, flags=0, h=pv._h):    # the device form's checks,
        return L.clfa_pvoc_trace_dev(h, ptr(a), ptr(o), ptr(n), ptr(b), ln, F, first, nbins, flags, None)   # on host addresses

    for f in (host, devf):
        assert f(F=0) == good and f(F=-1) == CL_INVALID_VALUE
        assert f(F=0, a=None, o=None, n=None, b=None) == good
        for kw in (dict(a=None), dict(o=None), dict(n=None), dict(h=None)):
            assert f(**kw) == CL_INVALID_VALUE, kw
        for first, nbins in ((0, 0), (0, M + 2), (1, M + 1), (-1, 2), (M + 1, 1), (M, 2), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(first=first, nbins=nbins) == CL_INVALID_VALUE, (first, nbins)
            assert f(first=first, nbins=nbins, F=0) == CL_INVALID_VALUE, (first, nbins)
        for flags in (2, 3, 4, -1, 1 << 30):
            assert f(flags=flags) == CL_INVALID_VALUE, flags
            assert f(flags=flags, F=0) == CL_INVALID_VALUE, flags
        for ln in (0, -1):
            assert f(ln=ln) == CL_INVALID_VALUE, ln          # asked of a list that is given,
            assert f(ln=ln, b=None) == good, ln              # and not looked at without one
        # each output against each input and against the other output: the two share the last one or two words of the
        # lower one (two where that keeps both on 8 bytes, so that the overlap is all a device form can object to)
        args = {"a": a, "o": out, "n": nn, "b": lst}
        for okey in ("o", "b"):
            for xkey in ("a", "n", "o", "b"):
                if xkey == okey:
                    continue
                for lower, upper in ((xkey, okey), (okey, xkey)):
                    n0, n1 = args[lower].size, args[upper].size
                    both = np.zeros(n0 + n1 + 2, np.uint32)
                    start = (-both.ctypes.data % 8) // 4
                    s1 = start + n0 - 1
                    s1 -= (s1 - start) % 2
                    v0 = both[start:start + n0].view(args[lower].dtype).reshape(args[lower].shape)
                    v1 = both[s1:s1 + n1].view(args[upper].dtype).reshape(args[upper].shape)
                    assert v0.ctypes.data % 8 == 0 and v1.ctypes.data % 8 == 0 and v1.ctypes.data < v0.ctypes.data + v0.nbytes
                    assert f(**{lower: v0, upper: v1}) == CL_INVALID_VALUE, (lower, upper)
    # the device form's alignment: frames on 8 bytes, n and the list on 4 (the blocking form takes any address)
    bytes_ = np.zeros(a.nbytes + 16, np.uint8)
    base = bytes_.ctypes.data + (-bytes_.ctypes.data % 8)
    for kw, off, refused in (("a", 4, True), ("o", 4, True), ("n", 2, True), ("b", 2, True), ("a", 8, False), ("n", 4, False)):
        assert devf(**{kw: base + off}) == (CL_INVALID_VALUE if refused else good), (kw, off)
    assert devf(b=base + 2, ln=0) == CL_INVALID_VALUE and devf(b=None, ln=0) == good
    assert host() == good and host(flags=1, first=M, nbins=1) == good and host(b=None, ln=-3) == good
    assert host(n=np.array([np.nan, -1, np.inf], f32)) == good         # every n has a meaning
    if good != 0:
        assert np.all(out == 7.0) and np.all(lst == 9)
    # the Python layer: shapes and ranges
    with pytest.raises(ValueError):
        pv.trace(a[:, :, :-1], 3)
    for kw in (dict(first_bin=-1), dict(first_bin=M + 1), dict(nbins=0), dict(first_bin=2, nbins=M)):
        with pytest.raises(fa.ClError) as e:
            pv.trace(a, 3, **kw)
        assert e.value.code == CL_INVALID_VALUE


def gpu_cases(size, C, F):
    """the (name, frames, first_bin, nbins, n) the GPU test runs on the levels recipe: the four ranges, the planted n"""
    B = size // 2 + 1
    x = tm.levels(size, C, F, size)
    return [("levels range %d %d" % r, x, r[0], r[1], tm.n_row(F, r[1], size + i)) for i, r in enumerate(tm.ranges(B))]


@pytest.mark.parametrize("mutant", tm.MUTANTS)
def test_every_mutant_of_the_model_changes_a_frame_at_every_size(mutant):
    for size in GPU_SIZES:
        changed = total = 0
        for name, x, first, nbins, n in gpu_cases(size, 1, 37):
            good, glist = tm.trace(x, n, first, nbins, False, nbins + 3)
            bad, blist = tm.trace(x, n, first, nbins, False, nbins + 3, mutant=mutant)
            differs = np.any(bits(good) != bits(bad), axis=(0, 2, 3)) | np.any(glist != blist, axis=(0, 2))
            changed += int(differs.sum())
            total += differs.size
        print("PVOCTRACE mutant %s size %d: %d of %d frame-cases differ" % (mutant, size, changed, total))
        assert changed >= 1, "size %d: no frame notices the mutant %s" % (size, mutant)
