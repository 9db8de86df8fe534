"""The stereo demix of clfa_pvoc without a GPU: properties of the numpy model (tests/pvoc_demix_model.py), the kernels'
per-bin code (opencl_fft_amd/csrc/pvoc_demix_bin.hpp, two bisections) built with g++ against the model's literal scan, twelve
mutants of the model on the GPU test's own inputs, and the library's new symbols and device-free argument checks — which
answer on a machine without a device too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_demix_model as dm
from tests.pvoc_inputs import SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL_INVALID_VALUE = -30
f32 = np.float32
GPU_SIZES = (64, 128, 512, 2048, 16384)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_cases(size, C, F):
    """the (name, left, right, par, P, first_bin, nbins) the GPU test runs at every size: the panned recipe at P = 1, 8 and
    100 over all bins and over the inner range (3, B - 5), the rows of (pos, width) walking the widths 1, 4, 2P + 1 and the
    positions -1, -0.0, 0.37, 1 from a different start in each; and two unrelated streams, one with NaNs.  The largest
    size has P = 100 over all bins alone: its model is the slowest."""
    B = size // 2 + 1
    whole, inner = (0, None), (3, B - 5)
    plan = [(1, whole), (8, inner), (8, whole), (100, whole), (1, inner)] + ([(100, inner)] if size < 16384 else [])
    cases = []
    for i, (P, (first, nbins)) in enumerate(plan):
        left, right, _ = dm.panned(size, C, F, P, size + i)
        cases.append(("panned P %d range %d %s" % (P, first, nbins), left, right, dm.par_rows(F, P, i), P, first, nbins))
    left, right = dm.pair(size, C, F, 40)
    cases.append(("two raw streams P 8", left, right, dm.par_rows(F, 8, 2), 8, 0, None))
    return cases


# ---- properties of the model -------------------------------------------------------------------------------------------

def test_the_panned_sources_come_apart():
    """P = 10; sources at 0.3 left, the centre and 0.6 right; width 1: the kept set of each position is that source's bins"""
    size, C, F, P = 256, 2, 6, 10
    pans = [(-1, 7), (1, 10), (1, 4)]            # u = -3, 0, 6
    left, right, src = dm.panned(size, C, F, P, 11, pans)
    for i, pos in enumerate((-0.3, 0.0, 0.6)):
        out, prof = dm.demix(left, right, np.tile(np.array([pos, 1], f32), (F, 1)), P)
        assert np.array_equal(out[..., 0] != 0, src == i), pos
        assert (src == i).any()
        # and the profile shows the three sources and nothing else
        assert np.array_equal(np.nonzero(prof.sum(axis=(0, 1)))[0], [P - 3, P, P + 6])


def _tree_depth(M):
    W = min(M, 256)
    return M // W + int(np.log2(W)) + 1


@pytest.mark.parametrize("size,P", [(64, 1), (64, 8), (512, 8), (512, 100), (2048, 8)])
def test_the_profile_and_the_kept_amps_agree(size, P):
    C, F = 2, 12
    M = size // 2
    for name, (left, right) in (("panned", dm.panned(size, C, F, P, 5)[:2]), ("pair", dm.pair(size, C, F, 6))):
        for first, nbins in ((0, None), (3, M + 1 - 5)):
            par = dm.par_rows(F, P, 1)
            out, prof = dm.demix(left, right, par, P, first, nbins)
            assert not np.isnan(prof).any() and not np.signbit(prof).any(), "a column is finite or +inf, never a NaN"
            assert np.array_equal(bits(dm.demix(left, right, par, P, first, nbins, az=False)[0]), bits(out))
            c, H = dm.window(par, P)
            j = np.arange(2 * P + 1) - P
            inside = np.abs(j[None, :] - c[:, None]) <= H[:, None]                    # (F, 2P + 1)
            with np.errstate(all="ignore"):
                win = np.where(inside[None], prof.astype(np.float64), 0).sum(-1)
                amps = out[..., 0].astype(np.float64).sum(-1)
            fin = np.isfinite(amps)
            assert np.array_equal(np.isfinite(win), fin), name
            assert np.all(np.abs(win - amps)[fin] <= _tree_depth(M) * 2.0 ** -24 * amps[fin]), name
            # a NaN or an infinite input is never kept; the freq is one of the inputs'
            odd = ~np.isfinite(left[..., 0]) | ~np.isfinite(right[..., 0])
            assert odd.any() and not bits(out[..., 0])[odd].any(), name
            assert np.all((bits(out[..., 1]) == bits(left[..., 1])) | (bits(out[..., 1]) == bits(right[..., 1])))


def test_minus_zero_is_the_centre_and_the_clamps():
    size, C, F, P = 128, 1, 4, 8
    left, right, _ = dm.panned(size, C, F, P, 3)
    rows = lambda pos, width: np.tile(np.array([pos, width], f32), (F, 1))
    a, pa = dm.demix(left, right, rows(-0.0, 3), P)
    b, pb = dm.demix(left, right, rows(0.0, 3), P)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(pa), bits(pb))
    assert list(dm.window(np.array([[-0.0, 1], [np.nan, np.nan], [7, 1e9], [-7, -3], [0.37, 4], [0.5, 2.9], [0.3125, 17.5]], f32), 8)[0]) \
        == [0, -8, 8, -8, 3, 4, 2]                                   # rintf: 2.96 -> 3, 4.0 -> 4, 2.5 -> 2 (to even)
    assert list(dm.window(np.array([[0, 1], [0, np.nan], [0, 1e9], [0, -3], [0, 4], [0, 2.9], [0, 17.5]], f32), 8)[1]) \
        == [0, 0, 8, 0, 2, 1, 8]
    assert dm.values_ok(rows(-1, 17), 8) and dm.values_ok(rows(1, 1), 8)
    for pos, width in ((1.5, 3), (np.nan, 3), (0, 0.5), (0, 18), (0, np.nan), (np.inf, 1), (0, np.inf)):
        assert not dm.values_ok(rows(pos, width), 8), (pos, width)


# ---- the kernels' per-bin code against the literal scan ----------------------------------------------------------------------

PROGRAM = r"""
#include "pvoc_demix_bin.hpp"
extern "C" void demix_bins(const float *L, const float *R, long n, int P, int *left, int *placed, int *u, float *mag) {
  for (long i = 0; i < n; i++) {
    const clfa::DemixBin b = clfa::demix_bin(L[i], R[i], P);
    left[i] = b.left, placed[i] = b.placed, u[i] = b.u, mag[i] = b.mag;
  }
}
extern "C" void demix_windows(const float *par, long F, int P, int *c, int *H) {
  for (long f = 0; f < F; f++) {
    const clfa::DemixWindow w = clfa::demix_window(par[2 * f], par[2 * f + 1], P);
    c[f] = w.c, H[f] = w.H;
  }
}
"""


@pytest.fixture(scope="module")
def host_bins(tmp_path_factory):
    d = tmp_path_factory.mktemp("demix_bin")
    (d / "prog.cpp").write_text(PROGRAM)
    so = str(d / "libdemix_bin.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall",
                           "-I", os.path.join(ROOT, "opencl_fft_amd", "csrc"), str(d / "prog.cpp"), "-o", so])
    return ctypes.CDLL(so)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _host_scan(lib, L, R, P):
    L, R = np.ascontiguousarray(L, f32).ravel(), np.ascontiguousarray(R, f32).ravel()
    left, placed, u = (np.zeros(L.size, np.int32) for _ in range(3))
    mag = np.zeros(L.size, f32)
    lib.demix_bins(_ptr(L), _ptr(R), ctypes.c_long(L.size), P, _ptr(left), _ptr(placed), _ptr(u), _ptr(mag))
    return left.astype(bool), placed.astype(bool), u, mag


@pytest.mark.parametrize("P", [1, 2, 3, 8, 10, 100, 101, 1000, 1024])
def test_the_bisections_give_the_scans_bits(host_bins, P):
    """the side, whether the bin is placed, and where it is, u and the bits of mag: on bins at a gain of the grid and an ulp
    beside it, between the gains, exactly tied, of either sign, tiny, huge, and every pair of a list of odd values"""
    rng = np.random.default_rng(P)
    n = 20000 if P < 200 else 3000
    with np.errstate(all="ignore"):
        loud = (10.0 ** rng.uniform(-3, 3, n)).astype(f32)
        on = dm.gains(P)[rng.integers(0, P + 1, n)] * loud
        odd = np.array([0, -0.0, 1, -1, 2, -2, 0.5, -0.5, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3e38, -3e38, 1e-40, 3,
                        0.75], f32)
        a, b = np.meshgrid(odd, odd)
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-40, 37, n)).astype(f32)
        y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-40, 37, n)).astype(f32)
        tl = (2.0 ** rng.integers(-3, 4, n)).astype(f32)
        tq = (tl * ((rng.integers(0, P, n) + 0.5) / P)).astype(f32)
        tiny = lambda: (rng.integers(0, 40, n) * f32(1e-45)).astype(f32)
        cases = [(loud, (loud * rng.random(n).astype(f32)).astype(f32)), (loud, on), (on, loud),
                 (loud, np.nextafter(on, f32(np.inf))), (np.nextafter(on, f32(-np.inf)), loud), (a.ravel(), b.ravel()), (x, y),
                 (x, (x * rng.uniform(-1.5, 1.5, n)).astype(f32)), (tl, tq), (-tl, -tq), (-tq, -tl), (tiny(), tiny())]
    for i, (L, R) in enumerate(cases):
        wl, wp, wu, wm = dm.scan(L, R, P)
        gl, gp, gu, gm = _host_scan(host_bins, L, R, P)
        assert np.array_equal(gl, wl) and np.array_equal(gp, wp), i
        assert np.array_equal(gu[wp], wu[wp]) and np.array_equal(bits(gm)[wp], bits(wm)[wp]), i
    par = np.concatenate([dm.edge_rows(10, P), dm.par_rows(12, P),
                          np.stack([rng.uniform(-1.2, 1.2, 500), rng.uniform(0, 2 * P + 3, 500)], 1).astype(f32)])
    c, H = np.zeros(len(par), np.int32), np.zeros(len(par), np.int32)
    host_bins.demix_windows(_ptr(par), ctypes.c_long(len(par)), P, _ptr(c), _ptr(H))
    wc, wH = dm.window(par, P)
    assert np.array_equal(c, wc) and np.array_equal(H, wH)


# ---- the mutants ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", GPU_SIZES + (256, 1024))
def test_every_mutant_of_the_model_changes_an_output_at_this_size(size):
    cases = [(c, dm.demix(*c[1:])) for c in gpu_cases(size, 1, 5)]
    for mutant in dm.MUTANTS:
        changed = []
        for (name, left, right, par, P, first, nbins), (good, gprof) in cases:
            if mutant == "g_recip" and P & (P - 1) == 0:
                continue                        # the two grids are the same numbers
            bad, bprof = dm.demix(left, right, par, P, first, nbins, mutant=mutant)
            if np.any(bits(good) != bits(bad)) or np.any(bits(gprof) != bits(bprof)):
                changed.append(name)
        print("PVOCDEMIX mutant %s size %d: noticed by %d of %d cases" % (mutant, size, len(changed), len(cases)))
        assert changed, "size %d: no case notices the mutant %s" % (size, mutant)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_library_exports_the_demix_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = [s[0] for s in _lib.SYMBOLS]
    for n in ("clfa_pvoc_demix_dev", "clfa_pvoc_demix", "clfa_pvoc_demix_kernel_name"):
        assert hasattr(L, n) and n in bound, n
    bad = fa.Pvoc(0, 48, 16, SR)
    assert bad.demix_kernel_name() == "" and bad.demix_kernel_name(az=True) == ""
    pv = fa.Pvoc(0, 64, 16, SR, 2)
    ok = pv.get_error() == 0
    assert pv.demix_kernel_name() == ("k_pvoc_demix" if ok else "")
    assert pv.demix_kernel_name(az=True) == ("k_pvoc_demix_az" if ok else "")
    assert _lib.lib().clfa_pvoc_demix_kernel_name(None, 1) == b""
    for m in ("demix", "demix_device", "demix_kernel_name"):
        assert callable(getattr(pv, m))


def test_argument_errors_come_before_the_device_lookup():
    """an object created on device 99: a bad argument is CLFA_INVALID_VALUE, a good call the object's error"""
    size, C, F, P = 64, 2, 3, 8
    M = size // 2
    none = fa.Pvoc(99, size, 16, SR, C)
    good = none.get_error()
    assert good != 0 and none.demix_kernel_name() == ""
    L = _lib.lib()
    left, right, _ = dm.panned(size, C, F, P, 5)
    par = dm.par_rows(F, P)
    ptr = lambda x: None if x is None else (x if isinstance(x, int) else x.ctypes.data)
    out = np.full(left.shape, 7.0, f32)
    az = np.full((C, F, 2 * P + 1), 9.0, f32)
    assert all(a.ctypes.data % 8 == 0 for a in (left, right, out, par, az))

    def host(l=left, r=right, o=out, p=par, a=az, F=F, P=P, first=0, nbins=M + 1, h=none._h):
        return L.clfa_pvoc_demix(h, ptr(l), ptr(r), ptr(o), ptr(p), ptr(a), F, P, first, nbins)

    def devf(l=left, r=right, o=out, p=par, a=az, F=F, P=P, first=0, nbins=M + 1, h=none._h):   # the device form's checks,
        return L.clfa_pvoc_demix_dev(h, ptr(l), ptr(r), ptr(o), ptr(p), ptr(a), F, P, first, nbins, None)   # on host addresses

    for f in (host, devf):
        assert f() == good and f(a=None) == good and f(r=left) == good          # the two inputs may be one buffer
        assert f(F=0) == good and f(F=-1) == CL_INVALID_VALUE
        assert f(F=0, l=None, r=None, o=None, p=None, a=None) == good
        for kw in (dict(l=None), dict(r=None), dict(o=None), dict(p=None), dict(h=None)):
            assert f(**kw) == CL_INVALID_VALUE, kw
        for P_ in (0, -1, 1025, 2 ** 31 - 1):
            assert f(P=P_) == CL_INVALID_VALUE and f(P=P_, F=0) == CL_INVALID_VALUE and f(P=P_, a=None) == CL_INVALID_VALUE, P_
        assert f(P=1, a=None) == good and f(P=1024, a=None, p=np.tile(np.array([0, 1], f32), (F, 1))) == good
        for first, nbins in ((0, 0), (0, M + 2), (1, M + 1), (-1, 2), (M + 1, 1), (M, 2), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert f(first=first, nbins=nbins) == CL_INVALID_VALUE, (first, nbins)
            assert f(first=first, nbins=nbins, F=0) == CL_INVALID_VALUE, (first, nbins)
        # each output against each input and against the other output: the two share the last one or two words of the
        # lower one (two where that keeps both on 8 bytes, so that the overlap is all a device form can object to)
        args = {"l": left, "r": right, "o": out, "p": par, "a": az}
        for okey in ("o", "a"):
            for xkey in args:
                if xkey == okey:
                    continue
                for lower, upper in ((xkey, okey), (okey, xkey)):
                    n0, n1 = args[lower].size, args[upper].size
                    both = np.zeros(n0 + n1 + 2, np.uint32)
                    start = (-both.ctypes.data % 8) // 4
                    s1 = start + n0 - 1
                    s1 -= (s1 - start) % 2
                    v0 = both[start:start + n0].view(f32).reshape(args[lower].shape)
                    v1 = both[s1:s1 + n1].view(f32).reshape(args[upper].shape)
                    for v, key in ((v0, lower), (v1, upper)):
                        if key == "p":
                            v[:] = par                                   # values the blocking form accepts
                    assert v0.ctypes.data % 8 == 0 and v1.ctypes.data % 8 == 0 and v1.ctypes.data < v0.ctypes.data + v0.nbytes
                    assert f(**{lower: v0, upper: v1}) == CL_INVALID_VALUE, (lower, upper)
    # the device form's alignment: frames on 8 bytes, par and the profile on 4 (the blocking form takes any address)
    bytes_ = np.zeros(left.nbytes + 16, np.uint8)
    base = bytes_.ctypes.data + (-bytes_.ctypes.data % 8)
    for kw, off, refused in (("l", 4, True), ("r", 4, True), ("o", 4, True), ("p", 2, True), ("a", 2, True), ("l", 8, False),
                             ("p", 4, False), ("a", 4, False)):
        assert devf(**{kw: base + off}) == (CL_INVALID_VALUE if refused else good), (kw, off)
    # the blocking form refuses per-frame values outside their meaning; the device form clamps them
    for pos, width in ((1.5, 3), (-1.0000001, 3), (np.nan, 3), (np.inf, 3), (0, 0.5), (0, 2 * P + 2), (0, np.nan), (0, -np.inf)):
        bad = par.copy()
        bad[F - 1] = (pos, width)
        assert host(p=bad) == CL_INVALID_VALUE and devf(p=bad) == good, (pos, width)
    edge = np.array([[-1, 1], [1, 2 * P + 1], [-0.0, 1.5]], f32)
    assert host(p=edge) == good
    assert np.all(out == 7.0) and np.all(az == 9.0)
    # the Python layer: shapes, ranges, values
    with pytest.raises(ValueError):
        none.demix(left[:, :, :-1], right[:, :, :-1], 0, 1, P)
    with pytest.raises(ValueError):
        none.demix(left, right[:, :-1], 0, 1, P)
    for args, kw in (((0, 1, P), dict(first_bin=-1)), ((0, 1, P), dict(nbins=0)), ((0, 1, P), dict(first_bin=2, nbins=M)),
                     ((0, 1, 0), {}), ((0, 1, 1025), dict(az=True)), ((2, 1, P), {}), ((0, 0, P), {}),
                     ((np.array([0, 0, np.nan], f32), 1, P), {})):
        with pytest.raises(fa.ClError) as e:
            none.demix(left, right, *args, **kw)
        assert e.value.code == CL_INVALID_VALUE, (args, kw)
    with pytest.raises(fa.ClError) as e:
        none.demix(left, right, np.array([-1, 0, 1], f32), 3, P, az=True)
    assert e.value.code == good


# ---- the Python layer's argument contract, a row per call (the style of tests/test_python_args_cpu.py) --------------------

def _demix_rows():
    import torch
    INVALID, NO_DEVICE = CL_INVALID_VALUE, -1
    size, F = 64, 3
    M = size // 2
    f64 = torch.float64
    PV, PV1 = fa.Pvoc(0, size, 16, SR, 2), fa.Pvoc(0, size, 16, SR, 1)
    fr = lambda c=2, f=F, dt=torch.float32: torch.zeros(((c,) if c else ()) + (f, M + 1, 2), dtype=dt)
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    strided = lambda t: torch.stack([t, t], dim=-1)[..., 0]
    nfr = lambda c=2: np.zeros(((c,) if c else ()) + (F, M + 1, 2), f32)
    host = lambda code: (fa.ClError, code)
    return [
        ("demix_device numbers", lambda: PV.demix_device(fr(), fr(), fr(), (0.25, 3), 8, stream=0), NO_DEVICE),
        ("demix_device rows", lambda: PV.demix_device(fr(), fr(), fr(), z(F, 2), 8, 2, 5, stream=0), NO_DEVICE),
        ("demix_device az_out", lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 8, az_out=z(2, F, 17), stream=0), NO_DEVICE),
        ("demix_device one channel, no axis", lambda: PV1.demix_device(fr(None), fr(None), fr(None), (0, 1), 8, az_out=z(F, 17),
                                                                       stream=0), NO_DEVICE),
        ("demix_device float64 out", lambda: PV.demix_device(fr(), fr(), fr(dt=f64), (0, 1), 8, stream=0), INVALID),
        ("demix_device other F", lambda: PV.demix_device(fr(), fr(f=F + 1), fr(), (0, 1), 8, stream=0), INVALID),
        ("demix_device one number", lambda: PV.demix_device(fr(), fr(), fr(), 0.5, 8, stream=0), INVALID),
        ("demix_device rows of one column", lambda: PV.demix_device(fr(), fr(), fr(), z(F, 1), 8, stream=0), INVALID),
        ("demix_device rows float64", lambda: PV.demix_device(fr(), fr(), fr(), z(F, 2, dt=f64), 8, stream=0), INVALID),
        ("demix_device rows strided", lambda: PV.demix_device(fr(), fr(), fr(), strided(z(F, 2)), 8, stream=0), INVALID),
        ("demix_device az_out of other points",
         lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 8, az_out=z(2, F, 16), stream=0), INVALID),
        ("demix_device az_out float64",
         lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 8, az_out=z(2, F, 17, dt=f64), stream=0), INVALID),
        ("demix_device az_out without axis, two channels",
         lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 8, az_out=z(F, 17), stream=0), INVALID),
        ("demix_device az_out strided",
         lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 8, az_out=strided(z(2, F, 17)), stream=0), INVALID),
        ("demix_device no points", lambda: PV.demix_device(fr(), fr(), fr(), (0, 1), 0, stream=0), INVALID),
        ("demix", lambda: PV.demix(nfr(), nfr(), 0.25, 3, 8), host(NO_DEVICE)),
        ("demix with the profile", lambda: PV.demix(nfr(), nfr(), np.zeros(F), np.full(F, 17.0), 8, az=True), host(NO_DEVICE)),
        ("demix width too large", lambda: PV.demix(nfr(), nfr(), 0, 18, 8), host(INVALID)),
        ("demix no axis, two channels", lambda: PV.demix(nfr(None), nfr(None), 0, 1, 8),
         (ValueError, "frames must be (2, F, %d, 2)" % (M + 1))),
    ]


@pytest.mark.skipif(fa.device_count() > 0, reason="a HIP device is present: these calls would hand host addresses to a kernel")
def test_the_python_layers_rows():
    """CPU tensors and stream=0 on objects that found no device: a call the layer accepts returns the library's answer
    (-1, before it touches memory), one it refuses returns -30 or raises; and both forms are reached"""
    rows = _demix_rows()
    assert len({r[0] for r in rows}) == len(rows)
    for what, call, outcome in rows:
        try:
            got = call()
        except ValueError as e:
            got = (ValueError, str(e))
        except fa.ClError as e:
            got = (fa.ClError, e.code)
        assert got == outcome, what
    reached = {r[0].split()[0] for r in rows if r[2] in (-1, (fa.ClError, -1))}
    assert {"demix_device", "demix"} <= reached
