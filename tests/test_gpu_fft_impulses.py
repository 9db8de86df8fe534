"""Per-bin GPU tests of every FFT route: impulse families against exact float64 (tests/fft_exact.py), a poisoned
neighbour, and guard bands around the buffers.

The dense-noise tests of tests/test_gpu_fft.py accept relL2 <= 1e-6: one twiddle entry off by eps moves that norm by about
eps / sqrt(n).  A delta at j transforms to a w^(jk) (/ n): every bin has the same magnitude, max|err| / max|ref| is the worst
single bin, and each bin is one product of table entries — so the same bar (TOL of SURVEY.md section 8d, which the
reference's own float32 arithmetic meets on these inputs: tests/test_fft_exact_cpu.py) now holds per table entry.  Every
transform of every batch is compared.  Each case prints `IMPULSE <route> n=<n> batch=<b> fwd/inv worst-bin <e>`; the lines of
one run are profiles/fft_impulses.txt.
"""
import numpy as np
import pytest

import opencl_fft_amd as fa
from tests import fft_exact as fx
from tests.gpu_guard import flat
from tests.util import TOL, rel_err

pytestmark = pytest.mark.gpu

AMP = 1 - 0.5j          # both components of a complex delta / bin
RAMP = 0.75             # real deltas


def _plan(real, n, fwd):
    p = (fa.Clrfft if real else fa.Clcfft)(0, n, fwd)
    assert p.get_error() == 0, p.get_log()
    return p


def _sync():
    import torch
    torch.cuda.synchronize()


def _deltas(rows, width, js, amp):
    """(rows, width) complex (as (rows, width, 2) float32) or real zeros on the device with amp scattered at [r, js[r]]"""
    import torch
    r = torch.arange(rows, device="cuda")
    j = torch.from_numpy(np.asarray(js, dtype=np.int64)).cuda()
    if isinstance(amp, complex):
        x = torch.zeros((rows, width, 2), device="cuda")
        x[r, j, 0], x[r, j, 1] = amp.real, amp.imag
    else:
        x = torch.zeros((rows, width), device="cuda")
        x[r, j] = amp
    return x


def _run(plan, x, group=None, oop=False):
    """exec on the whole batch (group None) or in launches of at most `group` transforms (the few-transform routes)"""
    import torch
    rows = x.shape[0]
    y = torch.full_like(x, float("nan")) if oop else x
    for lo in range(0, rows, group or rows):
        hi = min(rows, lo + (group or rows))
        if oop:
            assert plan.exec_device_oop(x[lo:hi], y[lo:hi], hi - lo) == 0
        else:
            assert plan.exec_device(x[lo:hi], hi - lo) == 0
    _sync()
    return y


def _worst(y, chunks, as_complex):
    """(worst relL2, worst max / max) of device rows against the float64 chunks: the criterion of util.assert_parity, per
    chunk of at most 64 MiB of reference (every row has the same magnitude, so chunks check no less than the whole)"""
    l2w = mxw = 0.0
    for lo, hi, want in chunks:
        got = y[lo:hi].cpu().numpy().reshape(hi - lo, -1)
        if as_complex:
            got = got.view(np.complex64)
        l2, mx = rel_err(got, want)
        l2w, mxw = max(l2w, l2), max(mxw, mx)
    return l2w, mxw


# Every route, also those outside the reference's range (n > 65536, Bluestein, real sizes above 131072), measured inside
# TOL on these inputs (profiles/fft_impulses.txt: worst 7.9e-7, real size 65536 forward; the Bluestein routes beside their
# float32 model, fft_exact.bluestein_f32): no case carries a bound of its own.
def _report(route, n, batch, fwd, l2, mx, model=None):
    print("IMPULSE %s n=%d batch=%d %s worst-bin %.3g%s" % (route, n, batch, "fwd" if fwd else "inv", mx,
                                                            "" if model is None else " model %.3g" % model))
    assert l2 <= TOL and mx <= TOL, "%s n=%d batch=%d fwd=%s: relL2=%.3g max/max=%.3g (tol %.1g)" % (route, n, batch, fwd, l2, mx, TOL)


# ---- (a) impulse families ---------------------------------------------------------------------------------------------------

def _big_family(n, row):
    """j < 64 plus the powers of two times the row length of the two-pass split (72 positions)"""
    return np.unique(np.concatenate([np.arange(64), row << np.arange(8)])).astype(np.int64)


C2C = [("k_fft_tiny", 2, None, None), ("k_fft_tiny", 4, None, None)]
C2C += [("k_fft_small" if n <= 64 else "k_fft_lds", n, None, None) for n in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192)]
C2C += [("spread", 16384, None, 3), ("k_cfft_2x", 16384, None, None),
        ("spread", 32768, None, 3), ("k_fft_4step", 32768, None, None),
        ("spread", 65536, None, 3),
        ("k_big2_cols", 1 << 17, "big", None), ("k_big2_cols", 1 << 19, "big", None), ("k_big_cols", 1 << 23, "big3", None)]


@pytest.mark.parametrize("route,n,family,group", C2C, ids=["%s-%d" % (c[0], c[1]) for c in C2C])
def test_c2c_impulses(route, n, family, group):
    """spread: the column / row kernel pair a batch of up to CUs / 4 transforms takes — the family runs three transforms per
    launch; the other routes take the whole family in one launch (more than CUs / 4 transforms for n >= 16384)"""
    if family == "big":
        js = _big_family(n, 1 << (n.bit_length() - 1 - (n.bit_length() - 1) // 2))     # n = N1 x N2, rows of N2 = 2^(logn - logn / 2)
    elif family == "big3":
        js = np.array([0, 1, 1 << 11, 1 << 12, (1 << 22) + 1, n - 1], dtype=np.int64)
    else:
        js = fx.impulse_positions(n)
    assert group is not None or n < 16384 or n > 65536 or js.size >= 70
    for fwd in (True, False):
        plan = _plan(False, n, fwd)
        if route != "spread":
            assert plan.kernel_name() == route
        y = _run(plan, _deltas(js.size, n, js, AMP), group)
        l2, mx = _worst(y, fx.cfft_impulse_chunks(n, js, fwd, AMP), True)
        _report(route, n, group or js.size, fwd, l2, mx)


def test_c2c_impulses_resident_65536_in_and_out_of_place():
    """the full 513-position family on k_fft_res16, in place and src -> dst: the same bits, and every bin of both"""
    import torch
    n = 65536
    js = fx.impulse_positions(n)
    assert js.size == 513
    for fwd in (True, False):
        plan = _plan(False, n, fwd)
        assert plan.kernel_name() == "k_fft_res16"
        x = _deltas(js.size, n, js, AMP)
        y = _run(plan, x, oop=True)
        assert int((x != 0).sum()) == 2 * js.size, "source modified"
        z = _run(plan, x)
        assert torch.equal(y.view(torch.int32), z.view(torch.int32)), "out of place and in place differ"
        del x, z
        l2, mx = _worst(y, fx.cfft_impulse_chunks(n, js, fwd, AMP), True)
        _report("k_fft_res16", n, js.size, fwd, l2, mx)


@pytest.mark.parametrize("n,cap", [(3, None), (100, 300), (1000, 300), (4095, 300), (44100, 4)])
def test_any_length_impulses(n, cap):
    """Bluestein's algorithm (k_blue_lds: one launch; "bluestein": composed of two power-of-two plans), with the float32
    model's worst bin beside the kernel's where the model applies (convolution length <= 65536)"""
    js = fx.impulse_positions(n, cap)
    m = 1 << int(np.ceil(np.log2(2 * n - 1)))
    route = "k_blue_lds" if 256 <= m <= 8192 else "bluestein"
    for fwd in (True, False):
        plan = _plan(False, n, fwd)
        assert plan.kernel_name() == route
        x = _deltas(js.size, n, js, AMP)
        host = x.cpu().numpy().view(np.complex64).reshape(js.size, n)
        y = _run(plan, x)
        want = fx.cfft_impulses(n, js, fwd, AMP)
        l2, mx = _worst(y, [(0, js.size, want)], True)
        model = rel_err(fx.bluestein_f32(host, n, fwd), want)[1] if m <= 65536 else None
        _report(route, n, js.size, fwd, l2, mx, model)


REAL = [("k_fft_lds", 4, None, None), ("k_fft_lds", 64, None, None), ("k_fft_lds", 1024, None, None),
        ("k_fft_lds", 8192, None, None), ("k_fft_lds", 16384, None, None),
        ("spread", 32768, None, 3), ("k_rfft_2x", 32768, None, None), ("spread", 65536, None, 3), ("k_rfft_2x", 65536, None, None),
        ("spread", 131072, None, 3), ("k_fft_res16", 131072, None, None),
        ("k_blue_lds", 1000, None, None), ("k_big2_cols", 1 << 19, 72, None)]


@pytest.mark.parametrize("route,size,cap,group", REAL, ids=["%s-%d" % (c[0], c[1]) for c in REAL])
def test_real_impulses(route, size, cap, group):
    """packed real plans: forward of real deltas, inverse of single-bin spectra (bin 0's two halves and the un-conjugated
    bin M/2 among them); spread = the complex column / row pair plus the pack kernel, three transforms per launch"""
    m = size // 2
    js, ks = fx.real_positions(size, cap), fx.real_bins(size, cap)
    f, i = _plan(True, size, True), _plan(True, size, False)
    if route in ("k_rfft_2x", "k_fft_res16", "k_blue_lds", "k_big2_cols"):
        assert f.kernel_name() == route and i.kernel_name() == route
        assert group is not None or size in (1000, 1 << 19) or min(js.size, ks.size) >= 70
    y = _run(f, _deltas(js.size, size, js, RAMP), group)
    l2, mx = _worst(y, fx.rfft_impulse_chunks(size, js, RAMP), True)
    _report("real " + route, size, group or js.size, True, l2, mx)
    y = _run(i, _deltas(ks.size, m, ks, AMP).view(ks.size, size), group)
    l2, mx = _worst(y, fx.irfft_single_bin_chunks(size, ks, AMP), False)
    _report("real " + route, size, group or ks.size, False, l2, mx)


# ---- (b), (c): the routes at their smallest batch of several transforms per workgroup or launch -------------------------------------

ROUTES = [(False, 2, 257, "k_fft_tiny"), (False, 4, 257, "k_fft_tiny"), (False, 8, 333, "k_fft_small"), (False, 64, 37, "k_fft_small"),
          (False, 1024, 9, "k_fft_lds"), (False, 8192, 3, "k_fft_lds"), (False, 16384, 3, None), (False, 16384, 70, "k_cfft_2x"),
          (False, 32768, 3, None), (False, 32768, 70, "k_fft_4step"), (False, 65536, 3, None), (False, 65536, 70, "k_fft_res16"),
          (False, 1 << 17, 3, "k_big2_cols"), (False, 1 << 23, 2, "k_big_cols"),
          (False, 100, 37, "k_blue_lds"), (False, 3, 7, "bluestein"), (False, 44100, 2, "bluestein"),
          (True, 4, 777, None), (True, 64, 130, "k_fft_small"), (True, 1024, 9, "k_fft_lds"), (True, 8192, 37, "k_fft_lds"),
          (True, 16384, 11, "k_fft_lds"), (True, 32768, 3, None), (True, 32768, 70, "k_rfft_2x"), (True, 65536, 3, None),
          (True, 65536, 70, "k_rfft_2x"), (True, 131072, 3, None), (True, 131072, 70, "k_fft_res16"), (True, 1000, 7, "k_blue_lds"),
          (True, 1 << 19, 2, "k_big2_cols")]
ROUTE_IDS = ["%s-%d-%d" % ("real" if r[0] else "c2c", r[1], r[2]) for r in ROUTES]


def _noise(real, n, batch, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((batch, n) if real else (batch, n, 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1


@pytest.mark.parametrize("real,n,batch,kernel", ROUTES, ids=ROUTE_IDS)
def test_poisoned_neighbour(real, n, batch, kernel):
    """one transform of the batch replaced by NaN: it comes out all NaN, and every other transform keeps its bits — no value
    of one transform reaches another (shared workgroups, lane pairs, staging rows, workspaces)"""
    import torch
    for fwd in (True, False):
        plan = _plan(real, n, fwd)
        if kernel:
            assert plan.kernel_name() == kernel
        x = _noise(real, n, batch, n + batch)
        base = x.clone()
        assert plan.exec_device(base, batch) == 0
        _sync()
        assert not torch.isnan(base).any()
        for bs in sorted({0, batch // 2, batch - 1}):
            y = x.clone()
            y[bs] = float("nan")
            assert plan.exec_device(y, batch) == 0
            _sync()
            assert bool(torch.isnan(y[bs]).all()), "transform %d is not all NaN (fwd=%s)" % (bs, fwd)
            y[bs] = base[bs]
            assert torch.equal(y.view(torch.int32), base.view(torch.int32)), "NaN of transform %d reached a neighbour (fwd=%s)" % (bs, fwd)


@pytest.mark.parametrize("misalign", [2, 0], ids=["align8", "align16"])
@pytest.mark.parametrize("real,n,batch,kernel", ROUTES, ids=ROUTE_IDS)
def test_guard_bands(real, n, batch, kernel, misalign):
    """the batch in the middle of a buffer of canaries, at the least alignment include/clfft_amd.h asks for (8 bytes, complex
    and real plans alike) and at 16: nothing before or behind the data changes, in place and out of place; out of place the
    source keeps its bits and the destination is written completely, with the bits of the in-place call"""
    import torch
    nf = batch * n * (1 if real else 2)
    for fwd in (True, False):
        plan = _plan(real, n, fwd)
        x = _noise(real, n, batch, 7 * n + batch).reshape(-1)
        plain = x.clone()
        assert plan.exec_device(plain, batch) == 0
        g = flat((nf,), misalign=misalign)
        data = g.data
        data.copy_(x)
        assert plan.exec_device(data, batch) == 0
        _sync()
        assert g.intact(), "in place: wrote outside the batch (fwd=%s)" % fwd
        scale = float(plain.abs().max())
        assert float((data - plain).abs().max()) <= 1e-6 * scale, "in place: result differs from the aligned call"
        sg, dg = flat((nf,), misalign=misalign), flat((nf,), misalign=misalign)
        src, dst = sg.data, dg.data
        src.copy_(x)
        assert plan.exec_device_oop(src, dst, batch) == 0
        _sync()
        assert sg.intact() and dg.intact(), "out of place: wrote outside the batch (fwd=%s)" % fwd
        assert torch.equal(src.view(torch.int32), x.view(torch.int32)), "source modified (fwd=%s)" % fwd
        assert not dg.unwritten(), "destination not written completely (fwd=%s)" % fwd
        assert torch.equal(dst.view(torch.int32), data.view(torch.int32)), "out of place differs from in place (fwd=%s)" % fwd
