"""The one-stream shaping operations of clfa_pvoc on the device (pvoc_shape.hip: k_pvoc_shape, k_pvoc_lock, k_pvoc_warp)
against the numpy restatement of their definitions (tests/pvoc_shape_model.py).

Band, mask, stencil, arp and lock are bit-equal with the float32 model: every operation of theirs is a single correctly
rounded float32 step, the band's division included (where the model gives a NaN the device gives a NaN; payloads are not
compared).  The warp's freq column and every copied bin are bit-equal with the input; its amps go through logf, two LDS
transforms and expf, which are not numpy's, so the contract is the one of tests/test_gpu_pvoc_ops.py and
tests/test_gpu_pvoc_pair.py: the relative L2 error of the amps against the float64 model is at most MARGIN times the
float32 model's own error on the same inputs.

MARGIN.  The rule: the smallest of 2, 4, 8 that clears the largest ratio measured over every case of this file by a factor
1.5.  Every case prints its ratio (`PVOCSHAPE ...` lines, pytest -s).
MEASURED over every case of this file on an MI355X (56 ratios): they lie between 0.31 and 1.84.  With lowest_bin = 1 the
device's error is 7.2e-8 .. 7.0e-7 on analysed frames against the model's 7.0e-8 .. 7.2e-7, and 9.5e-8 .. 1.3e-6 on the
tilted raw frames against 5.1e-8 .. 1.7e-6; with lowest_bin = M - 1 a call computes one bin per frame and both errors,
taken over the whole array, are 3e-11 .. 1.2e-7.  The largest ratios: 1.84 (size 64, 100 tilted frames of one channel,
coefs 1: 9.46e-8 against 5.14e-8), 1.78 (size 1024, lowest_bin and coefs 511: 3.18e-9 against 1.78e-9) and 1.75 (size
16384, coefs 80).  1.84 x 1.5 = 2.8 rules out 2, so MARGIN is 4.

The sample matters.  The L2 norm of a tilted frame is carried by the two or three bins at the top of its slope, so a call
of a few such frames measures a dozen values, and the float32 model's own error on a dozen values is no yardstick: a first
version of this file ran 1 channel x 5 frames at size 64, where the tilted frames with coefs 1 gave 1.92e-7 against a
model error of 1.77e-8 — less than the 6e-8 of a single float32 rounding — a ratio of 10.86, while the same rows on
3 x 129 frames gave 1.56e-7 against 1.11e-7.  The device's figure was the ordinary one in both; the group that is live
only in part is now 1 x 100 frames (of the 128 a workgroup holds), and the ratios above are those of the file as it is.
"""
import numpy as np
import pytest
import torch

from opencl_fft_amd import _lib
from tests import pvoc_ops_model as om
from tests import pvoc_shape_model as sm
from tests.gpu_guard import CANARY, DEV, bits, dev, flat, run, same
from tests.pvoc_inputs import SR, analysed, make_pvoc
from tests.pvoc_inputs import raw_freq_first as raw     # freqs drawn first, NaN amps and freqs among the plain frames

pytestmark = pytest.mark.gpu
MARGIN = 4.0            # see the docstring: the largest ratio measured is 1.84
CL_INVALID_VALUE = -30
f32 = np.float32
RATIO = {"max": 0.0}
NAMES = ("band", "mask", "stencil", "arp", "lock", "warp")


def fpw(size):
    """frames per workgroup of k_pvoc_warp (LdsGeom: 16 points per lane, at least 256 lanes)"""
    t = max(size // 2 // 16, 1)
    return max(t, 256) // t


def make(size, channels=1, hop=None, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, hop or size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert [pv.shape_kernel_name(op) for op in NAMES] == ["k_pvoc_shape"] * 4 + ["k_pvoc_lock", "k_pvoc_warp"]
    return pv


def chunks(pool, F):
    """the rows of `pool` (n, 4) as calls of F rows each, the last one filled up from the start of the pool"""
    pool = np.asarray(pool, f32)
    out = []
    for i in range(0, len(pool), F):
        out.append(np.ascontiguousarray(np.take(pool, np.arange(i, i + F) % len(pool), axis=0)))
    return out


def cols(r, n):
    """the first n columns of the rows as device tensors (F,)"""
    return [dev(r[:, i]) for i in range(n)]


def table_of(size, seed=0):
    """a table over the bins: positive values over six decades, a zero and a NaN"""
    t = (10.0 ** np.random.default_rng(size + seed).uniform(-3, 3, size // 2 + 1)).astype(f32)
    t[size // 8], t[size // 4 + 1] = 0, np.nan
    return t


def band_pools(a):
    """BAND rows for the frames a: the edges exactly on |freq| values of channel 0 (an x on each of the four edges), lc == lf
    and hf == hc, an invalid order, a NaN edge, a band wide open and one in the middle"""
    F = a.shape[1]
    on_x, closed = [], []
    for f in range(F):
        x = np.abs(a[0, f, :, 1])
        x = np.unique(x[np.isfinite(x)])
        e = x[[len(x) // 8, len(x) // 3, len(x) // 2, (3 * len(x)) // 4]]
        on_x.append(e)
        closed.append((e[0], e[0], e[3], e[3]))
    rest = [(300, 200, 3000, 4000), (100, np.nan, 3000, 4000), (0, 0, 3e38, 3e38), (1000, 5000, 9000, 20000),
            (np.nan, np.nan, np.nan, np.nan), (0, 0, 0, 0), (500, 500, 500, 30000), (100, 200, 3000, np.inf)]
    return [np.asarray(on_x, f32), np.asarray(closed, f32)] + chunks(rest, F)


MASK_POOL = [(v, 0, 0, 0) for v in (0.6, 0.0, 1.0, -0.5, np.nan, 1.5, 0.25, 2.0 ** -20)]
STENCIL_POOL = [(0.0, 1.0), (0.5, 0.0), (-2.0, 1e-3), (np.nan, 1.0), (0.25, np.nan), (3.0, 1e10), (0.0, -1.0), (1.0, np.inf)]
ARP_POOL = [(0.0, 1.0, 2.0), (1.0, 0.6, -0.5), (np.nan, 1.0, 3.0), (0.5, 0.0, 1.0), (0.37, np.nan, 0.0), (1.5, 0.25, np.nan),
            (-1.0, 2.0, 1.0), (0.999, 0.5, 1e-3)]
LOCK_POOL = [(1.0, 0.01), (0.0, 0.5), (1.0, 0.5), (np.nan, 0.3), (-3.0, 0.0), (1.0, 10.0), (0.0, 0.0), (2.0, np.nan)]


def check_shape_bits(pv, a, what):
    """band, mask, stencil, arp on the frames a: bit-equal with the float32 model, with per-frame arrays and with numbers"""
    size, F = pv.size, a.shape[1]
    da = dev(a)
    tab = table_of(size)
    dt = dev(tab)
    for r in band_pools(a):
        for reject in (False, True):
            got = run(lambda o: pv.band_device(da, o, *cols(r, 4), reject=reject), a.shape)
            same(got, sm.shape32(sm.BAND, a, r, size, SR, reject=reject), "%s: band reject %d" % (what, reject))
    got = run(lambda o: pv.band_device(da, o, 400.0, 2500.0, 2500.0, 11000.0, reject=True), a.shape)
    same(got, sm.shape32(sm.BAND, a, sm.rows(F, 400, 2500, 2500, 11000), size, SR, reject=True), what + ": band by numbers")
    for r in chunks(MASK_POOL, F):
        got = run(lambda o: pv.mask_device(da, o, dt, *cols(r, 1)), a.shape)
        same(got, sm.shape32(sm.MASK, a, r, size, SR, tab), what + ": mask")
    got = run(lambda o: pv.mask_device(da, o, dt, 0.7), a.shape)
    same(got, sm.shape32(sm.MASK, a, sm.rows(F, 0.7), size, SR, tab), what + ": mask by numbers")
    for r in chunks([v + (0, 0) for v in STENCIL_POOL], F):
        got = run(lambda o: pv.stencil_device(da, o, dt, *cols(r, 2)), a.shape)
        same(got, sm.shape32(sm.STENCIL, a, r, size, SR, tab), what + ": stencil")
    got = run(lambda o: pv.stencil_device(da, o, dt, 0.1, 2.0), a.shape)
    same(got, sm.shape32(sm.STENCIL, a, sm.rows(F, 0.1, 2.0), size, SR, tab), what + ": stencil by numbers")
    for r in chunks([v + (0,) for v in ARP_POOL], F):
        got = run(lambda o: pv.arp_device(da, o, *cols(r, 3)), a.shape)
        same(got, sm.shape32(sm.ARP, a, r, size, SR), what + ": arp")
    got = run(lambda o: pv.arp_device(da, o, 0.3, 0.9, 2.0), a.shape)
    same(got, sm.shape32(sm.ARP, a, sm.rows(F, 0.3, 0.9, 2.0), size, SR), what + ": arp by numbers")


# size 512: M + 1 = 257 bins, two tiles, the second with one live lane
SHAPES = [(64, 1, 3), (512, 2, 5), (16384, 1, 2)]


@pytest.mark.parametrize("grid_max", [None, 2])
@pytest.mark.parametrize("size,channels,F", SHAPES)
def test_band_mask_stencil_arp_are_the_models_bits(size, channels, F, grid_max, monkeypatch):
    pv = make(size, channels, grid_max=grid_max, monkeypatch=monkeypatch)
    check_shape_bits(pv, raw(size, channels, F, 4), "size %d ch %d F %d raw" % (size, channels, F))
    check_shape_bits(pv, analysed(size, channels, F, 3), "size %d ch %d F %d analysed" % (size, channels, F))


def check_lock(pv, a, what, pool=LOCK_POOL):
    """the lock on the frames a: bit-equal with the float32 model; returns how many freqs changed"""
    size, F = pv.size, a.shape[1]
    da = dev(a)
    changed = 0
    for r in chunks([v + (0, 0) for v in pool], F):
        got = run(lambda o: pv.lock_device(da, o, *cols(r, 2)), a.shape)
        want = sm.shape32(sm.LOCK, a, r, size, SR)
        same(got, want, what + ": lock")
        changed += int((bits(want[..., 1]) != bits(a[..., 1])).sum())
    got = run(lambda o: pv.lock_device(da, o), a.shape)
    same(got, sm.shape32(sm.LOCK, a, sm.rows(F, 1.0, 0.01), size, SR), what + ": lock by default")
    return changed


@pytest.mark.parametrize("grid_max", [None, 2])
@pytest.mark.parametrize("size,channels,F", SHAPES)
def test_lock_is_the_models_bits(size, channels, F, grid_max, monkeypatch):
    pv = make(size, channels, grid_max=grid_max, monkeypatch=monkeypatch)
    check_lock(pv, raw(size, channels, F, 4), "size %d ch %d F %d raw" % (size, channels, F))
    a = analysed(size, channels, max(F, 3), 3)
    changed = check_lock(pv, a, "size %d ch %d analysed" % (size, channels), [(1.0, 0.5), (1.0, 0.01), (1.0, 10.0)])
    assert changed > 0, "no freq was locked: the test would pass on a copy"


def planted(size, C, F, seed):
    """frames with peaks planted where the halo of k_pvoc_lock crosses the tile boundaries (256 bins a tile), at the first
    and the last bin that can be a peak, and in the bins beside those, which cannot; freqs near the bin centres"""
    B = size // 2 + 1
    M = B - 1
    rng = np.random.default_rng(seed)
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32) + f32(0.01)
    freq = (np.arange(B) * (SR / size) + rng.standard_normal((C, F, B)) * SR / size / 4).astype(f32)
    plan = [(2, M - 2, 254, 257), (255, 258, M - 1), (256, M, 1), (254, 257, 2), (253, 256, 259, M - 2)]
    for f in range(F):
        for k in plan[f % len(plan)]:
            amp[:, f, k] = 100 + k
    return np.stack([amp, freq], axis=-1), plan


@pytest.mark.parametrize("grid_max", [None, 2])
def test_lock_across_the_tile_boundaries(grid_max, monkeypatch):
    size, C, F = 1024, 2, 5
    M = size // 2
    assert M + 1 == 513
    pv = make(size, C, grid_max=grid_max, monkeypatch=monkeypatch)
    a, plan = planted(size, C, F, 9)
    pk = sm.peaks(a[..., 0])
    for f in range(F):
        for k in plan[f]:
            assert pk[:, f, k].all() == (2 <= k <= M - 2), (f, k)
    changed = check_lock(pv, a, "size 1024 planted", [(1.0, 0.5), (1.0, 0.5), (0.0, 0.5), (np.nan, 0.5), (1.0, 0.0)])
    assert changed > 0
    # every planted peak hands its freq to both neighbours at a tolerance this wide: the bins on the other side of a tile
    # boundary among them (255 | 256, 511 | 512)
    r = sm.rows(F, 1.0, 10.0)
    got = run(lambda o: pv.lock_device(dev(a), o, 1.0, 10.0), a.shape)
    same(got, sm.shape32(sm.LOCK, a, r, size, SR), "size 1024 planted, wide")
    for f in range(F):
        for k in plan[f]:
            if 2 <= k <= M - 2:
                for nb in (k - 1, k + 1):
                    assert np.array_equal(bits(got[:, f, nb, 1]), bits(a[:, f, k, 1])), (f, k, nb)
    assert np.array_equal(bits(got[..., 0]), bits(a[..., 0]))
    assert np.array_equal(bits(got[:, :, [0, M]]), bits(a[:, :, [0, M]]))


def warp_pool(size):
    """WARP rows: s of 0.25, 1, 1.37 and 4; shifts of 0, +-3.4 bins and past every bin; an s out of range and a NaN s"""
    b = 3.4 * SR / size
    pool = [(0.25, 0.0, 1.0), (1.0, 0.0, 1.0), (1.37, b, -0.8), (4.0, -b, 1.1), (1.37, 2 * SR, 1.0), (5.0, 0.0, 2.0),
            (np.nan, 0.0, 1.0), (1.0, b, 1.0), (0.25, -b, 0.5), (4.0, 0.0, 1.0), (1.37, 0.0, 1.0), (0.8, -b, 1.0)]
    return [v + (0.0,) for v in pool]


def check_warp(pv, a, r, lowest, coefs, what):
    """freq and every copied bin bit-equal with the input, amps within MARGIN of the float32 model's error against float64"""
    size = pv.size
    M = size // 2
    da = dev(a)
    sc, sh, gn = cols(r, 3)
    got = run(lambda o: pv.warp_device(da, o, sc, sh, lowest_bin=lowest, gain=gn, coefs=coefs), a.shape)
    m32 = sm.shape32(sm.WARP, a, r, size, SR, lowest=lowest, coefs=coefs)
    m64 = sm.warp64_amps(a, r, size, SR, lowest, coefs)
    assert np.isfinite(m32).all() and np.isfinite(m64).all(), "the inputs overflow the model"
    assert np.array_equal(bits(got[..., 1]), bits(a[..., 1])), what + ": freq"
    copied = np.r_[0:lowest, M]
    assert np.array_equal(bits(got[:, :, copied]), bits(a[:, :, copied])), what + ": the copied bins"
    plain = ~((r[:, 0] >= 0.25) & (r[:, 0] <= 4) & (np.abs(r[:, 1] * om.bpf_of(size, SR)) <= M))
    assert np.array_equal(bits(got[:, plain]), bits(m32[:, plain])), what + ": the frames of plain gain"
    e_dev, e_f32 = om.rel_l2(got[..., 0], m64), om.rel_l2(m32[..., 0], m64)
    ratio = e_dev / max(e_f32, 1e-300)
    RATIO["max"] = max(RATIO["max"], ratio)
    print("PVOCSHAPE %s lowest %d coefs %d: amps relL2 %.3g (float32 model %.3g, ratio %.2f; largest so far %.2f)"
          % (what, lowest, coefs, e_dev, e_f32, ratio, RATIO["max"]))
    assert e_dev <= MARGIN * e_f32, "%s: %.3g against %.3g" % (what, e_dev, e_f32)
    return got


def warp_cases(pv, C, F, what):
    size = pv.size
    M = size // 2
    pool = chunks(warp_pool(size), F)
    for kind, a in (("analysed", analysed(size, C, F, 3)), ("tilted", raw(size, C, F, 5, tilt=True))):
        for i, coefs in enumerate(sorted({1, min(80, M - 1), M - 1})):
            for j, r in enumerate(pool):
                check_warp(pv, a, r, 1, coefs, "%s %s rows %d" % (what, kind, j))
            check_warp(pv, a, pool[i % len(pool)], M - 1, coefs, "%s %s" % (what, kind))
        check_warp(pv, a, pool[0], 3, min(24, M - 1), "%s %s" % (what, kind))


@pytest.mark.parametrize("size,channels,F", [(64, 1, 100), (64, 3, 129), (1024, 3, 9)])
def test_warp_accuracy(size, channels, F, monkeypatch):
    """channels x F is no multiple of the frames a workgroup holds (128 at size 64, 8 at size 1024): a ragged last group,
    at size 64 once as the only group and once after three full ones"""
    assert (channels * F) % fpw(size) != 0
    pv = make(size, channels)
    warp_cases(pv, channels, F, "size %d ch %d F %d" % (size, channels, F))
    small = make(size, channels, grid_max=2, monkeypatch=monkeypatch)
    M = size // 2
    a, r = analysed(size, channels, F, 3), chunks(warp_pool(size), F)[0]
    whole = check_warp(pv, a, r, 2, min(24, M - 1), "size %d ch %d F %d" % (size, channels, F))
    capped = check_warp(small, a, r, 2, min(24, M - 1), "size %d ch %d F %d grid of 2" % (size, channels, F))
    assert np.array_equal(bits(whole), bits(capped)), "the grid cap changed the result"


def test_warp_size_16384_once(monkeypatch):
    """the tables-from-cache route of k_pvoc_warp: one frame per workgroup; also under a grid cap of 2"""
    size, C, F = 16384, 1, 3
    M = size // 2
    pv, small = make(size, C), make(size, C, grid_max=2, monkeypatch=monkeypatch)
    pool = chunks(warp_pool(size), F)
    a, t = analysed(size, C, F, 3), raw(size, C, F, 5, tilt=True)
    for j, r in enumerate(pool):
        check_warp(pv, a, r, 1, 80, "size 16384 analysed rows %d" % j)
    check_warp(pv, t, pool[0], 1, 40, "size 16384 tilted")
    check_warp(pv, t, pool[1], 1, 1, "size 16384 tilted")
    check_warp(pv, a, pool[2], 1, M - 1, "size 16384 analysed")
    check_warp(pv, a, pool[0], M - 1, 80, "size 16384 analysed")
    whole = check_warp(pv, t, pool[3], 7, 80, "size 16384 tilted")
    capped = check_warp(small, t, pool[3], 7, 80, "size 16384 tilted grid of 2")
    assert np.array_equal(bits(whole), bits(capped)), "the grid cap changed the result"


def _all_calls(pv, tab):
    """one device call per op: (name, call(frames_in, frames_out, rows), rows of F frames for the blocking form's ranges,
    the blocking form)"""
    def rows_of(F, seed):
        rng = np.random.default_rng(seed)
        u = lambda lo, hi: rng.uniform(lo, hi, F).astype(f32)
        return {"band": sm.rows(F, u(0, 500), u(500, 2000), u(2000, 9000), u(9000, 20000)), "mask": sm.rows(F, u(0, 1)),
                "stencil": sm.rows(F, u(0, 1), u(0, 2)), "arp": sm.rows(F, u(0, 1), u(0, 1), u(0, 2)),
                "lock": sm.rows(F, (np.arange(F) % 3 != 1).astype(f32), u(0, 1)),
                "warp": sm.rows(F, u(0.25, 4), u(-2000, 2000), u(0.5, 2))}
    dev_calls = {
        "band": lambda x, o, r, **kw: pv.band_device(x, o, *cols(r, 4), reject=True, **kw),
        "mask": lambda x, o, r, **kw: pv.mask_device(x, o, tab, *cols(r, 1), **kw),
        "stencil": lambda x, o, r, **kw: pv.stencil_device(x, o, tab, *cols(r, 2), **kw),
        "arp": lambda x, o, r, **kw: pv.arp_device(x, o, *cols(r, 3), **kw),
        "lock": lambda x, o, r, **kw: pv.lock_device(x, o, *cols(r, 2), **kw),
        "warp": lambda x, o, r, **kw: pv.warp_device(x, o, r_col(r, 0), r_col(r, 1), 3, r_col(r, 2), 30, **kw)}
    host_calls = {
        "band": lambda x, r: pv.band(x, r[:, 0], r[:, 1], r[:, 2], r[:, 3], reject=True),
        "mask": lambda x, r: pv.mask(x, tab.cpu().numpy(), r[:, 0]),
        "stencil": lambda x, r: pv.stencil(x, tab.cpu().numpy(), r[:, 0], r[:, 1]),
        "arp": lambda x, r: pv.arp(x, r[:, 0], r[:, 1], r[:, 2]),
        "lock": lambda x, r: pv.lock(x, r[:, 0], r[:, 1]),
        "warp": lambda x, r: pv.warp(x, r[:, 0], r[:, 1], 3, r[:, 2], 30)}
    return rows_of, dev_calls, host_calls


def r_col(r, i):
    return dev(r[:, i])


def test_the_calls_are_stateless_splittable_and_repeatable():
    size, C, F = 1024, 2, 11
    M = size // 2
    pv = make(size, C)
    # states away from their initial values
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr = torch.zeros((C, F, M + 1, 2), device=DEV)
    sp = torch.zeros_like(spec)
    sig = torch.zeros((C, F * pv.hop), device=DEV)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0 and pv.adsyn_device(fr, sig) == 0
    assert pv.smooth_device(fr, torch.zeros_like(fr), 0.5, 0.5) == 0 and pv.freeze_device(fr, torch.zeros_like(fr), 0.0, 1.0) == 0
    torch.cuda.synchronize()

    def state():
        return (pv.read_prev(), pv.read_phase()) + tuple(pv.adsyn_state()) + (pv.time_state("smooth"), pv.time_state("freeze"))

    before = state()

    def unchanged():
        return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(state(), before))

    tab = dev(np.where(np.isnan(table_of(size)), f32(0.5), table_of(size)))
    rows_of, dev_calls, host_calls = _all_calls(pv, tab)
    rows = rows_of(F, 2)
    first = {}
    for name in NAMES:
        x, y = torch.zeros_like(fr), torch.zeros_like(fr)
        assert dev_calls[name](fr, x, rows[name]) == 0 and dev_calls[name](fr, y, rows[name]) == 0
        torch.cuda.synchronize()
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name + ": the same call twice"
        first[name] = x
    assert not torch.equal(first["lock"][..., 1].view(torch.int32), fr[..., 1].view(torch.int32)), "the lock locked nothing"
    # a call split into two calls
    cut = 4
    for name in NAMES:
        lo, hi = torch.zeros_like(fr[:, :cut]).contiguous(), torch.zeros_like(fr[:, cut:]).contiguous()
        assert dev_calls[name](fr[:, :cut].contiguous(), lo, rows[name][:cut]) == 0
        assert dev_calls[name](fr[:, cut:].contiguous(), hi, rows[name][cut:]) == 0
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([lo, hi], dim=1).view(torch.int32), first[name].view(torch.int32)), name + ": split"
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = {name: torch.zeros_like(fr) for name in NAMES}
    with torch.cuda.stream(side):
        for name in NAMES:
            assert dev_calls[name](fr, outs[name], rows[name]) == 0
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(first[name].view(torch.int32), outs[name].view(torch.int32)), name + ": side stream"
    # all six calls captured into one graph on one stream (none allocates), replayed
    outs = {name: torch.zeros_like(fr) for name in NAMES}
    held = {name: [dev(rows[name][:, i]) for i in range(4)] for name in NAMES}      # the per-frame tensors outlive the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.band_device(fr, outs["band"], *held["band"], reject=True) == 0
        assert pv.mask_device(fr, outs["mask"], tab, held["mask"][0]) == 0
        assert pv.stencil_device(fr, outs["stencil"], tab, *held["stencil"][:2]) == 0
        assert pv.arp_device(fr, outs["arp"], *held["arp"][:3]) == 0
        assert pv.lock_device(fr, outs["lock"], *held["lock"][:2]) == 0
        assert pv.warp_device(fr, outs["warp"], held["warp"][0], held["warp"][1], 3, held["warp"][2], 30) == 0
    for o in outs.values():
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for name in NAMES:
        assert torch.equal(first[name].view(torch.int32), outs[name].view(torch.int32)), name + ": graph replay"
    assert unchanged()
    # the blocking forms are the device forms
    ha = fr.cpu().numpy()
    for name in NAMES:
        h = host_calls[name](ha, rows[name])
        assert np.array_equal(bits(h), bits(first[name].cpu().numpy())), name + ": host form"
    assert unchanged()


def test_errors_write_nothing():
    size, C, F = 64, 2, 5
    M = size // 2
    pv = make(size, C)
    a = dev(analysed(size, C, F, 3))
    s = dev(np.full(F, 0.5, f32))
    tab = dev(np.full(M + 1, 0.5, f32))
    g = flat((C, F, M + 1, 2))
    out = g.data
    calls = [lambda x, o, p, t=tab: pv.band_device(x, o, p, p, p, p), lambda x, o, p, t=tab: pv.mask_device(x, o, t, p),
             lambda x, o, p, t=tab: pv.stencil_device(x, o, t, p, p), lambda x, o, p, t=tab: pv.arp_device(x, o, p, p, p),
             lambda x, o, p, t=tab: pv.lock_device(x, o, p, p), lambda x, o, p, t=tab: pv.warp_device(x, o, p, p, coefs=5)]
    L = _lib.lib()
    rows = dev(sm.rows(F, 0.5, 0.5, 0.5, 0.5))
    # an unknown op, bad flags, the warp's ranges
    for op in (-1, 6, 99):
        assert L.clfa_pvoc_shape_dev(pv._h, op, a.data_ptr(), out.data_ptr(), F, rows.data_ptr(), tab.data_ptr(), 0, 1, 5, None) \
            == CL_INVALID_VALUE
    for op, flags in ((0, 2), (0, 3), (1, 1), (4, 1), (5, 1)):
        assert L.clfa_pvoc_shape_dev(pv._h, op, a.data_ptr(), out.data_ptr(), F, rows.data_ptr(), tab.data_ptr(), flags, 1, 5,
                                     None) == CL_INVALID_VALUE
    assert L.clfa_pvoc_shape_dev(pv._h, 1, a.data_ptr(), out.data_ptr(), F, rows.data_ptr(), None, 0, 1, 5, None) == CL_INVALID_VALUE
    for coefs in (0, M, -3):
        assert pv.warp_device(a, out, 1.0, coefs=coefs) == CL_INVALID_VALUE
    for lowest in (0, M, -1):
        assert pv.warp_device(a, out, 1.0, lowest_bin=lowest, coefs=5) == CL_INVALID_VALUE
    # shapes, dtypes, strides
    for call in calls:
        assert call(a[:, :4].contiguous(), out, s) == CL_INVALID_VALUE
        assert call(a, out, s[:4].contiguous()) == CL_INVALID_VALUE
        assert call(a, out, s.double()) == CL_INVALID_VALUE
        assert call(a.double(), out, s) == CL_INVALID_VALUE
        assert call(a.transpose(0, 1), out, s) == CL_INVALID_VALUE
    assert pv.mask_device(a, out, tab[:-1].contiguous(), s) == CL_INVALID_VALUE
    assert pv.stencil_device(a, out, tab.double(), s, s) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert g.untouched()
    # an output overlapping the input or the table, shifted by one pair
    n = C * F * (M + 1) * 2
    buf = torch.full((2 * n + M + 1,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    lo, hi = buf[:n].view(C, F, M + 1, 2), buf[n - 2:2 * n - 2].view(C, F, M + 1, 2)
    tail = buf[2 * n - 4:2 * n - 4 + M + 1]
    for call in calls:
        assert call(lo, hi, s) == CL_INVALID_VALUE and call(hi, lo, s) == CL_INVALID_VALUE and call(lo, lo, s) == CL_INVALID_VALUE
    assert calls[1](a, hi, s, tail) == CL_INVALID_VALUE and calls[2](a, hi, s, tail) == CL_INVALID_VALUE
    # ... or the rows, by one element
    rbuf = torch.full((n + 4 * F,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    o2, r2 = rbuf[:n].view(C, F, M + 1, 2), rbuf[n - 1:n - 1 + 4 * F]
    for op in range(6):
        assert L.clfa_pvoc_shape_dev(pv._h, op, a.data_ptr(), o2.data_ptr(), F, r2.data_ptr(), tab.data_ptr(), 0, 1, 5, None) \
            == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == CANARY).all()) and bool((rbuf.view(torch.int32) == CANARY).all())
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, M + 1, 2), device=DEV)
    for call in calls:
        assert call(e, e.clone(), s[:0].contiguous()) == 0
    # and a good call still works: the lock of a frame with lock 0 is a copy
    assert pv.lock_device(a, out, 0.0) == 0
    torch.cuda.synchronize()
    assert g.intact() and np.array_equal(bits(out.cpu().numpy()), bits(a.cpu().numpy()))
