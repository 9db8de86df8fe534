"""The stereo demix of clfa_pvoc on the device (pvoc_demix.hip: k_pvoc_demix, k_pvoc_demix_az) against the numpy restatement
of its definition (tests/pvoc_demix_model.py), which does the scan over the gains literally.

Everything is compared bit for bit: every float32 operation of the definition is rounded on its own, so there is no
tolerance to choose.  The inputs are the model file's recipes and tests/pvoc_inputs.py's frames
(tests/test_pvoc_demix_cpu.py shows that gpu_cases notices twelve mutants of the model at every size run here).  Both
outputs lie in the guard bands of tests/gpu_guard.py: the frames 8-byte and not 16-byte aligned, the profile 4-byte and not
8-byte aligned."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard
from tests import pvoc_demix_model as dm
from tests.gpu_guard import CANARY, DEV, bits, dev, same
from tests.pvoc_inputs import SR, analysed, make_pvoc, raw
from tests.test_pvoc_demix_cpu import gpu_cases

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
f32 = np.float32
SIZES = (64, 128, 512, 2048, 16384)


def make(size, channels=1, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert pv.demix_kernel_name() == "k_pvoc_demix" and pv.demix_kernel_name(az=True) == "k_pvoc_demix_az"
    return pv


def run_guarded(pv, left, right, par, P, first=0, nbins=None, az=True, stream=None, same_buffer=False):
    """one device call into guarded outputs: (frames, profile or None) as numpy, the guard bands checked, every element
    written; par: a (pos, width) pair of numbers, or rows that go to the device"""
    dl = dev(left)
    dr = dl if same_buffer else dev(right)
    dp = par if isinstance(par, tuple) else dev(np.asarray(par, f32))
    out = gpu_guard.flat(left.shape, misalign=2)
    prof = gpu_guard.flat(left.shape[:2] + (2 * P + 1,), misalign=1) if az else None
    assert out.data.data_ptr() % 16 == 8 and (prof is None or prof.data.data_ptr() % 8 == 4)
    if stream is not None:
        torch.cuda.synchronize()          # the arrays above were filled on the current stream
    assert pv.demix_device(dl, dr, out.data, dp, P, first, nbins, az_out=prof.data if az else None, stream=stream) == 0
    torch.cuda.synchronize()
    for g, what in ((out, "the frames"), (prof, "the profile")):
        if g is not None:
            g.check_sides(what)
            assert not g.unwritten(), "an element of %s was not written" % what
    return out.data.cpu().numpy(), prof.data.cpu().numpy() if az else None


def check(pv, left, right, par, P, first, nbins, what, stream=None, without=True):
    """with the profile against the model, and without it the same frames"""
    what = "%s P %d range %d %s" % (what, P, first, nbins)
    rows = np.tile(np.array(par, f32), (left.shape[1], 1)) if isinstance(par, tuple) else par
    want, wprof = dm.demix(left, right, rows, P, first, nbins)
    got, prof = run_guarded(pv, left, right, par, P, first, nbins, True, stream)
    same(got, want, what)
    assert not np.isnan(wprof).any() and np.array_equal(bits(prof), bits(wprof)), what + ": the profile"
    if without:
        alone, _ = run_guarded(pv, left, right, par, P, first, nbins, False, stream)
        assert np.array_equal(bits(alone), bits(got)), what + ": the frames without the profile"


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_one_call_is_the_models_bits(size, channels):
    """the cases of the CPU test at 1, 5 and 37 frames; at 37 frames two unrelated streams of analysed and of raw frames
    besides, over the inner range"""
    pv = make(size, channels)
    B = size // 2 + 1
    for F in (1, 5, 37):
        for name, left, right, par, P, first, nbins in gpu_cases(size, channels, F):
            check(pv, left, right, par, P, first, nbins, "size %d ch %d F %d %s" % (size, channels, F, name))
    what = "size %d ch %d analysed against raw" % (size, channels)
    check(pv, analysed(size, channels, 37, 3), raw(size, channels, 37, 4), dm.par_rows(37, 8, 5), 8, 3, B - 5, what)
    check(pv, analysed(size, channels, 37, 3), analysed(size, channels, 37, 8), (0.37, 4.0), 8, 0, None, what + ", numbers")


@pytest.mark.parametrize("size", [256, 1024])
def test_the_sizes_between(size):
    """W = 128, and W = 256 with two rows"""
    C, F = 2, 12
    pv = make(size, C)
    for name, left, right, par, P, first, nbins in gpu_cases(size, C, F):
        check(pv, left, right, par, P, first, nbins, "size %d %s" % (size, name))


def test_the_most_points_and_the_edge_values_of_par():
    """P = 1024 at size 64; a NaN, infinities and values out of range in par, which the device form clamps"""
    size, C, F = 64, 2, 12
    pv = make(size, C)
    left, right, _ = dm.panned(size, C, F, 1024, 9)
    check(pv, left, right, dm.par_rows(F, 1024, 3), 1024, 0, None, "P 1024")
    check(pv, left, right, dm.par_rows(F, 1024, 7), 1024, 3, size // 2 + 1 - 5, "P 1024")
    for P in (1, 8, 100):
        left, right, _ = dm.panned(size, C, F, P, 10 + P)
        check(pv, left, right, dm.edge_rows(F, P), P, 0, None, "edge values")
    left, right, _ = dm.panned(512, C, F, 8, 4)
    check(make(512, C), left, right, dm.edge_rows(F, 8), 8, 3, 252, "edge values, size 512")


@pytest.mark.parametrize("size", [64, 2048])
def test_the_two_inputs_in_one_buffer(size):
    """every bin is then RIGHT, and at u = 0 where its amp is an ordinary number (a denormal amp times a gain rounds to the
    amp before n reaches P: the scan decides, and the odd bins of the full recipe have some)"""
    C, F, P = 3, 5, 8
    pv = make(size, C)
    for pans in ([(-1, 3), (1, 5)], None):
        left, _, _ = dm.panned(size, C, F, P, 2, pans)
        want, wprof = dm.demix(left, left, dm.par_rows(F, P), P)
        got, prof = run_guarded(pv, left, left, dm.par_rows(F, P), P, same_buffer=True)
        same(got, want, "one buffer")
        assert np.array_equal(bits(prof), bits(wprof)) and np.array_equal(bits(got[..., 1]), bits(left[..., 1]))
        if pans:
            assert not wprof[..., :P].any() and not wprof[..., P + 1:].any() and wprof[..., P].all()


@pytest.mark.parametrize("grid_max", [1, 3])
@pytest.mark.parametrize("size", [64, 512, 2048])
def test_the_bits_do_not_depend_on_the_grid(size, grid_max, monkeypatch):
    C, F = 3, 37
    pv = make(size, C, grid_max=grid_max, monkeypatch=monkeypatch)
    for name, left, right, par, P, first, nbins in gpu_cases(size, C, F)[1:4]:
        check(pv, left, right, par, P, first, nbins, "size %d grid %d %s" % (size, grid_max, name))


@pytest.mark.parametrize("size", [64, 2048])
def test_a_stream_cut_into_calls_gives_the_uncut_bits(size):
    C, F, P = 3, 37, 8
    pv = make(size, C)
    B = size // 2 + 1
    left, right, _ = dm.panned(size, C, F, P, size)
    par = dm.par_rows(F, P, 1)
    whole, wprof = run_guarded(pv, left, right, par, P, 3, B - 5)
    parts, profs, a = [], [], 0
    for cut in (1, 2, 5, 29):
        got, prof = run_guarded(pv, left[:, a:a + cut], right[:, a:a + cut], par[a:a + cut], P, 3, B - 5)
        parts.append(got)
        profs.append(prof)
        a += cut
    assert a == F
    same(np.concatenate(parts, axis=1), whole, "size %d cut" % size)
    assert np.array_equal(bits(np.concatenate(profs, axis=1)), bits(wprof))


def test_a_call_on_another_stream():
    size, C, F = 512, 3, 12
    pv = make(size, C)
    name, left, right, par, P, first, nbins = gpu_cases(size, C, F)[1]
    check(pv, left, right, par, P, first, nbins, "the current stream")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(pv, left, right, par, P, first, nbins, "a second stream")
    check(pv, left, right, par, P, first, nbins, "a second stream, named", stream=side)


def test_a_graph_replay_reads_the_par_of_its_time():
    size, C, F, P = 1024, 2, 12, 8
    B = size // 2 + 1
    pv = make(size, C)
    left, right, _ = dm.panned(size, C, F, P, 12)
    dl, dr, out = dev(left), dev(right), torch.zeros((C, F, B, 2), device=DEV)
    prof = torch.zeros((C, F, 2 * P + 1), device=DEV)
    rows = [dm.par_rows(F, P, s) for s in (0, 1, 2)]
    dp = dev(rows[0])
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.demix_device(dl, dr, out, dp, P, az_out=prof) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.demix_device(dl, dr, out, dp, P, az_out=prof) == 0
    for row in rows[1:]:
        dp.copy_(torch.from_numpy(row))
        out.zero_()
        prof.zero_()
        g.replay()
        torch.cuda.synchronize()
        want, wprof = dm.demix(left, right, row, P)
        same(out.cpu().numpy(), want, "replay")
        assert np.array_equal(bits(prof.cpu().numpy()), bits(wprof))
    assert not np.array_equal(bits(dm.demix(left, right, rows[1], P)[0]), bits(dm.demix(left, right, rows[2], P)[0]))


def _states(pv):
    return (pv.read_prev(), pv.read_phase(), pv.desc_state()) + tuple(pv.adsyn_state()) + \
        tuple(pv.time_state(op) for op in ("blur", "smooth", "freeze"))


def _equal_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_the_blocking_form_the_states_and_refused_calls():
    size, C, F, P = 64, 2, 9, 8
    M = size // 2
    B, J = M + 1, 2 * P + 1
    pv = make(size, C)
    assert pv.blur_setup(3) == 0
    # every state away from its initial value
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr, sp, sig = torch.zeros((C, F, B, 2), device=DEV), torch.zeros_like(spec), torch.zeros((C, F * pv.hop), device=DEV)
    fo, d8 = torch.zeros_like(fr), torch.zeros((C, F, 8), device=DEV)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0 and pv.adsyn_device(fr, sig) == 0
    assert pv.blur_device(fr, fo, 2.0) == 0 and pv.smooth_device(fr, fo) == 0 and pv.freeze_device(fr, fo) == 0
    assert pv.describe_device(fr, d8) == 0
    torch.cuda.synchronize()
    states = _states(pv)
    left, right, _ = dm.panned(size, C, F, P, 21)
    par = dm.par_rows(F, P, 2)
    # the blocking form gives the device form's bits, and refuses what the device form clamps
    got, prof = run_guarded(pv, left, right, par, P, 3, B - 5)
    hgot, hprof = pv.demix(left, right, par[:, 0], par[:, 1], P, 3, B - 5, az=True)
    same(hgot, got, "host form")
    assert np.array_equal(bits(hprof), bits(prof)) and hprof.dtype == f32 and hprof.shape == (C, F, J)
    same(pv.demix(left, right, par[:, 0], par[:, 1], P, 3, B - 5), got, "host form without the profile")
    same(pv.demix(left, right, 0.37, 4, P), dm.demix(left, right, np.tile(np.array([0.37, 4], f32), (F, 1)), P)[0], "numbers")
    for pos, width in ((1.5, 3), (np.nan, 3), (0, 0.5), (0, J + 1), (0, np.nan), (-np.inf, 3)):
        with pytest.raises(fa.ClError) as e:
            pv.demix(left, right, pos, width, P)
        assert e.value.code == CL_INVALID_VALUE, (pos, width)
    one = make(size, 1)
    h, hp = one.demix(left[0], right[0], par[:, 0], par[:, 1], P, az=True)
    w, wp = dm.demix(left[:1], right[:1], par, P)
    same(h, w[0], "one channel, host form")
    assert np.array_equal(bits(hp), bits(wp[0]))
    o, op = torch.zeros((F, B, 2), device=DEV), torch.zeros((F, J), device=DEV)
    assert one.demix_device(dev(left[0]), dev(right[0]), o, dev(par), P, az_out=op) == 0
    same(o.cpu().numpy(), w[0], "one channel, device form")
    assert np.array_equal(bits(op.cpu().numpy()), bits(wp[0]))
    assert _equal_bytes(_states(pv), states), "a demix call touched a state"
    # refused calls write nothing: overlaps by one pair or one word, bad ranges and points, wrong tensors
    nf, na = left.size, C * F * J
    buf = torch.full((3 * nf + na + 2 * F,), CANARY, dtype=torch.int32, device=DEV)
    fbuf = buf.view(torch.float32)
    shape = left.shape
    gl, gr, gout = (fbuf[i * nf:(i + 1) * nf].view(*shape) for i in range(3))
    ga, gp = fbuf[3 * nf:3 * nf + na].view(C, F, J), fbuf[3 * nf + na:].view(F, 2)
    frames_at = lambda at: fbuf[at:at + nf].view(*shape)
    prof_at = lambda at: fbuf[at:at + na].view(C, F, J)
    par_at = lambda at: fbuf[at:at + 2 * F].view(F, 2)
    refused = [
        (gl, gr, frames_at(2 * nf - 2), gp, None), (gl, gr, frames_at(nf - 2), gp, None), (gl, gr, frames_at(2), gp, None),
        (frames_at(2 * nf + 2), gr, gout, gp, None), (gl, frames_at(2 * nf - 2), gout, gp, None),
        (gl, gr, gout, par_at(3 * nf - 1), None), (gl, gr, gout, par_at(2 * nf - 1), ga),
        (gl, gr, gout, gp, prof_at(3 * nf - 1)), (gl, gr, gout, gp, prof_at(nf - 1)), (gl, gr, gout, gp, prof_at(2 * nf - 1)),
        (gl, gr, gout, gp, prof_at(3 * nf + 1)), (gl, gr, gout, par_at(3 * nf + na - 1), ga),
    ]
    for l, r, o_, p_, a_ in refused:
        assert pv.demix_device(l, r, o_, p_, P, az_out=a_) == CL_INVALID_VALUE
    for first, nbins in ((0, 0), (1, M + 1), (-1, 3), (M + 1, 1), (M, 2)):
        assert pv.demix_device(gl, gr, gout, gp, P, first, nbins, az_out=ga) == CL_INVALID_VALUE, (first, nbins)
    L = fa._lib.lib()
    for points in (0, 1025, -1):
        assert pv.demix_device(gl, gr, gout, gp, points) == CL_INVALID_VALUE
        assert L.clfa_pvoc_demix_dev(pv._h, gl.data_ptr(), gr.data_ptr(), gout.data_ptr(), gp.data_ptr(), ga.data_ptr(), F,
                                     points, 0, B, None) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout[:, :F - 1].contiguous(), gp, P) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr[:, :F - 1].contiguous(), gout, gp, P) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp[:F - 1].contiguous(), P) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp.double(), P) == CL_INVALID_VALUE
    assert pv.demix_device(gl.double(), gr, gout, gp, P) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp, P, az_out=ga[:, :F - 1].contiguous()) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp, P, az_out=ga.double()) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp, P, az_out=ga[..., :J - 1]) == CL_INVALID_VALUE
    assert pv.demix_device(gl, gr, gout, gp, P + 1, az_out=ga) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, B, 2), device=DEV)
    assert pv.demix_device(e, e, torch.zeros_like(e), (0.0, 1.0), P, az_out=torch.zeros((C, 0, J), device=DEV)) == 0
    z = np.zeros((C, 0, B, 2), f32)
    assert pv.demix(z, z, 0, 1, P).shape == (C, 0, B, 2)
    assert _equal_bytes(_states(pv), states)
    # an object without a device: a bad argument is still an invalid value, a good call the object's error
    none = fa.Pvoc(99, size, size // 4, SR, C)
    assert none.get_error() != 0 and none.demix_kernel_name() == "" and none.demix_kernel_name(az=True) == ""
    assert none.demix_device(gl, gr, gout, gp, 0) == CL_INVALID_VALUE
    assert none.demix_device(gl, gr, gout, gp, P, 0, 0) == CL_INVALID_VALUE
    assert none.demix_device(gl, gr, gout, gp, P, az_out=ga) == none.get_error()
