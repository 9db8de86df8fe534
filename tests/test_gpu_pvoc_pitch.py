"""The pitch of clfa_pvoc on the device (pitch_kernels.hip: k_pvoc_pitch) against the numpy restatement of its definition
(tests/pvoc_pitch_model.py).

Everything is compared bit for bit: the definition fixes every rounding and the order of every sum, so there is no
tolerance to choose.  Where the model gives a NaN the device gives a NaN.  The inputs are the planted cases of the model
file (tests/test_pvoc_pitch_cpu.py shows that they tell seven mutants from the model at every size run here),
tests/pvoc_inputs.py's raw frames with NaN amps and freqs, harmonic series planted into frames, and harmonic tones
analysed on the device.  Both outputs lie in the guard bands of tests/gpu_guard.py: the rows 4-byte and not 8-byte
aligned, the peak list 8-byte and not 16-byte aligned."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import gpu_guard
from tests import pvoc_pitch_model as pt
from tests.gpu_guard import CANARY, DEV, bits, dev, same
from tests.pvoc_inputs import SR, analyse_device, make_pvoc, raw_freq_first

pytestmark = pytest.mark.gpu
CL_INVALID_VALUE = -30
f32 = np.float32
SIZES = (64, 128, 256, 512, 2048, 16384)      # W = 32, 64, 128, 256; then 4 and 32 rows a lane
_TONES = {}


def make(size, channels=1, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert pv.pitch_kernel_name() == "k_pvoc_pitch"
    return pv


def full(args):
    return dict(pt.DEFAULTS, **args)


def run_guarded(pv, x, args, peaks=True, stream=None):
    """one device call into guarded outputs: (rows, list or None) as numpy, the guard bands checked, every element written"""
    a = full(args)
    dx = dev(x)
    rows = gpu_guard.flat(x.shape[:2] + (4,), misalign=1)
    lst = gpu_guard.flat(x.shape[:2] + (a["npeaks"], 2), misalign=2) if peaks else None
    assert rows.data.data_ptr() % 8 == 4 and (lst is None or lst.data.data_ptr() % 16 == 8)
    if stream is not None:
        torch.cuda.synchronize()          # the arrays above were filled on the current stream
    assert pv.pitch_device(dx, rows.data, peaks_out=None if lst is None else lst.data, stream=stream, **a) == 0
    torch.cuda.synchronize()
    for g, what in ((rows, "the rows"), (lst, "the peak list")):
        if g is not None:
            g.check_sides(what)
            assert not g.unwritten(), "an element of %s was not written" % what
    return rows.data.cpu().numpy(), None if lst is None else lst.data.cpu().numpy()


def check(pv, x, args, what, peaks=True, stream=None):
    got, lst = run_guarded(pv, x, args, peaks, stream)
    want, wlst = pt.pitch(x, **args)
    what = "%s %s" % (what, sorted(args.items()))
    same(got, want, what + ": the rows")
    if peaks:
        same(lst, wlst, what + ": the peak list")
    return got


def harmonic_tones(size, C, F, seed):
    """frames of harmonic tones (20 harmonics of amplitude 1 / h below sr / 2, a random phase each, a little noise), a
    channel each, analysed on the device at hop size / 4 (numpy, cached, read-only)"""
    key = (size, C, F, seed)
    if key not in _TONES:
        rng = np.random.default_rng(seed)
        hop = size // 4
        t = np.arange(size + (F - 1) * hop) / SR
        x = 0.005 * rng.standard_normal((C, len(t)))
        for c in range(C):
            f0 = rng.uniform(3.2, 12.0) * SR / size
            for h in range(1, 21):
                if h * f0 < SR / 2:
                    x[c] += np.cos(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) / h
        a = analyse_device(x, size, hop)
        assert a.shape[1] == F
        a.setflags(write=False)
        _TONES[key] = a
    return _TONES[key]


def ranges(M):
    """all of 1..M-1, a single bin, a range that ends at M-1"""
    return ((1, M - 1), (M // 3, 1), (M - 7, 6))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_the_planted_cases_are_the_models_bits(size, channels):
    """at 1, 5 and 37 frames, with and without the list by turns (both at 37 frames)"""
    pv = make(size, channels)
    turn = 0
    for F in (1, 5, 37):
        for name, x, args in pt.planted(size, channels, F):
            turn += 1
            for peaks in ((True, False) if F == 37 else (bool(turn & 1),)):
                check(pv, x, args, "size %d ch %d F %d %s" % (size, channels, F, name), peaks)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_frames_with_nans_series_and_tones_are_the_models_bits(size, channels):
    """raw frames with NaN amps and NaN freqs, planted series and tones analysed on the device: the three ranges, npeaks
    1, 16 and 32, with and without the list"""
    pv = make(size, channels)
    M, F = size // 2, 37
    found = 0
    tones = harmonic_tones(size, channels, F, size)
    tones_args = dict(thresh=float(f32(0.01) * tones[..., 0].max()), fmin=2 * SR / size, fmax=SR / 4)
    for name, x, base in (("raw with NaNs", raw_freq_first(size, channels, F, 5), dict(thresh=1e-20, fmin=20.0, fmax=30000.0)),
                          ("raw with NaNs, tol 0.5", raw_freq_first(size, channels, F, 6), dict(thresh=0.0, fmin=1.0, fmax=48000.0, tol=0.5, decay=1.0)),
                          ("series", pt.tones(size, channels, F, size), dict(thresh=0.01, fmin=50.0, fmax=2000.0)),
                          ("tones", tones, tones_args)):
        for i, (first, nbins) in enumerate(ranges(M)):
            for j, npeaks in enumerate((1, 16, 32)):
                args = dict(base, first_bin=first, nbins=nbins, npeaks=npeaks)
                got = check(pv, x, args, "size %d ch %d %s" % (size, channels, name), peaks=bool((i + j) & 1) or npeaks == 16)
                found += int((got[..., pt.F0] > 0).sum())
    assert found > 0
    # the default call on the tones: the model's bits, and a pitch in every frame
    rows = check(pv, tones, tones_args, "tones, defaults")
    assert np.all(rows[:, 1:, pt.F0] > 0)


@pytest.mark.parametrize("size", [64, 512, 2048])
def test_the_bits_do_not_depend_on_the_grid(size, monkeypatch):
    """one workgroup: the item loop runs"""
    C, F = 3, 37
    pv = make(size, C, grid_max=1, monkeypatch=monkeypatch)
    for name, x, args in pt.planted(size, C, F)[::3]:
        check(pv, x, args, "size %d grid 1 %s" % (size, name))
    check(pv, pt.tones(size, C, F, 2), dict(thresh=0.01, fmin=50.0, fmax=2000.0, npeaks=32), "size %d grid 1 series" % size)
    check(pv, raw_freq_first(size, C, F, 5), dict(thresh=0.0, fmin=20.0, fmax=30000.0), "size %d grid 1 raw" % size, peaks=False)


@pytest.mark.parametrize("size", [64, 2048])
def test_a_stream_cut_into_calls_gives_the_uncut_bits(size):
    C, F = 3, 37
    pv = make(size, C)
    x = pt.tones(size, C, F, size + 1)
    args = dict(thresh=0.01, fmin=50.0, fmax=2000.0, npeaks=16)
    whole, wlst = run_guarded(pv, x, args)
    for cut in (1, 4):
        parts = [run_guarded(pv, x[:, a:a + cut], args) for a in range(0, F, cut)]
        same(np.concatenate([p[0] for p in parts], axis=1), whole, "size %d cut into calls of %d: the rows" % (size, cut))
        same(np.concatenate([p[1] for p in parts], axis=1), wlst, "size %d cut into calls of %d: the list" % (size, cut))
    same(whole, pt.pitch(x, **args)[0], "size %d uncut" % size)


def test_a_call_on_another_stream():
    size, C, F = 512, 3, 12
    pv = make(size, C)
    x = pt.tones(size, C, F, 8)
    args = dict(thresh=0.01, fmin=50.0, fmax=2000.0)
    check(pv, x, args, "the current stream")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        check(pv, x, dict(args, npeaks=5), "a second stream")
    check(pv, x, dict(args, npeaks=7), "a second stream, named", stream=side)


def test_a_graph_replay_gives_the_plain_calls_bits():
    size, C, F, NP = 1024, 2, 12, 9
    pv = make(size, C)
    args = full(dict(thresh=0.01, fmin=50.0, fmax=2000.0, npeaks=NP))
    inputs = [pt.tones(size, C, F, s) for s in (1, 2, 3)]
    plains = [run_guarded(pv, x, args) for x in inputs[1:]]
    dx = dev(inputs[0])
    rows, lst = torch.zeros((C, F, 4), device=DEV), torch.zeros((C, F, NP, 2), device=DEV)
    # the warm-up, on a side stream as torch's notes on graphs ask
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.pitch_device(dx, rows, peaks_out=lst, **args) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.pitch_device(dx, rows, peaks_out=lst, **args) == 0
    for x, (plain, plst) in zip(inputs[1:], plains):
        dx.copy_(torch.from_numpy(np.array(x)))
        rows.zero_()
        lst.zero_()
        g.replay()
        torch.cuda.synchronize()
        same(rows.cpu().numpy(), plain, "replay: the rows")
        same(lst.cpu().numpy(), plst, "replay: the list")
        same(plain, pt.pitch(x, **args)[0], "the plain call")
    assert not np.array_equal(bits(pt.pitch(inputs[1], **args)[0]), bits(pt.pitch(inputs[2], **args)[0]))


def _states(pv):
    return (pv.read_prev(), pv.read_phase(), pv.desc_state()) + tuple(pv.adsyn_state()) + \
        tuple(pv.time_state(op) for op in ("blur", "smooth", "freeze"))


def _equal_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def test_the_blocking_form_the_states_and_refused_calls():
    size, C, F, NP = 64, 2, 9, 6
    M = size // 2
    B = M + 1
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
    x = pt.tones(size, C, F, 21)
    args = dict(thresh=0.01, fmin=50.0, fmax=2000.0, npeaks=NP, first_bin=2, nbins=M - 4)
    # the blocking form gives the device form's bits
    got, lst = run_guarded(pv, x, args)
    hrows, hlst = pv.pitch(x, peaks=True, **args)
    same(hrows, got, "host form: the rows")
    same(hlst, lst, "host form: the list")
    same(pv.pitch(x, **args), got, "host form without the list")
    same(got, pt.pitch(x, **args)[0], "the device form")
    one = make(size, 1)
    h, hl = one.pitch(x[0], peaks=True, **args)
    w, wl = pt.pitch(x[:1], **args)
    same(h, w[0], "one channel, host form")
    same(hl, wl[0], "one channel, host form: the list")
    o, ol = torch.zeros((F, 4), device=DEV), torch.zeros((F, NP, 2), device=DEV)
    assert one.pitch_device(dev(x[0]), o, peaks_out=ol, **args) == 0
    same(o.cpu().numpy(), w[0], "one channel, device form")
    same(ol.cpu().numpy(), wl[0], "one channel, device form: the list")
    assert _equal_bytes(_states(pv), states), "a pitch call touched a state"
    # refused calls write nothing: overlaps by one pair or one word, bad ranges and values, wrong tensors
    nf, nr, nl = x.size, C * F * 4, C * F * NP * 2
    buf = torch.full((nf + nr + nl,), CANARY, dtype=torch.int32, device=DEV)
    fbuf = buf.view(torch.float32)
    gin, grows, gl = fbuf[:nf].view(*x.shape), fbuf[nf:nf + nr].view(C, F, 4), fbuf[nf + nr:].view(C, F, NP, 2)
    assert gin.data_ptr() % 8 == 0 and gl.data_ptr() % 8 == 0
    a = full(args)
    assert pv.pitch_device(gin, fbuf[nf - 1:nf - 1 + nr].view(C, F, 4), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(fbuf[2:nf + 2].view(*x.shape), fbuf[:nr].view(C, F, 4), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, grows, peaks_out=fbuf[nf - 2:nf - 2 + nl].view(C, F, NP, 2), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, grows, peaks_out=fbuf[nf + nr - 2:nf + nr - 2 + nl].view(C, F, NP, 2), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, fbuf[nf + nr + nl - nr:].view(C, F, 4), peaks_out=gl, **a) == CL_INVALID_VALUE
    for first, nbins in ((0, 3), (1, M), (1, 0), (-1, 3), (M, 1), (M - 1, 2)):
        assert pv.pitch_device(gin, grows, peaks_out=gl, **dict(a, first_bin=first, nbins=nbins)) == CL_INVALID_VALUE, (first, nbins)
    nan = float("nan")
    for kw in (dict(npeaks=0), dict(npeaks=33), dict(thresh=nan), dict(thresh=-1.0), dict(fmin=0.0), dict(fmin=nan), dict(fmax=nan),
               dict(fmax=10.0), dict(tol=0.6), dict(tol=nan), dict(decay=0.0), dict(decay=1.5), dict(decay=nan)):
        assert pv.pitch_device(gin, grows, **dict(a, **kw)) == CL_INVALID_VALUE, kw
    assert pv.pitch_device(gin, grows, peaks_out=gl[:, :, :NP - 1].contiguous(), **a) == CL_INVALID_VALUE   # not npeaks pairs
    assert pv.pitch_device(gin, grows[:, :F - 1].contiguous(), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, grows.double(), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, grows[..., :3], **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin, grows, peaks_out=gl.double(), **a) == CL_INVALID_VALUE
    assert pv.pitch_device(gin[:, :F - 1].contiguous(), grows, **a) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, B, 2), device=DEV)
    assert pv.pitch_device(e, torch.zeros((C, 0, 4), device=DEV), **a) == 0
    assert pv.pitch(np.zeros((C, 0, B, 2), f32), **args).shape == (C, 0, 4)
    assert _equal_bytes(_states(pv), states)
    # an object without a device: a bad argument is still an invalid value, a good call the object's error
    none = fa.Pvoc(99, size, size // 4, SR, C)
    assert none.get_error() != 0 and none.pitch_kernel_name() == ""
    assert none.pitch_device(gin, grows, **dict(a, npeaks=0)) == CL_INVALID_VALUE
    assert none.pitch_device(gin, grows, **a) == none.get_error()
