"""The frame operations of clfa_pvoc on the device (pvoc_ops.hip: k_pvoc_map, k_pvoc_read, k_pvoc_formant) against the numpy
restatement of their definitions (tests/pvoc_ops_model.py).

Scale and shift without keepform, and the timed read, are bit-equal with the float32 model: every operation of theirs is a
single correctly rounded float32 step.  With keepform the freq column is still bit-equal; the amps go through logf, two
LDS transforms and expf, which are not numpy's, so the contract is the one of tests/test_gpu_pvoc.py: the relative L2 error
of the amps against the float64 model is at most MARGIN times the float32 model's own error on the same inputs.

MARGIN.  The rule: the smallest of 2, 4, 8 that clears the largest ratio measured over every case of this file by a factor
1.5.  Every case prints its ratio (`PVOCOPS ...` lines, pytest -s).
MEASURED IN PART.  The first device run stopped at its fifth formant case: size 64, 1 channel, F = 1 gave ratios 1.30,
0.77, 1.15, 0.49 on analysed frames (errors 0.8e-7 .. 4.5e-7 against the model's 1.0e-7 .. 9.1e-7) and 2.15 on the tilted
raw frame (1.92e-13 against 8.92e-14: with s = 4 nearly all of that frame's energy sits in copied and empty bins, which
are exact on both sides, so the ratio is that of a handful of small bins).  2.15 x 1.5 = 3.2 rules out 2, so MARGIN is 4,
the smallest value the rule allows on what has been measured.  The other cases of this file (3 channels, size 1024 and
16384, the capped grids) have not run on a device yet: their `PVOCOPS` lines decide whether 4 stands.
"""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from opencl_fft_amd import _lib
from tests import pvoc_model as pm
from tests import pvoc_ops_model as om
from tests import pvoc_inputs, stft_model
from tests.gpu_guard import CANARY, DEV, bits, dev, flat, run
from tests.pvoc_inputs import SR, hann, make_pvoc

pytestmark = pytest.mark.gpu
MARGIN = 4.0            # see the docstring: the largest ratio measured so far is 2.15
CL_INVALID_VALUE = -30
f32 = np.float32
RATIO = {"max": 0.0}


def fpw(size):
    """frames per workgroup of k_pvoc_formant (LdsGeom: 16 points per lane, at least 256 lanes)"""
    t = max(size // 2 // 16, 1)
    return max(t, 256) // t


def make(size, channels=1, hop=None, grid_max=None, monkeypatch=None):
    pv = make_pvoc(size, hop or size // 4, channels, env={"CLFA_PVOC_OPS_GRID_MAX": grid_max}, monkeypatch=monkeypatch)
    assert (pv.ops_kernel_name("scale"), pv.ops_kernel_name("shift", True), pv.ops_kernel_name("read")) == \
        ("k_pvoc_map", "k_pvoc_formant", "k_pvoc_read")
    return pv


def analysed(size, C, F, seed=3):
    """the shared frames with the tones of test_gpu_pvoc.py: bins 10.37 and size / 2 - 3.21"""
    return pvoc_inputs.analysed(size, C, F, seed, seeded_tones=False)


def raw(size, C, F, seed=4, tilt=False):
    """the shared raw frames; tilt (the formant cases): the whole span of 60 decades as the slope, no forced zero"""
    return pvoc_inputs.raw(size, C, F, seed, tilt, decades=30, zero=False)


def frame_counts(size):
    return [1, 5, fpw(size) + 1]


def per_frame(F, kind, size, seed=0):
    rng = np.random.default_rng(F + seed)
    if kind == "scale":
        s = rng.uniform(0.25, 4.0, F).astype(f32)
        s[0] = 0.25
        s[-1] = 4.0
        if F > 2:
            s[1] = 1.0
        return s
    hz = (rng.uniform(-40, 40, F) * SR / size).astype(f32)
    hz[0] = -3 * SR / size
    if F > 2:
        hz[1] = 0.0
        hz[2] = 1e9           # past every bin
    return hz


def positions(Fin, Fout, seed=0):
    rng = np.random.default_rng(Fout + seed)
    p = rng.uniform(-1.0, Fin + 0.5, Fout).astype(f32)
    special = [-2.5, Fin + 7.0, np.nan, float(Fin - 1), 0.0, float(Fin // 2), Fin - 1 - 0.25, np.inf, -np.inf]
    for i, v in enumerate(special[:Fout]):
        p[i] = v
    return p


def check_bits(pv, fr, what):
    """scale and shift without keepform and the read on `fr`: bit-equal with the float32 model"""
    size, (C, F, B, _) = pv.size, fr.shape
    d = dev(fr)
    s, hz = per_frame(F, "scale", size), per_frame(F, "shift", size)
    got = run(lambda o: pv.scale_device(d, o, dev(s), gain=0.7), fr.shape)
    assert np.array_equal(bits(got), bits(om.op32("scale", fr, s, size, SR, gain=0.7))), what + ": scale"
    got = run(lambda o: pv.shift_device(d, o, dev(hz), lowest_bin=3, gain=1.25), fr.shape)
    assert np.array_equal(bits(got), bits(om.op32("shift", fr, hz, size, SR, lowest=3, gain=1.25))), what + ": shift"
    # plain numbers
    got = run(lambda o: pv.scale_device(d, o, 1.5), fr.shape)
    assert np.array_equal(bits(got), bits(om.op32("scale", fr, 1.5, size, SR))), what + ": scale by a number"
    got = run(lambda o: pv.shift_device(d, o, -777.0, lowest_bin=B - 2), fr.shape)
    assert np.array_equal(bits(got), bits(om.op32("shift", fr, -777.0, size, SR, lowest=B - 2))), what + ": shift by a number"
    for Fout in (1, F + 4, 2 * F + 9):
        pos = positions(F, Fout)
        got = run(lambda o: pv.read_device(d, dev(pos), o), (C, Fout, B, 2))
        assert np.array_equal(bits(got), bits(om.read32(fr, pos))), what + ": read %d" % Fout


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_map_and_read_are_the_models_bits(size, channels, monkeypatch):
    pv = make(size, channels)
    for F in frame_counts(size):
        check_bits(pv, analysed(size, channels, F), "size %d ch %d F %d analysed" % (size, channels, F))
        check_bits(pv, raw(size, channels, F), "size %d ch %d F %d raw" % (size, channels, F))
    # more items than the launched grid takes in one stride: launches of at most 2 workgroups
    small = make(size, channels, grid_max=2, monkeypatch=monkeypatch)
    check_bits(small, raw(size, channels, 7), "size %d ch %d grid of 2" % (size, channels))


def check_formant(pv, fr, coefs, what):
    """scale and shift with keepform: freq bit-equal, amps within MARGIN of the float32 model's error against float64"""
    size, (C, F, B, _) = pv.size, fr.shape
    d = dev(fr)
    s, hz = per_frame(F, "scale", size, 1), per_frame(F, "shift", size, 1)
    for op, par, kw, mk in (("scale", s, dict(gain=0.9), {}), ("shift", hz, dict(lowest_bin=2, gain=1.1), dict(lowest=2))):
        fn = pv.scale_device if op == "scale" else pv.shift_device
        got = run(lambda o: fn(d, o, dev(par), keepform=True, coefs=coefs, **kw), fr.shape)
        m32 = om.op32(op, fr, par, size, SR, keepform=True, gain=kw["gain"], coefs=coefs, **mk)
        m64 = om.op64_amps(op, fr, par, size, SR, keepform=True, gain=kw["gain"], coefs=coefs, **mk)
        assert np.isfinite(m32).all() and np.isfinite(m64).all(), "the inputs overflow the model"
        assert np.array_equal(bits(got[..., 1]), bits(m32[..., 1])), "%s %s: freq" % (what, op)
        e_dev, e_f32 = om.rel_l2(got[..., 0], m64), om.rel_l2(m32[..., 0], m64)
        ratio = e_dev / max(e_f32, 1e-300)
        RATIO["max"] = max(RATIO["max"], ratio)
        print("PVOCOPS %s %s coefs %d: amps relL2 %.3g (float32 model %.3g, ratio %.2f; largest so far %.2f)"
              % (what, op, coefs, e_dev, e_f32, ratio, RATIO["max"]))
        assert e_dev <= MARGIN * e_f32, "%s %s: %.3g against %.3g" % (what, op, e_dev, e_f32)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [64, 1024])
def test_formant_accuracy(size, channels, monkeypatch):
    pv = make(size, channels)
    for F in frame_counts(size):
        for coefs in (1, min(24, size // 2 - 1)):
            check_formant(pv, analysed(size, channels, F), coefs, "size %d ch %d F %d analysed" % (size, channels, F))
        check_formant(pv, raw(size, channels, F, tilt=True), 12, "size %d ch %d F %d raw" % (size, channels, F))
    small = make(size, channels, grid_max=2, monkeypatch=monkeypatch)
    F = (2 * fpw(size)) // channels + 3         # more than two groups of frames
    check_formant(small, analysed(size, channels, F), 20, "size %d ch %d grid of 2" % (size, channels))
    check_formant(small, analysed(size, channels, F), size // 2 - 1, "size %d ch %d grid of 2, all coefs" % (size, channels))


def test_size_16384_once():
    """the tables-from-cache route of k_pvoc_formant, and the widest rows of the other two kernels"""
    size, C, F = 16384, 2, 3
    pv = make(size, C)
    fr = analysed(size, C, F)
    check_bits(pv, fr, "size 16384")
    check_formant(pv, fr, 80, "size 16384 analysed")
    check_formant(pv, raw(size, C, F, tilt=True), 40, "size 16384 raw")


@pytest.mark.parametrize("size", [64, 1024])
def test_confinement(size):
    C, F = 2, fpw(size) + 1
    M = size // 2
    pv = make(size, C)
    clean = np.array(analysed(size, C, F))
    c0, f0, k0 = 1, F // 2, M // 3
    s, hz = per_frame(F, "scale", size, 2), per_frame(F, "shift", size, 2)
    s[f0], hz[f0] = 0.5, 2 * SR / size         # (two sources per bin at 0.5: k0 may lose its bin to k0 + 1)
    calls = [("scale", s, lambda d, o, kf: pv.scale_device(d, o, dev(s), keepform=kf, coefs=10), {}),
             ("shift", hz, lambda d, o, kf: pv.shift_device(d, o, dev(hz), lowest_bin=2, keepform=kf, coefs=10), dict(lowest=2))]
    for bad_k in (k0, k0 + 1):
        bad = clean.copy()
        bad[c0, f0, bad_k, 0] = np.nan
        for op, par, call, mk in calls:
            src = om.maps(op, M, par, mk.get("lowest", 1), om.bpf_of(size, SR))[f0]
            want = np.zeros((C, F, M + 1), bool)
            want[c0, f0, src == bad_k] = True
            for kf in (False, True):
                got = run(lambda o: call(dev(bad), o, kf), bad.shape)
                assert np.array_equal(np.isnan(got[..., 0]), want), "%s keepform %d: where the NaN went" % (op, kf)
                assert not np.isnan(got[..., 1]).any()
                ref = run(lambda o: call(dev(clean), o, kf), clean.shape)
                got[c0, f0], ref[c0, f0] = 0, 0
                assert np.array_equal(bits(got), bits(ref)), "%s keepform %d: another frame changed" % (op, kf)
            if op == "shift":
                assert want.any()
    # an Inf amp with keepform stays inside its frame
    bad = clean.copy()
    bad[c0, f0, k0, 0] = np.inf
    for op, par, call, mk in calls:
        got, ref = run(lambda o: call(dev(bad), o, True), bad.shape), run(lambda o: call(dev(clean), o, True), clean.shape)
        got[c0, f0], ref[c0, f0] = 0, 0
        assert np.array_equal(bits(got), bits(ref)), op
    # a NaN frame that a read gives the weight a == 0 (as frame i + 1 of an integer position, and never as frame i)
    bad = clean.copy()
    bad[:, f0] = np.nan
    pos = np.array([f0 - 1, f0 + 1, 0, f0 - 1.0, F + 3], f32)
    got = run(lambda o: pv.read_device(dev(bad), dev(pos), o), (C, pos.size, M + 1, 2))
    assert not np.isnan(got).any() and np.array_equal(bits(got), bits(om.read32(bad, pos)))


def test_the_calls_are_stateless_and_repeatable():
    size, C, F = 1024, 2, 11
    M = size // 2
    pv = make(size, C)
    # states away from their initial values
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    fr = torch.zeros((C, F, M + 1, 2), device=DEV)
    sp = torch.zeros_like(spec)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0
    state = (pv.read_prev(), pv.read_phase())
    s, hz, pos = dev(per_frame(F, "scale", size)), dev(per_frame(F, "shift", size)), dev(positions(F, F))
    calls = [lambda o, st: pv.scale_device(fr, o, s, stream=st), lambda o, st: pv.scale_device(fr, o, s, keepform=True, coefs=30, stream=st),
             lambda o, st: pv.shift_device(fr, o, hz, lowest_bin=4, keepform=True, coefs=30, stream=st),
             lambda o, st: pv.shift_device(fr, o, hz, stream=st), lambda o, st: pv.read_device(fr, pos, o, stream=st)]
    first = []
    for call in calls:
        a, b = torch.zeros_like(fr), torch.zeros_like(fr)
        assert call(a, None) == 0 and call(b, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the same call twice"
        first.append(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = [torch.zeros_like(fr) for _ in calls]
    with torch.cuda.stream(side):
        for call, o in zip(calls, outs):
            assert call(o, None) == 0
    torch.cuda.synchronize()
    for a, o in zip(first, outs):
        assert torch.equal(a.view(torch.int32), o.view(torch.int32)), "side stream"
    # every call captured (none allocates), replayed twice
    outs = [torch.zeros_like(fr) for _ in calls]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for call, o in zip(calls, outs):
            assert call(o, None) == 0
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, o in zip(first, outs):
            assert torch.equal(a.view(torch.int32), o.view(torch.int32)), "graph replay"
    assert np.array_equal(bits(pv.read_prev()), bits(state[0])) and np.array_equal(pv.read_phase(), state[1])
    # the host forms are the device forms
    h = fr.cpu().numpy()
    assert np.array_equal(bits(pv.scale(h, s.cpu().numpy(), keepform=True, coefs=30)), bits(first[1].cpu().numpy()))
    assert np.array_equal(bits(pv.shift(h, hz.cpu().numpy())), bits(first[3].cpu().numpy()))
    assert np.array_equal(bits(pv.read(h, pos.cpu().numpy())), bits(first[4].cpu().numpy()))
    assert np.array_equal(bits(pv.read_prev()), bits(state[0])) and np.array_equal(pv.read_phase(), state[1])


def test_errors_write_nothing():
    size, C, F = 64, 2, 5
    M = size // 2
    pv = make(size, C)
    fr = dev(analysed(size, C, F))
    s = dev(per_frame(F, "scale", size))
    g = flat((C, F, M + 1, 2))
    out = g.data
    for coefs in (0, M, -3):
        assert pv.scale_device(fr, out, s, keepform=True, coefs=coefs) == CL_INVALID_VALUE
        assert pv.shift_device(fr, out, s, keepform=True, coefs=coefs) == CL_INVALID_VALUE
    for lowest in (0, M, -1):
        assert pv.shift_device(fr, out, s, lowest_bin=lowest) == CL_INVALID_VALUE
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    assert L.clfa_pvoc_read_dev(pv._h, fr.data_ptr(), 2 ** 24 + 1, s.data_ptr(), out.data_ptr(), F, st) == CL_INVALID_VALUE
    assert L.clfa_pvoc_read_dev(pv._h, fr.data_ptr(), 0, s.data_ptr(), out.data_ptr(), F, st) == CL_INVALID_VALUE
    # shapes, dtypes, strides
    assert pv.scale_device(fr[:, :4].contiguous(), out, s) == CL_INVALID_VALUE
    assert pv.scale_device(fr, out, s[:4].contiguous()) == CL_INVALID_VALUE
    assert pv.scale_device(fr.double(), out, s) == CL_INVALID_VALUE
    assert pv.read_device(fr, 1.0, out) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert g.untouched()
    # an output overlapping the frames, or the per-frame array, even partly
    n = C * F * (M + 1) * 2
    buf = torch.full((2 * n + F,), CANARY, dtype=torch.int32, device=DEV).view(torch.float32)
    a, b = buf[:n].view(C, F, M + 1, 2), buf[n - 2:2 * n - 2].view(C, F, M + 1, 2)
    par = buf[2 * n - 4:2 * n - 4 + F]
    for call in (lambda i, o, p: pv.scale_device(i, o, p), lambda i, o, p: pv.scale_device(i, o, p, keepform=True, coefs=5),
                 lambda i, o, p: pv.shift_device(i, o, p), lambda i, o, p: pv.read_device(i, p, o)):
        assert call(a, b, s) == CL_INVALID_VALUE and call(b, a, s) == CL_INVALID_VALUE and call(a, a, s) == CL_INVALID_VALUE
        assert call(fr, b, par) == CL_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int32) == CANARY).all())
    # F == 0: success, nothing happens
    e = torch.zeros((C, 0, M + 1, 2), device=DEV)
    assert pv.scale_device(e, e.clone(), s[:0].contiguous()) == 0 and pv.read_device(fr, s[:0].contiguous(), e) == 0


def _model_chain(x, size, hop, scale):
    """Stft.analyze -> Pvoc.analyze -> scale -> Pvoc.synthesize -> Stft.synthesize(normalize) on the numpy models"""
    w = hann(size)
    fr = stft_model.windowed_frames_f32(x[None], size, hop, w)
    P = fa.onesided_to_packed(np.fft.rfft(fr.astype(np.float64), axis=-1)).astype(np.complex64)
    f32fr = pm.analyze32(P, pm.initial_prev(1, size), size, hop, SR)
    moved = om.op32("scale", f32fr, scale, size, SR)
    th, _ = pm.phases(moved[..., 1], pm.initial_phase(1, size), hop, SR)
    Q = pm.synth32(moved, th)
    r = np.fft.irfft(fa.packed_to_onesided(Q.astype(np.complex128)), n=size, axis=-1)
    return stft_model.overlap_add(r, w, hop, normalize=True)[0][0]


def _peak(y, lo, n):
    return int(np.argmax(np.abs(np.fft.rfft(np.asarray(y[lo:lo + n], np.float64)))))


def test_end_to_end_pitch_scale_moves_a_sinusoid():
    """a sinusoid on bin 320 of an 8192-point rfft (bin 40 of the 1024-point frames) scaled by 1.5: the steady part of the
    output peaks at bin 480"""
    size, hop, F, nfft, b = 1024, 256, 64, 8192, 320
    n = size + (F - 1) * hop
    x = (0.5 * np.cos(2 * np.pi * b / nfft * np.arange(n) + 0.4)).astype(f32)
    lo = 4 * size
    assert _peak(x, lo, nfft) == b
    assert _peak(_model_chain(x, size, hop, 1.5), lo, nfft) == round(1.5 * b), "the models' chain"
    an, sy, pv = fa.Stft(0, size, hop, window=hann(size)), fa.Stft(0, size, hop, window=hann(size), fwd=False), make(size, 1, hop)
    spec = an.analyze(x[None])
    y = sy.synthesize(pv.synthesize(pv.scale(pv.analyze(spec), 1.5, keepform=False)), normalize=True)[0]
    assert _peak(y, lo, nfft) == round(1.5 * b)
