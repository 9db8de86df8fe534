"""The phase vocoder on the device (clfa_pvoc, pvoc_kernels.hip) against the numpy restatement of its definitions
(tests/pvoc_model.py): the integer phase state exactly, the previous-spectrum state bit for bit, the (amp, freq) frames and
the spectra within MARGIN of the model's own float32 evaluation, measured against float64.

MARGIN.  The device's atan2f / sincospif are not numpy's, so equality with the float32 model is not the contract; the
contract is an error against float64 of at most MARGIN times the float32 model's error on the same inputs.  The rule for
its value: the smallest of 2, 4, 8 that clears the largest ratio measured over every case of this file by a factor 1.5.
Every case prints its ratios (`PVOC ...` lines, pytest -s); profiles/pvoc_bins.txt holds a device run's.
MEASURED over every case of this file on an MI355X (145 calls and the two round trips): the analysis ratios lie between
0.91 and 1.08 (the largest: size 64, hop 3, 1 channel, 1 frame of Stft spectra), the synthesis ratios between 0.35 and
0.88 (the largest: size 1024, hop 3, 1 channel, 2 frames of Stft spectra), the round trip through Stft gives 1.00 at both
sizes.  1.08 x 1.5 = 1.62 stays under 2, so MARGIN is 2.  Why: both errors are dominated by the same roundings — of freq
to float32 in the analysis (about 2^-24 k hop / size turns of dev), of the phase to a float32 angle in the synthesis —
and the device functions add less than numpy's float32 ones there (sincospif takes half turns, so the product with pi
is not rounded).  These are aggregates over a whole call, which a loud bin dominates; every bin on its own scale is held
by tests/test_gpu_pvoc_bins.py.
"""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import pvoc_model as pm
from tests.gpu_guard import CANARY, DEV, flat
from tests.pvoc_inputs import SR, hann, make_pvoc, two_tones

pytestmark = pytest.mark.gpu
MARGIN = 2.0
CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59


def make(size, hop, channels=1):
    pv = make_pvoc(size, hop, channels)
    assert pv.kernel_name() == "k_pvoc_analyze" and pv.kernel_name(True) == "k_pvoc_walk"
    return pv


def stft_spectra(size, hop, C, F, seed):
    """Stft.analyze_device on noise plus two sinusoids (one between bins, one near Nyquist): (C, F, M) complex64 on the device"""
    x = two_tones(size, hop, C, F, seed)
    st = fa.Stft(0, size, hop, window=hann(size))
    assert st.get_error() == 0 and st.frames(x.shape[1]) == F
    out = torch.zeros((C, F, size // 2), dtype=torch.complex64, device=DEV)
    assert st.analyze_device(torch.from_numpy(x.astype(np.float32)).to(DEV), out) == 0
    torch.cuda.synchronize()
    return out


def random_spectra(size, C, F, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.view_as_complex(torch.randn((C, F, size // 2, 2), device=DEV, generator=g).contiguous())


def analyze(pv, spec):
    C, F, M = spec.shape
    fr = torch.zeros((C, F, M + 1, 2), device=DEV)
    assert pv.analyze_device(spec, fr) == 0
    return fr


def synthesize(pv, fr):
    C, F, B, _ = fr.shape
    sp = torch.zeros((C, F, B - 1), dtype=torch.complex64, device=DEV)
    assert pv.synthesize_device(fr, sp) == 0
    return sp


RATIOS = {"analysis": 0.0, "synthesis": 0.0}


def check_call(pv, spec, prev, theta, what):
    """one analysis and one synthesis of `spec` on `pv` whose states the model holds as (prev, theta): states exact,
    results within MARGIN of the float32 model's error; returns the new model states"""
    size, hop = pv.size, pv.hop
    P = spec.cpu().numpy()
    fr_t = analyze(pv, spec)
    fr = fr_t.cpu().numpy()
    amp, dev, _, new_prev = pm.analyze64(P, prev, size, hop, SR)
    got_prev = pv.read_prev()
    assert np.array_equal(got_prev.view(np.uint32), new_prev.view(np.uint32)), "%s: prev state" % what
    truth = amp * np.exp(2j * np.pi * dev)
    e_dev = pm.rel_l2(pm.phasors(fr, size, hop, SR), truth)
    e_f32 = pm.rel_l2(pm.phasors(pm.analyze32(P, prev, size, hop, SR), size, hop, SR), truth)
    # amplitudes on their own: one sqrt of two products
    assert np.abs(fr[..., 0] - amp).max() <= 4 * 2.0 ** -24 * max(amp.max(), 1e-30), "%s: amp" % what
    sp = synthesize(pv, fr_t).cpu().numpy()
    th, new_theta = pm.phases(fr[..., 1], theta, hop, SR)
    assert np.array_equal(pv.read_phase(), new_theta), "%s: phase state" % what
    s_truth = pm.synth64(fr, th)
    s_dev, s_f32 = pm.rel_l2(sp, s_truth), pm.rel_l2(pm.synth32(fr, th), s_truth)
    print("PVOC %s: analysis relL2 %.3g (float32 model %.3g, ratio %.2f)  synthesis %.3g (%.3g, ratio %.2f)"
          % (what, e_dev, e_f32, e_dev / max(e_f32, 1e-300), s_dev, s_f32, s_dev / max(s_f32, 1e-300)))
    RATIOS["analysis"] = max(RATIOS["analysis"], e_dev / max(e_f32, 1e-300))
    RATIOS["synthesis"] = max(RATIOS["synthesis"], s_dev / max(s_f32, 1e-300))
    assert e_dev <= MARGIN * e_f32, "%s: analysis %.3g against %.3g" % (what, e_dev, e_f32)
    assert s_dev <= MARGIN * s_f32, "%s: synthesis %.3g against %.3g" % (what, s_dev, s_f32)
    return new_prev, new_theta


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("hopk", ["q", "3", "s"])
@pytest.mark.parametrize("size", [64, 1024])
def test_frames_spectra_and_states_match_the_model(size, hopk, channels):
    """every frame count around the scan's chunk, Stft spectra and raw random ones, on ONE object: the states carry over
    from call to call, as the model's do"""
    hop = {"q": size // 4, "3": 3, "s": size}[hopk]
    pv = make(size, hop, channels)
    ch = pv.scan_chunk()
    prev, theta = pm.initial_prev(channels, size), pm.initial_phase(channels, size)
    assert np.array_equal(pv.read_prev(), prev) and np.array_equal(pv.read_phase(), theta)
    for i, F in enumerate([1, 2, ch - 1, ch, ch + 1, 2 * ch + 3]):
        for kind in ("stft", "random"):
            spec = stft_spectra(size, hop, channels, F, size + F) if kind == "stft" else random_spectra(size, channels, F, F)
            prev, theta = check_call(pv, spec, prev, theta, "size %d hop %d ch %d F %d %s" % (size, hop, channels, F, kind))
    assert pv.workspace_bytes() > 0
    assert pv.reset() == 0
    assert np.array_equal(pv.read_prev(), pm.initial_prev(channels, size)) and not pv.read_phase().any()
    print("PVOC largest ratios so far: analysis %.2f synthesis %.2f" % (RATIOS["analysis"], RATIOS["synthesis"]))


def test_size_16384_once():
    size, hop, C = 16384, 4096, 2
    pv = make(size, hop, C)
    F = pv.scan_chunk() + 1
    check_call(pv, stft_spectra(size, hop, C, F, 5), pm.initial_prev(C, size), pm.initial_phase(C, size), "size 16384")


def run_cut(pv, spec, cuts):
    """analysis and synthesis of spec's frames in calls cut at `cuts`, from the reset state: (frames, spectra, prev, theta)"""
    assert pv.reset() == 0
    C, F, M = spec.shape
    fr = torch.zeros((C, F, M + 1, 2), device=DEV)
    sp = torch.zeros((C, F, M), dtype=torch.complex64, device=DEV)
    for a, b in zip([0] + cuts, cuts + [F]):
        # (a call takes contiguous tensors: the channels' frames of one call are copied out and back)
        part = spec[:, a:b].contiguous()
        pf = analyze(pv, part)
        fr[:, a:b] = pf
        sp[:, a:b] = synthesize(pv, pf)
    torch.cuda.synchronize()
    return fr, sp, pv.read_prev(), pv.read_phase()


def same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(torch.view_as_real(a[1]), torch.view_as_real(b[1]))
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3], b[3]))


@pytest.mark.parametrize("size,hop,channels", [(64, 16, 3), (1024, 3, 1), (1024, 256, 3)])
def test_split_invariance(size, hop, channels, monkeypatch):
    pv = make(size, hop, channels)
    ch = pv.scan_chunk()
    F = 2 * ch + 3
    spec = stft_spectra(size, hop, channels, F, 11) + 0.05 * random_spectra(size, channels, F, 12)
    whole = run_cut(pv, spec, [])
    assert same(whole, run_cut(pv, spec, [ch - 1, ch])), "cut at chunk-1 / 1 / rest"
    assert same(whole, run_cut(pv, spec, [1, 2, ch + 7])), "another cut"
    # the same call in sub-batches of one chunk (the switch is read at creation)
    monkeypatch.setenv("CLFA_PVOC_CHUNKS_MAX", "1")
    small = make(size, hop, channels)
    monkeypatch.delenv("CLFA_PVOC_CHUNKS_MAX")
    assert same(whole, run_cut(small, spec, [])), "sub-batches of one chunk"
    assert small.workspace_bytes() == 4 * channels * (size // 2 + 1) < pv.workspace_bytes()


def test_scan_with_several_chunks_per_segment(monkeypatch):
    """34 chunks (33 whole ones and one of 5 frames) in one call: k_pvoc_scan's waves take 3 chunks each, the last occupied
    segment is short and the segments after it are empty.  The phase state is the model's serial sum; the spectra and the
    states are the bits of the same frames cut into two calls and of sub-batches of 5 chunks (other segment lengths)"""
    size, hop, channels = 64, 16, 2
    pv = make(size, hop, channels)
    ch = pv.scan_chunk()
    F = 33 * ch + 5
    spec = stft_spectra(size, hop, channels, F, 61) + 0.05 * random_spectra(size, channels, F, 62)
    whole = run_cut(pv, spec, [])
    _, new_theta = pm.phases(whole[0].cpu().numpy()[..., 1], pm.initial_phase(channels, size), hop, SR)
    assert np.array_equal(whole[3], new_theta), "phase state after one call of 34 chunks"
    assert same(whole, run_cut(pv, spec, [ch * 17 + 1])), "cut at 17 chunks + 1"
    monkeypatch.setenv("CLFA_PVOC_CHUNKS_MAX", "5")
    small = make(size, hop, channels)
    monkeypatch.delenv("CLFA_PVOC_CHUNKS_MAX")
    assert same(whole, run_cut(small, spec, [])), "sub-batches of 5 chunks"
    assert small.workspace_bytes() == 5 * 4 * channels * (size // 2 + 1) < pv.workspace_bytes()


@pytest.mark.parametrize("size,hop,channels", [(64, 16, 3), (1024, 256, 1)])
def test_side_stream_and_graph_replay(size, hop, channels):
    pv = make(size, hop, channels)
    F = 2 * pv.scan_chunk() + 3
    spec = stft_spectra(size, hop, channels, F, 21)
    whole = run_cut(pv, spec, [])          # (also the warm-up: the workspace exists from here on)
    ws = pv.workspace_bytes()
    fr = torch.zeros_like(whole[0])
    sp = torch.zeros_like(whole[1])
    side = torch.cuda.Stream()
    assert pv.reset() == 0
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.analyze_device(spec, fr) == 0
        assert pv.synthesize_device(fr, sp) == 0
    torch.cuda.synchronize()
    assert same(whole, (fr, sp, pv.read_prev(), pv.read_phase())), "side stream"
    # captured, then replayed twice: the second replay continues from the first one's states, like a second call
    fr.zero_()
    sp.zero_()
    assert pv.reset() == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.analyze_device(spec, fr) == 0
        assert pv.synthesize_device(fr, sp) == 0
    assert pv.reset() == 0     # (whatever the capture itself did to the states)
    g.replay()
    torch.cuda.synchronize()
    assert same(whole, (fr, sp, pv.read_prev(), pv.read_phase())), "graph replay"
    g.replay()
    torch.cuda.synchronize()
    twice = (fr.clone(), sp.clone(), pv.read_prev(), pv.read_phase())
    assert pv.reset() == 0
    f1 = analyze(pv, spec)
    synthesize(pv, f1)
    f2 = analyze(pv, spec)
    s2 = synthesize(pv, f2)
    torch.cuda.synchronize()
    assert same(twice, (f2, s2, pv.read_prev(), pv.read_phase())), "second replay = second call"
    assert pv.workspace_bytes() == ws


@pytest.mark.parametrize("size", [64, 1024])
def test_round_trip_through_stft(size):
    """Stft -> Pvoc.analyze -> Pvoc.synthesize -> Stft.synthesize(normalize) gives the signal's interior back as well as the
    same chain does with the model's float32 conversions in the middle"""
    hop, C = size // 4, 2
    F = 2 * 64 + 3
    n = size + (F - 1) * hop
    rng = np.random.default_rng(size)
    t = np.arange(n)
    x = (0.1 * rng.standard_normal((C, n)) + 0.7 * np.cos(2 * np.pi * 10.37 / size * t)).astype(np.float32)
    w = hann(size)
    an, sy = fa.Stft(0, size, hop, window=w), fa.Stft(0, size, hop, window=w, fwd=False)
    spec = torch.zeros((C, F, size // 2), dtype=torch.complex64, device=DEV)
    assert an.analyze_device(torch.from_numpy(x).to(DEV), spec) == 0
    pv = make(size, hop, C)
    back = synthesize(pv, analyze(pv, spec))
    P = spec.cpu().numpy()
    fr32 = pm.analyze32(P, pm.initial_prev(C, size), size, hop, SR)
    th, _ = pm.phases(fr32[..., 1], pm.initial_phase(C, size), hop, SR)
    back32 = torch.from_numpy(np.ascontiguousarray(pm.synth32(fr32, th))).to(DEV)
    ys = []
    for b in (back, back32):
        y = torch.zeros((C, n), device=DEV)
        assert sy.synthesize_device(b, y, normalize=True) == 0
        torch.cuda.synchronize()
        ys.append(y.cpu().numpy())
    inner = slice(size, n - size)
    e_dev, e_f32 = pm.rel_l2(ys[0][:, inner], x[:, inner]), pm.rel_l2(ys[1][:, inner], x[:, inner])
    print("PVOC round trip size %d: relL2 %.3g (float32 model's conversions %.3g, ratio %.2f)" % (size, e_dev, e_f32, e_dev / e_f32))
    assert e_dev <= MARGIN * e_f32, (e_dev, e_f32)
    assert e_f32 < 1e-2, "the model's own chain does not return the signal"


def test_special_bins_and_zero_spectrum():
    size, hop, C, F = 64, 16, 1, 3
    M = size // 2
    pv = make(size, hop, C)
    P = np.zeros((C, F, M), np.complex64)
    P[0, :, 0] = [-2.0 - 0.5j, -1.0 - 3.0j, 4.0 - 1.0j]      # Re P[0] < 0 and Im P[0] < 0 (then a change of sign)
    P[0, :, M // 2] = [1.0 + 2.0j, -2.0 + 1.0j, 0.5 - 1.0j]
    P[0, :, 5] = [1.0j, -1.0, -1.0j]
    fr = analyze(pv, torch.from_numpy(P).to(DEV))
    f = fr.cpu().numpy()
    amp, dev, freq, _ = pm.analyze64(P, pm.initial_prev(C, size), size, hop, SR)
    for k in (0, M // 2, M, 5):
        assert np.allclose(f[0, :, k, 0], amp[0, :, k], rtol=1e-6), k
    assert np.allclose(f[0, :, 0, 0], [2, 1, 4]) and np.allclose(f[0, :, M, 0], [0.5, 3, 1])
    for k in (M // 2, 5):      # phases away from the cut: freq itself compares
        assert np.allclose(f[0, :, k, 1], freq[0, :, k], rtol=1e-5, atol=1e-3), (k, f[0, :, k, 1], freq[0, :, k])
    # every other bin is zero: amp 0 and the bin-centre frequency, (float)k * (float)(sr / size) to the bit
    zero = [k for k in range(M + 1) if k not in (0, M // 2, M, 5)]
    fz = f[0][:, zero]                                        # (F, bins, 2)
    assert not fz[..., 0].any()
    want = np.arange(M + 1, dtype=np.float32) * np.float32(SR / size)
    assert np.array_equal(fz[..., 1], np.broadcast_to(want[zero], (F, len(zero))))
    sp = synthesize(pv, fr).cpu().numpy()
    # freq is a float32 of about k + 4 dev: every phase increment carries about 2^-24 M / 4 turns of rounding, over F frames
    assert pm.rel_l2(sp, P) < 2 * np.pi * F * 2.0 ** -24 * M, sp[0][:, [0, M // 2, 5]]
    assert np.all(np.sign(sp[0, :, 0].real) == np.sign(P[0, :, 0].real)) and np.all(sp[0, :, 0].imag < 0)


@pytest.mark.parametrize("size,hop,channels", [(64, 16, 3), (1024, 3, 2)])
def test_guard_bands_and_a_nan_frequency(size, hop, channels):
    pv = make(size, hop, channels)
    M, F = size // 2, pv.scan_chunk() + 5
    spec = stft_spectra(size, hop, channels, F, 31)
    plain_fr = analyze(pv, spec)
    plain_sp = synthesize(pv, plain_fr)
    state = (pv.read_prev(), pv.read_phase())
    assert pv.reset() == 0
    fg, sg = flat((channels, F, M + 1, 2)), flat((channels, F, M, 2))
    fr = fg.data
    sp = torch.view_as_complex(sg.data)
    assert pv.analyze_device(spec, fr) == 0 and pv.synthesize_device(fr, sp) == 0
    torch.cuda.synchronize()
    assert fg.intact() and sg.intact(), "wrote outside an output"
    assert not fg.unwritten() and not sg.unwritten()
    assert torch.equal(fr, plain_fr) and torch.equal(torch.view_as_real(sp), torch.view_as_real(plain_sp))
    assert np.array_equal(pv.read_prev().view(np.uint32), state[0].view(np.uint32)) and np.array_equal(pv.read_phase(), state[1])
    # a NaN in one frame's freq: that bin's phase does not move in that frame, nothing else changes
    c0, f0, k0 = channels - 1, F // 2, 5
    bad = plain_fr.clone()
    bad[c0, f0, k0, 1] = float("nan")
    assert pv.reset() == 0
    sg.buf.fill_(CANARY)
    assert pv.synthesize_device(bad, sp) == 0
    torch.cuda.synchronize()
    assert sg.intact()
    th, new_theta = pm.phases(bad.cpu().numpy()[..., 1], pm.initial_phase(channels, size), hop, SR)
    assert np.array_equal(pv.read_phase(), new_theta)
    assert th[c0, f0, k0] == th[c0, f0 - 1, k0] and new_theta[c0, k0] != state[1][c0, k0]
    got, ref = torch.view_as_real(sp).clone(), torch.view_as_real(plain_sp).clone()
    assert bool(torch.isfinite(got).all())
    want = pm.synth64(bad.cpu().numpy(), th)[c0, f0:, k0]
    assert pm.rel_l2(sp[c0, f0:, k0].cpu().numpy(), want) < 1e-6
    got[c0, f0:, k0] = 0
    ref[c0, f0:, k0] = 0
    assert torch.equal(got, ref), "the NaN reached another bin, channel or an earlier frame"


def test_errors_leave_the_states_alone():
    size, hop, C = 64, 16, 2
    M, F = size // 2, 5
    pv = make(size, hop, C)
    spec = random_spectra(size, C, F, 41)
    fr = analyze(pv, spec)
    synthesize(pv, fr)
    state = (pv.read_prev(), pv.read_phase())

    def untouched(p=pv, st=state):
        return np.array_equal(p.read_prev().view(np.uint32), st[0].view(np.uint32)) and np.array_equal(p.read_phase(), st[1])

    # an output overlapping the input, even partly
    nfr, nsp = C * F * (M + 1) * 2, C * F * M * 2
    buf = torch.zeros(nfr + nsp, device=DEV)
    o_fr = buf[:nfr].view(C, F, M + 1, 2)
    o_sp = torch.view_as_complex(buf[nfr - 2:nfr - 2 + nsp].view(C, F, M, 2))
    assert pv.analyze_device(o_sp, o_fr) == CL_INVALID_VALUE and untouched()
    assert pv.synthesize_device(o_fr, o_sp) == CL_INVALID_VALUE and untouched()
    # a non-contiguous tensor
    wide = torch.zeros((C, F, 2 * M), dtype=torch.complex64, device=DEV)
    assert pv.analyze_device(wide[:, :, ::2], fr) == CL_INVALID_VALUE and untouched()
    assert pv.synthesize_device(torch.zeros((C, F, M + 1, 4), device=DEV)[..., ::2], spec) == CL_INVALID_VALUE and untouched()
    # a wrong bin count, channel count, frame count or dtype
    assert pv.analyze_device(spec, torch.zeros((C, F, M, 2), device=DEV)) == CL_INVALID_VALUE and untouched()
    assert pv.synthesize_device(torch.zeros((C, F, M, 2), device=DEV), spec) == CL_INVALID_VALUE and untouched()
    assert pv.analyze_device(spec[:1].contiguous(), fr[:1].contiguous()) == CL_INVALID_VALUE and untouched()
    assert pv.analyze_device(spec, torch.zeros((C, F + 1, M + 1, 2), device=DEV)) == CL_INVALID_VALUE and untouched()
    assert pv.analyze_device(spec, fr.double()) == CL_INVALID_VALUE and untouched()
    # F == 0: success, nothing happens
    assert pv.analyze_device(spec[:, :0].contiguous(), fr[:, :0].contiguous()) == 0 and untouched()
    assert pv.synthesize_device(fr[:, :0].contiguous(), spec[:, :0].contiguous()) == 0 and untouched()
    # a synthesis under capture before the workspace exists: CL_INVALID_OPERATION, nothing moves
    fresh = make(size, hop, C)
    assert fresh.workspace_bytes() == 0
    st0 = (fresh.read_prev(), fresh.read_phase())
    out = torch.full((C, F, M), 3.0 + 0j, dtype=torch.complex64, device=DEV)
    dummy = torch.zeros(4, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = fresh.synthesize_device(fr, out, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)   # (the graph is not empty)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and fresh.workspace_bytes() == 0 and untouched(fresh, st0)
    assert fresh.synthesize_device(fr, out) == 0 and fresh.workspace_bytes() > 0
    torch.cuda.synchronize()


def test_host_forms_equal_device_forms():
    size, hop, C, F = 256, 64, 2, 70
    pv, ph = make(size, hop, C), make(size, hop, C)
    spec = stft_spectra(size, hop, C, F, 51)
    fr = analyze(pv, spec)
    sp = synthesize(pv, fr)
    h_fr = ph.analyze(spec.cpu().numpy())
    h_sp = ph.synthesize(h_fr)
    assert np.array_equal(h_fr.view(np.uint32), fr.cpu().numpy().view(np.uint32))
    assert np.array_equal(h_sp.view(np.uint32), sp.cpu().numpy().view(np.uint32))
    assert np.array_equal(ph.read_phase(), pv.read_phase())
    one = make(size, hop, 1)
    assert one.analyze(spec[0].cpu().numpy()).shape == (F, size // 2 + 1, 2)
