"""The oscillator bank on the device (clfa_pvoc_adsyn, pvoc_adsyn.hip) against the restatement of its definition
(tests/pvoc_adsyn_model.py): the integer state exactly after every call, the samples bit for bit however the frames are
cut into calls, on a side stream, under graph replay and for another grid cap; exact per-sample probes whose expected
values are float32 numbers whatever the order of the sum; and the samples within MARGIN of the float32 model's own error
against the float64 truth.

MARGIN.  The device's cospif is not numpy's cos, so equality with the float32 model is not the contract; the contract is a
relative L2 error against float64 of at most MARGIN times the float32 model's error on the same inputs.  The rule for its
value is the project's (tests/test_gpu_pvoc.py): the smallest of 2, 4, 8 that clears the largest ratio measured over
every case of this file by a factor 1.5.  Measured on an MI355X over every case of this file: ratios 0.21 - 0.98 (the
largest on a call of one frame of three samples, size 64 hop 3 with 3 channels; typically 0.5 - 0.7); 0.98 x 1.5 = 1.47,
so MARGIN = 2.  Every case prints its ratios (`ADSYN ...` lines, pytest -s).  Why the ratios stay below 1: both errors
are dominated by the rounding of the phase's top 32 bits to a float32 number of half turns, which the two share; numpy
then rounds the product with pi, cospif does not.
"""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from tests import pvoc_adsyn_model as am
from tests import gpu_guard
from tests.gpu_guard import DEV
from tests.pvoc_inputs import SR, analyse_device, make_pvoc, two_tones

pytestmark = pytest.mark.gpu
MARGIN = 2.0
CL_INVALID_VALUE, CL_INVALID_OPERATION = -30, -59
f32 = np.float32
RATIO = {"max": 0.0}


def make(size, hop, channels=1, sr=SR):
    pv = make_pvoc(size, hop, channels, sr)
    assert pv.adsyn_kernel_name() == "k_adsyn_osc"
    return pv


def spoil(fr, rng, sr=SR):
    """about 1 bin in 8 of silent endpoints (Nyquist and above, NaN, infinities), about 1 in 8 of zero amps, a few
    negative frequencies"""
    C, F, B, _ = fr.shape
    u = rng.random((C, F, B))
    bad = np.array([sr / 2, -sr / 2, sr, np.nan, np.inf, -np.inf, 3e38], f32)
    fr[..., 1] = np.where(u < 0.125, bad[rng.integers(0, bad.size, (C, F, B))], fr[..., 1])
    fr[..., 0] = np.where((u >= 0.125) & (u < 0.25), f32(0), fr[..., 0])
    neg = (u >= 0.25) & (u < 0.27)
    fr[..., 1] = np.where(neg, -fr[..., 1], fr[..., 1])
    return fr


def random_frames(size, C, F, seed, sr=SR):
    rng = np.random.default_rng(seed)
    B = size // 2 + 1
    amp = np.abs(rng.standard_normal((C, F, B))).astype(f32)
    freq = (np.arange(B) * (sr / size) + rng.standard_normal((C, F, B)) * sr / size).astype(f32)
    return spoil(np.stack([amp, freq], axis=-1), rng, sr)


def analysed_frames(size, hop, C, F, seed):
    """Stft and Pvoc.analyze on the device, of noise plus two sinusoids (one between bins, one near Nyquist)"""
    rng = np.random.default_rng(seed)
    fr = analyse_device(two_tones(size, hop, C, F, rng), size, hop)
    assert fr.shape[1] == F
    return spoil(fr, rng)


def run(pv, fr_t, fmod=None, sel=(0, None, 1), gain=1.0, stream=None):
    C, F = fr_t.shape[:2]
    out = torch.zeros((C, F * pv.hop), device=DEV)
    assert pv.adsyn_device(fr_t, out, fmod=fmod, first_bin=sel[0], nbins=sel[1], step=sel[2], gain=gain, stream=stream) == 0
    return out


def state_equal(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def picked(seg, frames):
    return {k: (v if k == "hop" else v[:, frames]) for k, v in seg.items()}


def accuracy(what, y, seg, gain=1.0, budget=6e6):
    """relative L2 of the device's samples against float64 beside the float32 model's, on every frame of the call or — where
    the model would take too long — on its first two, middle and last two frames"""
    C, F, nb = seg["A0"].shape
    hop = seg["hop"]
    frames = np.arange(F)
    if C * F * hop * nb > budget:
        frames = np.unique(np.clip([0, 1, F // 2, F - 2, F - 1], 0, F - 1))
    part = picked(seg, frames)
    got = y.reshape(C, F, hop)[:, frames].reshape(C, -1)
    truth = am.samples64(part, gain)
    e_dev, e_f32 = am.rel_l2(got, truth), am.rel_l2(am.samples32(part, gain), truth)
    ratio = e_dev / max(e_f32, 1e-300)
    RATIO["max"] = max(RATIO["max"], ratio)
    print("ADSYN %s: relL2 %.3g (float32 model %.3g, ratio %.2f; largest so far %.2f)" % (what, e_dev, e_f32, ratio, RATIO["max"]))
    assert np.isfinite(truth).all() and e_f32 > 0
    assert e_dev <= MARGIN * e_f32, "%s: %.3g against %.3g" % (what, e_dev, e_f32)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size,hop", [(64, 16), (64, 3), (64, 64), (1024, 256)])
def test_state_bits_and_accuracy(size, hop, channels, monkeypatch):
    """one object fed calls of every frame count around the scan's chunk: the state equals the integer model's after every
    call and the samples pass the accuracy rule; the same frames in ONE call on an object with another grid cap, the same
    calls on a side stream, and the same calls in one replayed graph give the same bits"""
    pv = make(size, hop, channels)
    ch = pv.scan_chunk()
    Fs = [1, 2, ch - 1, ch, ch + 1, 2 * ch + 3]
    state = am.initial_state(channels, size)
    assert state_equal(pv.adsyn_state(), state) and pv.adsyn_workspace_bytes() == 0
    parts, outs = [], []
    for i, F in enumerate(Fs):
        kind = "analysed" if i % 2 else "random"
        fr = analysed_frames(size, hop, channels, F, size + F) if i % 2 else random_frames(size, channels, F, size + F)
        fr_t = torch.from_numpy(fr).to(DEV)
        y = run(pv, fr_t)
        torch.cuda.synchronize()
        seg, state = am.segments(fr, state, hop, SR)
        what = "size %d hop %d ch %d F %d %s" % (size, hop, channels, F, kind)
        assert state_equal(pv.adsyn_state(), state), what
        accuracy(what, y.cpu().numpy(), seg)
        parts.append(fr_t)
        outs.append(y)
    assert pv.adsyn_workspace_bytes() > 0 and pv.workspace_bytes() == 0
    want = torch.cat(outs, dim=1)
    # one call, another grid cap (the switch is read at creation)
    monkeypatch.setenv("CLFA_PVOC_ADSYN_GRID_MAX", "3")
    one = make(size, hop, channels)
    monkeypatch.delenv("CLFA_PVOC_ADSYN_GRID_MAX")
    assert torch.equal(run(one, torch.cat(parts, dim=1).contiguous()), want), "one call, grid cap 3"
    assert state_equal(one.adsyn_state(), state)
    # the same calls on a side stream
    assert one.reset() == 0 and state_equal(one.adsyn_state(), am.initial_state(channels, size))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = torch.cat([run(one, p) for p in parts], dim=1)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and state_equal(one.adsyn_state(), state), "side stream"
    # ... and captured into one graph, replayed once (the workspace exists by now)
    assert one.reset() == 0
    bufs = [torch.zeros_like(o) for o in outs]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for p, b in zip(parts, bufs):
            assert one.adsyn_device(p, b) == 0
    assert one.reset() == 0     # (whatever the capture itself did to the state)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(bufs, dim=1), want) and state_equal(one.adsyn_state(), state), "graph replay"


def test_sub_batches_of_one_chunk(monkeypatch):
    size, hop, C = 64, 16, 2
    pv = make(size, hop, C)
    F = 3 * pv.scan_chunk() + 5
    fr = random_frames(size, C, F, 77)
    fr_t = torch.from_numpy(fr).to(DEV)
    fmod = torch.from_numpy(np.random.default_rng(78).uniform(0.5, 2, F).astype(f32)).to(DEV)
    want = run(pv, fr_t, fmod=fmod)
    monkeypatch.setenv("CLFA_PVOC_CHUNKS_MAX", "1")
    small = make(size, hop, C)
    monkeypatch.delenv("CLFA_PVOC_CHUNKS_MAX")
    assert torch.equal(run(small, fr_t, fmod=fmod), want) and state_equal(small.adsyn_state(), pv.adsyn_state())
    assert 0 < small.adsyn_workspace_bytes() < pv.adsyn_workspace_bytes()


def test_scan_with_several_chunks_per_segment(monkeypatch):
    """34 chunks (33 whole ones and one of 5 frames) in one call: k_adsyn_scan's waves take 3 chunks each, the last occupied
    segment is short and the segments after it are empty.  The state is the integer model's; samples and state are the bits
    of the same frames cut into two calls and of sub-batches of 5 chunks (other segment lengths)"""
    size, hop, C, sel = 64, 3, 2, (1, None, 2)
    pv = make(size, hop, C)
    ch = pv.scan_chunk()
    F = 33 * ch + 5
    fr = random_frames(size, C, F, 81)
    fm = np.random.default_rng(82).uniform(0.5, 2, F).astype(f32)
    fr_t, fmod = torch.from_numpy(fr).to(DEV), torch.from_numpy(fm).to(DEV)
    want = run(pv, fr_t, fmod=fmod, sel=sel)
    torch.cuda.synchronize()
    _, state = am.segments(fr, am.initial_state(C, size), hop, SR, fm, am.selection(size // 2, *sel))
    assert state_equal(pv.adsyn_state(), state), "state after one call of 34 chunks"
    cut = ch * 17 + 1
    assert pv.reset() == 0
    parts = [run(pv, fr_t[:, a:b].contiguous(), fmod=fmod[a:b].contiguous(), sel=sel) for a, b in ((0, cut), (cut, F))]
    assert torch.equal(torch.cat(parts, dim=1), want) and state_equal(pv.adsyn_state(), state), "cut at 17 chunks + 1"
    monkeypatch.setenv("CLFA_PVOC_CHUNKS_MAX", "5")
    small = make(size, hop, C)
    monkeypatch.delenv("CLFA_PVOC_CHUNKS_MAX")
    assert torch.equal(run(small, fr_t, fmod=fmod, sel=sel), want) and state_equal(small.adsyn_state(), state), "sub-batches of 5 chunks"
    assert 0 < small.adsyn_workspace_bytes() < pv.adsyn_workspace_bytes()


# ---- exact per-sample probes ------------------------------------------------------------------------------------------

PSR = 32768.0
COS_QUARTER = np.array([1.0, 0.0, -1.0, 0.0])


def probe_expected(seg, gain):
    """the samples of segments whose phases are whole quarter turns and whose amplitudes are small integers: every term
    and every partial sum is a float32 number, so the sum's order does not matter"""
    hop = seg["hop"]
    C, F, nb = seg["A0"].shape
    y = np.zeros((C, F, hop))
    w = (np.arange(1, hop + 1) / hop)[None, :, None]
    for f in range(F):
        ph = am._frame_phase(seg, f)
        assert not (ph & np.uint64((1 << 62) - 1)).any()
        a0, a1 = seg["A0"][:, f, None, :].astype(np.float64), seg["A1"][:, f, None, :].astype(np.float64)
        y[:, f] = ((a0 + (a1 - a0) * w) * COS_QUARTER[(ph >> np.uint64(62)).astype(np.int64)]).sum(axis=-1)
    y = gain * y.reshape(C, F * hop)
    assert np.array_equal(np.nan_to_num(y.astype(f32).astype(np.float64)), np.nan_to_num(y))     # exact in float32
    return y.astype(f32)


def probe_sizes():
    tile = fa.Pvoc(0, 64, 16, PSR).adsyn_tile_bins()
    big = 64
    while big // 2 + 1 <= tile:
        big *= 2
    return tile, big


@pytest.mark.parametrize("pattern", ["dc", "quarter"])
@pytest.mark.parametrize("case", ["64-all", "64-sparse", "64-last", "256-all", "256-sparse", "256-last", "tiles"])
def test_exact_probe(case, pattern):
    tile, big = probe_sizes()
    size = {"64": 64, "256": 256, "tiles": big}[case.split("-")[0]]
    hop = size // 4
    M = size // 2
    sel = {"all": (0, M + 1, 1), "sparse": (1, 5, 3), "last": (M, 1, 1), "tiles": (0, M + 1, 1)}[case.split("-")[-1]]
    if case == "tiles":
        assert M + 1 > tile, "the selection spans more than one LDS tile of k_adsyn_osc"
    C, gain = 3, 0.5
    pv = make(size, hop, C, PSR)
    ch = pv.scan_chunk()
    bins = am.selection(M, *sel)
    rng = np.random.default_rng(size + len(case))
    freq = f32(0.0 if pattern == "dc" else 8192.0)

    def frames(F, nan_outside):
        fr = np.zeros((C, F, M + 1, 2), f32)
        fr[..., 0] = rng.integers(0, 8, (C, F, M + 1)).astype(f32)
        fr[..., 1] = freq
        fr[1, ..., 0] = np.nan                      # the channel between the real ones: NaN amps, and NaN freqs in odd bins
        fr[1, :, 1::2, 1] = np.nan
        if nan_outside:
            outside = np.setdiff1d(np.arange(M + 1), bins)
            fr[:, :, outside, 0] = np.nan
        return fr

    # a priming call on every bin, so that every bin has a state to keep
    prime = frames(2, False)
    run(pv, torch.from_numpy(prime).to(DEV), gain=gain)
    _, state = am.segments(prime, am.initial_state(C, size), hop, PSR)
    assert state_equal(pv.adsyn_state(), state)
    for F in [1, ch + 2, 3]:
        fr = frames(F, True)
        n, stride = F * hop, F * hop + 5
        g = gpu_guard.rows(C, n, stride, misalign=1)
        rows = g.data
        assert pv.adsyn_device(torch.from_numpy(fr).to(DEV), rows, first_bin=sel[0], nbins=sel[1], step=sel[2], gain=gain) == 0
        torch.cuda.synchronize()
        assert g.intact(), "wrote outside the output rows"
        assert not g.unwritten(), "left an output sample unwritten"
        seg, new = am.segments(fr, state, hop, PSR, None, bins)
        want = probe_expected(seg, gain)
        got = rows.cpu().numpy()
        assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()     # (every selection holds an even bin)
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s %s F %d: a NaN leaked, or was lost" % (case, pattern, F)
        bad = np.flatnonzero((got != want)[[0, 2]].ravel())
        assert bad.size == 0, "%s %s F %d: %d samples differ, first at %d" % (case, pattern, F, bad.size, bad[0])
        assert np.abs(want[[0, 2]]).max() > 0
        got_state = pv.adsyn_state()
        assert state_equal(got_state, new), "%s %s F %d: state" % (case, pattern, F)
        outside = np.setdiff1d(np.arange(M + 1), bins)
        assert state_equal([a[:, outside] for a in got_state], [a[:, outside] for a in state]), "an unselected bin's state moved"
        state = new


# ---- fmod ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,hop,channels", [(64, 16, 3), (1024, 256, 1)])
def test_fmod(size, hop, channels):
    pv = make(size, hop, channels)
    F = pv.scan_chunk() + 3
    fr = random_frames(size, channels, F, 5 * size)
    fr_t = torch.from_numpy(fr).to(DEV)
    plain = run(pv, fr_t)
    plain_state = pv.adsyn_state()
    assert pv.reset() == 0
    assert torch.equal(run(pv, fr_t, fmod=torch.ones(F, device=DEV)), plain), "fmod of ones"
    assert state_equal(pv.adsyn_state(), plain_state)
    for m in (0.5, 2.0):
        assert pv.reset() == 0
        y = run(pv, fr_t, fmod=m)
        seg, state = am.segments(fr, am.initial_state(channels, size), hop, SR, np.full(F, m, f32))
        assert state_equal(pv.adsyn_state(), state), m
        accuracy("size %d fmod %g" % (size, m), y.cpu().numpy(), seg)
    # a NaN entry silences that frame's endpoints only: the frames before it are the plain call's, bit for bit; the state
    # is the model's (the frame after starts from silence at its own frequency)
    f0 = F // 2
    fm = np.ones(F, f32)
    fm[f0] = np.nan
    assert pv.reset() == 0
    y = run(pv, fr_t, fmod=torch.from_numpy(fm).to(DEV))
    seg, state = am.segments(fr, am.initial_state(channels, size), hop, SR, fm)
    assert state_equal(pv.adsyn_state(), state)
    assert torch.equal(y[:, :f0 * hop], plain[:, :f0 * hop]) and bool(torch.isfinite(y).all())
    assert not seg["A1"][:, f0].any() and not seg["A0"][:, f0 + 1].any() and seg["A1"][:, f0 + 1].any()
    assert bool((y[:, (f0 + 1) * hop - 1] == 0).all()), "the silenced frame ends at amplitude 0"
    accuracy("size %d fmod with a NaN" % size, y.cpu().numpy(), seg)


# ---- errors, capture, reset, host form ----------------------------------------------------------------------------

def test_errors_capture_and_reset():
    size, hop, C, F = 64, 16, 2, 5
    M = size // 2
    pv = make(size, hop, C)
    fr_t = torch.from_numpy(random_frames(size, C, F, 91)).to(DEV)
    run(pv, fr_t)
    state = pv.adsyn_state()
    assert state[0].any() and state[1].any() and state[2].any()
    untouched = lambda p=pv, st=state: state_equal(p.adsyn_state(), st)
    # an output overlapping the frames or fmod, even partly
    nfr = C * F * (M + 1) * 2
    buf = torch.zeros(nfr + C * F * hop + F, device=DEV)
    o_fr = buf[:nfr].view(C, F, M + 1, 2)
    o_fr.copy_(fr_t)
    assert pv.adsyn_device(o_fr, buf[nfr - 2:nfr - 2 + C * F * hop].view(C, F * hop)) == CL_INVALID_VALUE and untouched()
    o_out = buf[nfr:nfr + C * F * hop].view(C, F * hop)
    o_fm = buf[nfr + C * F * hop - 1:nfr + C * F * hop - 1 + F]
    assert pv.adsyn_device(o_fr, o_out, fmod=o_fm) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(o_fr, o_out, fmod=buf[nfr + C * F * hop:]) == 0
    assert pv.reset() == 0 and run(pv, fr_t) is not None and untouched()
    # sizes the wrong way round, wrong shapes and types
    out = torch.zeros((C, F * hop), device=DEV)
    assert pv.adsyn_device(fr_t, out[:, :F * hop - 1]) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out[:1]) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t[:, :, :M].contiguous(), out) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out.double()) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out, fmod=torch.ones(F + 1, device=DEV)) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out, step=0) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out, first_bin=1, nbins=M + 1) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t, out, nbins=0) == CL_INVALID_VALUE and untouched()
    assert pv.adsyn_device(fr_t[:, :0].contiguous(), out[:, :0]) == 0 and untouched()
    # the first call under capture: CL_INVALID_OPERATION, nothing moves
    fresh = make(size, hop, C)
    assert fresh.adsyn_workspace_bytes() == 0
    out.fill_(3.0)
    dummy = torch.zeros(4, device=DEV)
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = fresh.adsyn_device(fr_t, out, stream=torch.cuda.current_stream().cuda_stream)
        dummy.add_(1.0)   # (the graph is not empty)
    assert rc == CL_INVALID_OPERATION
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and fresh.adsyn_workspace_bytes() == 0
    assert state_equal(fresh.adsyn_state(), am.initial_state(C, size))
    # a capture after a warm call replays, and advances the state like a call
    first = run(fresh, fr_t)
    ws = fresh.adsyn_workspace_bytes()
    assert ws > 0 and untouched(fresh)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        assert fresh.adsyn_device(fr_t, out) == 0
    assert fresh.reset() == 0
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first) and untouched(fresh)
    g2.replay()
    torch.cuda.synchronize()
    second = run(pv, fr_t)      # pv is one call in: this is its second
    assert torch.equal(out, second) and state_equal(fresh.adsyn_state(), pv.adsyn_state())
    assert fresh.adsyn_workspace_bytes() == ws
    # reset() zeroes the new state; the old states behave as before
    spec = torch.view_as_complex(torch.randn((C, F, M, 2), device=DEV))
    frames = torch.zeros((C, F, M + 1, 2), device=DEV)
    sp = torch.zeros_like(spec)
    assert pv.analyze_device(spec, frames) == 0 and pv.synthesize_device(frames, sp) == 0
    torch.cuda.synchronize()
    theta, prev = pv.read_phase(), pv.read_prev()
    assert theta.any() and state_equal(pv.adsyn_state(), fresh.adsyn_state())       # analysis and synthesis left it alone
    run(pv, fr_t)
    assert np.array_equal(pv.read_phase(), theta) and np.array_equal(pv.read_prev(), prev)   # and the other way round
    assert pv.reset() == 0
    assert state_equal(pv.adsyn_state(), am.initial_state(C, size))
    assert not pv.read_phase().any() and np.array_equal(pv.read_prev(), np.ones((C, M + 1), np.complex64))


def test_host_form_equals_device_form():
    size, hop, C, F = 256, 64, 2, 70
    pv, ph = make(size, hop, C), make(size, hop, C)
    fr = random_frames(size, C, F, 51)
    fm = np.random.default_rng(52).uniform(0.5, 2, F).astype(f32)
    y = run(pv, torch.from_numpy(fr).to(DEV), fmod=torch.from_numpy(fm).to(DEV), sel=(2, 40, 3), gain=0.25)
    h = ph.adsyn(fr, fmod=fm, first_bin=2, nbins=40, step=3, gain=0.25)
    assert h.shape == (C, F * hop) and np.array_equal(h.view(np.uint32), y.cpu().numpy().view(np.uint32))
    assert state_equal(ph.adsyn_state(), pv.adsyn_state())
    one = make(size, hop, 1)
    assert one.adsyn(fr[0]).shape == (F * hop,)
