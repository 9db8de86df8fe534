"""The analysis of a stored signal at given time points on the device (tanal_kernels.hip: k_pvoc_tanal), at all nine
sizes 64 .. 16384.

The call is DEFINED by a composition the library already has: frame (c, g) is frame 1 of Pvoc.analyze_device (a fresh
object) on the two spectra Stft.analyze_device gives for the size + hop samples x_c[starts[g] - hop .. starts[g] + size),
zeros outside the row.  The kernel shares the transform sequence and the per-bin conversion with those two kernels, so
the first test asks for the same BITS, for every frame and bin.

Every case: C = 3 channels of 3 size + 5 samples in guarded rows at a longer, odd stride (the pads hold a NaN), the middle
channel all NaN (its frames are NaN exactly where a window covers a sample of the row: a frame whose windows lie outside
it is silent, as the definition has it); the frames go into a guarded output, every element written.  Fout
(pvoc_tanal_model.fout_for) gives at least seven full groups of the kernel's FPW frames and a ragged one over the 3 Fout
frames, and is no multiple of FPW.  The starts begin with fixed entries — both windows before the row, B and then only A
partly before it, past the end by degrees up to wholly silent, one start three times, a descending run — and go on with
draws from [-size, samples].  One more case puts a row 4 GiB into its buffer: the addresses are 64-bit.

The impulse probe (tests/pvoc_tanal_model.py) gives an analytic float64 truth per frame: where the impulse lies in one
window only, or in neither, the freq is the bin centre to the bit (and the amp +0 unless B holds it); where it lies in
both, every bin is held to bound x 2^-24 x the frame's largest amp, and the distance of dev on the circle of turns to
bound x s_k (pvoc_probe.dev_scale), bound = MARGIN x max(U32, 1), U32 the worst bin of the float32 yardstick tanal32 on
the same inputs against the same truth (capped by tests/test_pvoc_tanal_cpu.py: the reference's error, never the device's).

MARGIN (tests/pvoc_tanal_model.py).  The rule of tests/test_gpu_pvoc_bins.py: the smallest of 2, 4, 8 that clears, by a
factor 1.5, the largest ratio worst / max(U32, 1) over the cases of this file on the device.  Every case prints its ratios
(`PVOCTANAL ...` lines, pytest -s); profiles/pvoc_tanal_bins.txt holds a device run's.
MEASURED over the 27 probe cases on an MI355X (nine sizes; hops size / 4, 3 and size / 4 + 1), in the units above:
  amp   the device's worst bin 2.94 .. 7.11 against the yardstick's 3.10 .. 7.11; ratio 0.74 .. 1.55, the largest at size
        4096, hop 3: 5.82 at channel 0, frame 7, bin 1131 against 3.76.  Both are transforms of one impulse, log2(size)
        roundings deep, in different orders (the device's radix-16 passes, the reference's radix-2 ones);
  dev   0.00 .. 0.75 against 0.00 .. 0.71; the yardstick stays below 1, so the ratio is the device's value: at most 0.75,
        at sizes 8192 and 16384, hop 3.
The largest ratio of all is 1.55, and 1.55 x 1.5 = 2.33 is above 2 and below 4, so MARGIN is 4.  Every other test of the
file asks for bits.  The 71 cases take 3.5 s together.
"""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from opencl_fft_amd._base import CL_INVALID_VALUE
from tests import pvoc_probe as pp
from tests import pvoc_tanal_model as tm
from tests import stft_model
from tests.gpu_guard import CANARY, bits, dev, flat, rows
from tests.pvoc_inputs import analyse_device, hann, make_pvoc, two_tones

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR = pp.SR
C = 3
f32 = np.float32
RATIO = {"max": 0.0, "case": ""}
_WANT = {}


def hops_and_windows(size):
    return {"hann": (size // 4, hann(size)), "int3": (3, tm.int_window(size)), "int+1": (size // 4 + 1, tm.int_window(size))}


def tones(size, channels=C):
    """(channels, 3 size + 5) float32: two_tones in the outer channels, the middle one all NaN"""
    n = tm.samples_of(size)
    x = two_tones(size, 1, channels, n - size + 1, [size, 5]).astype(f32)
    assert x.shape == (channels, n)
    if channels == 3:
        x[1] = np.nan
    return x


def guarded_signal(x):
    """the rows at a longer, odd stride; the pads keep the canary, a NaN"""
    n = x.shape[1]
    g = rows(x.shape[0], n, n + 8).fill(x)
    assert g.data.stride(0) % 2 == 1 and np.isnan(np.array([CANARY], np.int32).view(f32))[0]
    return g


def run(pv, sig, w, starts, what):
    """one guarded device call: the frames (C, Fout, M + 1, 2) as numpy; the inputs unchanged"""
    dw, ds = dev(w), dev(starts)
    out = flat((pv.channels, len(starts), pv.M + 1, 2))
    assert pv.tanal_device(sig.data, dw, ds, out.data) == 0, what
    torch.cuda.synchronize()
    assert out.intact(), what + ": wrote outside the output"
    assert not out.unwritten(), what + ": an output element was not written"
    assert sig.unchanged(), what + ": the signal changed"
    assert np.array_equal(dw.cpu().numpy(), w) and np.array_equal(ds.cpu().numpy(), starts), what + ": an input changed"
    return out.data.cpu().numpy()


def composition(x, w, starts, size, hop):
    """the definition, on the device: the slices of the clean rows x built on the host, Stft.analyze_device, a fresh
    Pvoc(channels = rows x Fout).analyze_device, frame 1 -> (rows, Fout, M + 1, 2) numpy"""
    R, Fout, M = x.shape[0], len(starts), size // 2
    sl = tm.slices(x, starts, size, hop).reshape(R * Fout, size + hop)
    st = fa.Stft(0, size, hop, window=w)
    assert st.get_error() == 0 and st.frames(size + hop) == 2
    spec = torch.zeros((R * Fout, 2, M), dtype=torch.complex64, device=DEV)
    assert st.analyze_device(dev(sl), spec) == 0
    fr = torch.zeros((R * Fout, 2, M + 1, 2), device=DEV)
    assert fa.Pvoc(0, size, hop, SR, R * Fout).analyze_device(spec, fr) == 0
    torch.cuda.synchronize()
    return fr[:, 1].reshape(R, Fout, M + 1, 2).cpu().numpy()


def case(size, which):
    """(hop, w, starts, x, the composition's frames of channels 0 and 2), computed once"""
    if (size, which) not in _WANT:
        hop, w = hops_and_windows(size)[which]
        starts = tm.starts_for(size, hop, tm.fout_for(size))
        x = tones(size)
        want = composition(x[[0, 2]], w, starts, size, hop)
        want.setflags(write=False)
        _WANT[(size, which)] = (hop, w, starts, x, want)
    return _WANT[(size, which)]


def check_frames(got, want, what, starts, size, hop):
    """channels 0 and 2 against the composition, bit for bit; the NaN channel: a NaN reaches exactly the frames whose
    windows cover a sample of the row — the amp where B does, the freq where A or B does — and the others are silent at
    their bin centres"""
    assert np.isfinite(got[[0, 2]]).all(), what + ": channels 0 and 2 are finite"
    n, s = tm.samples_of(size), np.asarray(starts, np.int64)
    b_in, a_in = (s + size > 0) & (s < n), (s - hop + size > 0) & (s - hop < n)
    amp, freq = got[1, :, :, 0], got[1, :, :, 1]
    assert np.isnan(amp[b_in]).all() and np.isnan(freq[a_in | b_in]).all(), what + ": the NaN channel is NaN where a window covers it"
    assert not bits(amp[~b_in]).any(), what + ": the NaN channel is silent where B lies outside the row"
    out = ~(a_in | b_in)
    assert np.array_equal(bits(freq[out]), bits(np.broadcast_to(tm.centre(size, SR), freq[out].shape))), what + ": the bin centres"
    wrong = np.argwhere(bits(got[[0, 2]]) != bits(want))
    assert wrong.size == 0, "%s: %d values differ from the composition, the first at channel %d frame %d (start %d) bin %d %s" \
        % (what, len(wrong), 2 * wrong[0][0], wrong[0][1], starts[wrong[0][1]], wrong[0][2], ("amp", "freq")[wrong[0][3]])


@pytest.mark.parametrize("which", ["hann", "int3", "int+1"])
@pytest.mark.parametrize("size", pp.SIZES)
def test_the_bits_of_the_composition(size, which):
    hop, w, starts, x, want = case(size, which)
    fpw = stft_model.fpw(size)
    assert C * len(starts) >= 7 * fpw + 1 and (fpw == 1 or (len(starts) % fpw and (C * len(starts)) % fpw))
    what = "size %d hop %d %s" % (size, hop, which)
    pv = make_pvoc(size, hop, C)
    assert pv.tanal_kernel_name() == "k_pvoc_tanal"
    prev, phase = pv.read_prev(), pv.read_phase()
    got = run(pv, guarded_signal(x), w, starts, what)
    check_frames(got, want, what, starts, size, hop)
    assert np.array_equal(bits(pv.read_prev()), bits(prev)) and np.array_equal(pv.read_phase(), phase), what + ": a state changed"


@pytest.mark.parametrize("size", pp.SIZES)
def test_the_grid_cap_changes_nothing(size, monkeypatch):
    hop, w, starts, x, want = case(size, "hann")
    capped = make_pvoc(size, hop, C, env={"CLFA_PVOC_OPS_GRID_MAX": 2}, monkeypatch=monkeypatch)
    check_frames(run(capped, guarded_signal(x), w, starts, "size %d capped" % size), want, "size %d, two workgroups" % size, starts, size, hop)


@pytest.mark.parametrize("size", [64, 1024, 16384])
def test_on_the_hop_grid_it_is_the_stft_route(size):
    """starts = g hop: every frame g >= 1 is the frame Stft + Pvoc.analyze return for the whole signal"""
    hop = size // 4
    x = tones(size, 2)
    whole = analyse_device(x, size, hop)
    F = whole.shape[1]
    starts = (np.arange(F) * hop).astype(np.int32)
    pv = make_pvoc(size, hop, 2)
    got = run(pv, guarded_signal(x), hann(size), starts, "size %d hop grid" % size)
    wrong = np.argwhere(bits(got[:, 1:]) != bits(whole[:, 1:]))
    assert wrong.size == 0, "size %d: %d values differ, the first at channel %d frame %d bin %d" \
        % (size, len(wrong), wrong[0][0], wrong[0][1] + 1, wrong[0][2])
    assert not np.array_equal(bits(got[:, 0]), bits(whole[:, 0]))     # frame 0: the earlier window lies before the signal


@pytest.mark.parametrize("hopk", ["quarter", "3", "quarter+1"])
@pytest.mark.parametrize("size", pp.SIZES)
def test_the_impulse_probe_against_float64(size, hopk):
    hop = {"quarter": size // 4, "3": 3, "quarter+1": size // 4 + 1}[hopk]
    n, w = tm.samples_of(size), tm.int_window(size)
    starts = tm.starts_for(size, hop, tm.fout_for(size))
    x = np.full((C, n), np.nan, f32)
    probes = {}
    for ch in (0, 2):
        x[ch], pos, amps = tm.impulse_row(size, hop, n, ch)
        probes[ch] = (pos, amps)
    got = run(make_pvoc(size, hop, C), guarded_signal(x), w, starts, "size %d hop %d probe" % (size, hop))
    centre = tm.centre(size, SR)
    worst = {"amp": 0.0, "dev": 0.0}
    u32 = {"amp": 0.0, "dev": 0.0}
    where = {}
    for ch in (0, 2):
        pos, amps = probes[ch]
        amp64, dev64, _, kind = tm.impulse_truth(size, hop, SR, w, pos, amps, starts)
        assert (kind == tm.BOTH).sum() >= 3
        fr = got[ch]
        for g in np.nonzero(kind != tm.BOTH)[0]:
            at = "size %d channel %d frame %d start %d" % (size, ch, g, starts[g])
            bad = np.nonzero(bits(fr[g, :, 1]) != bits(centre))[0]
            assert bad.size == 0, "%s bin %d: freq %r is not the bin centre %r" % (at, bad[0], fr[g, bad[0], 1], centre[bad[0]])
            if kind[g] != tm.B_ONLY:
                bad = np.nonzero(bits(fr[g, :, 0]))[0]
                assert bad.size == 0, "%s bin %d: amp %r is not +0" % (at, bad[0], fr[g, bad[0], 0])
        e_dev = tm.probe_errors(fr, amp64, dev64, kind, size, hop, SR)
        e_f32 = tm.probe_errors(tm.tanal32(x[ch][None, :], w, starts, size, hop, SR)[0], amp64, dev64, kind, size, hop, SR)
        for q in worst:
            if e_dev[q][0] >= worst[q]:
                worst[q], where[q] = e_dev[q][0], (ch,) + e_dev[q][1]
            u32[q] = max(u32[q], e_f32[q][0])
    line = "PVOCTANAL size %d hop %d:" % (size, hop)
    for q in ("amp", "dev"):
        ratio = worst[q] / max(u32[q], 1.0)
        if ratio > RATIO["max"]:
            RATIO["max"], RATIO["case"] = ratio, "size %d hop %d %s" % (size, hop, q)
        line += "  %s %.2f at %s (float32 yardstick %.2f, ratio %.2f)" % (q, worst[q], where[q], u32[q], ratio)
    print(line + "  [largest ratio so far %.2f, %s]" % (RATIO["max"], RATIO["case"]))
    for q in ("amp", "dev"):
        assert u32[q] <= tm.CAPS_TANAL[q], "size %d hop %d: the yardstick's own %s error %.2f widens the bound" % (size, hop, q, u32[q])
        ch, g, k = where[q]
        assert worst[q] <= pp.bound(tm.MARGIN, u32[q]), \
            "size %d channel %d frame %d start %d bin %d: %s %.2f against %.2f of the float32 yardstick" \
            % (size, ch, g, starts[g], k, q, worst[q], u32[q])


@pytest.mark.parametrize("size", [64, 2048, 16384])
def test_the_host_form_and_a_captured_call(size):
    hop, w, starts, x, want = case(size, "hann")
    pv = make_pvoc(size, hop, C)
    host = pv.tanal(x, w, starts)
    check_frames(host, want, "size %d host form" % size, starts, size, hop)
    one = make_pvoc(size, hop, 1)
    assert np.array_equal(bits(one.tanal(x[0], w, starts)), bits(want[0]))
    sig, dw, ds = guarded_signal(x), dev(w), dev(starts)
    out = torch.zeros((C, len(starts), size // 2 + 1, 2), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert pv.tanal_device(sig.data, dw, ds, out) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pv.tanal_device(sig.data, dw, ds, out) == 0
    for turn in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        check_frames(out.cpu().numpy(), want, "size %d replay %d" % (size, turn), starts, size, hop)


def test_a_row_that_starts_four_gib_into_the_buffer():
    """64-bit addressing: two rows of 2^30 + 1 samples; the tail of the second, past byte 2^33, holds the only sound"""
    size, hop = 256, 64
    M, n, R = size // 2, 2 ** 30 + 1, 4 * size
    w = hann(size)
    region = two_tones(size, 1, 1, R - size + 1, [size, 9]).astype(f32)
    assert region.shape == (1, R)
    buf = torch.zeros(2 * (n + 2), device=DEV)
    x = buf.view(2, n + 2)[:, :n]
    x[1, n - R:] = dev(region[0])
    starts = np.concatenate([n - R + np.arange(-size, R + size, 37), [n - 1, n, n - size]]).astype(np.int32)
    out = flat((2, len(starts), M + 1, 2))
    assert make_pvoc(size, hop, 2).tanal_device(x, dev(w), dev(starts), out.data) == 0
    torch.cuda.synchronize()
    assert out.intact() and not out.unwritten()
    got = out.data.cpu().numpy()
    want = composition(region, w, starts - (n - R), size, hop)      # the row is silent before the region
    assert np.array_equal(bits(got[1]), bits(want[0]))
    assert not bits(got[0, :, :, 0]).any() and np.array_equal(bits(got[0, :, :, 1]), bits(np.broadcast_to(tm.centre(size, SR), got[0, :, :, 1].shape)))
    del x, buf
    torch.cuda.empty_cache()


def test_refusals_write_nothing():
    size, hop, Fout = 256, 64, 9
    M, n = size // 2, tm.samples_of(size)
    pv = make_pvoc(size, hop, C)
    L = fa.lib()
    sig = guarded_signal(tones(size))
    stride = sig.data.stride(0)
    dw, ds = dev(hann(size)), dev(tm.starts_for(size, hop, 15)[:Fout])
    out = flat((C, Fout, M + 1, 2))
    p = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream

    def call(x=p(sig.data), st=stride, n=n, w=p(dw), s=p(ds), o=p(out.data), F=Fout):
        return L.clfa_pvoc_tanal_dev(pv._h, x, st, n, w, s, o, F, stream)

    refused = [dict(x=None), dict(w=None), dict(s=None), dict(o=None),                       # NULL pointers
               dict(x=p(sig.data) + 2), dict(w=p(dw) + 2), dict(s=p(ds) + 1), dict(o=p(out.data) + 4),   # misaligned ones
               dict(n=0), dict(n=-5), dict(st=n - 1), dict(F=-1)]
    for kw in refused:
        assert call(**kw) == CL_INVALID_VALUE, kw
    # the output over the inputs: tensors that hold both
    frames = C * Fout * (M + 1) * 2
    both = torch.zeros(C * stride + frames + 64, device=DEV)
    base = p(both) + (-p(both)) % 8
    pad0 = base + 4 * (n + 1) + (4 * (n + 1)) % 8                       # inside the pad behind row 0 (8 floats wide)
    assert 4 * n <= pad0 - base < 4 * stride
    assert call(x=base, o=pad0) == CL_INVALID_VALUE                      # ... which no window ever reads
    assert call(x=base, o=base + 4 * ((C - 1) * stride + n) - 8 + (4 * ((C - 1) * stride + n)) % 8) == CL_INVALID_VALUE
    assert call(w=base, o=base + 4 * size - 8) == CL_INVALID_VALUE and call(s=base, o=base + 4 * Fout - 4) == CL_INVALID_VALUE
    assert call(w=base + 8 * frames, o=base + 8 * frames - 4 * frames + 8) == CL_INVALID_VALUE   # the output's end in the window
    # Python: a wrong dtype or shape
    assert pv.tanal_device(sig.data.double(), dw, ds, out.data) == CL_INVALID_VALUE
    assert pv.tanal_device(sig.data, dw, ds.long(), out.data) == CL_INVALID_VALUE
    assert pv.tanal_device(sig.data, dw[:-1], ds, out.data) == CL_INVALID_VALUE
    assert pv.tanal_device(sig.data[:2], dw, ds, out.data) == CL_INVALID_VALUE
    assert pv.tanal_device(sig.data, dw, ds[:-1], out.data) == CL_INVALID_VALUE
    assert pv.tanal_device(sig.data, dw, ds, out.data[..., :1]) == CL_INVALID_VALUE
    # no frames: success, and nothing written either
    assert call(F=0) == 0 and call(F=0, x=None, w=None, s=None, o=None) == 0
    empty = torch.zeros((C, 0, M + 1, 2), device=DEV)
    assert pv.tanal_device(sig.data, dw, ds[:0], empty) == 0
    torch.cuda.synchronize()
    assert out.untouched(), "a refused call wrote to the output"
    assert sig.unchanged() and not both.any()
    # the same call, accepted
    assert call() == 0
    torch.cuda.synchronize()
    assert out.intact() and not out.unwritten()
