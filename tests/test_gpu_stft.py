"""Short-time analysis / overlap-add synthesis on the device (clfa_stft, stft_kernels.hip) against the definition in
include/clfft_amd.h: analysis = the oracle's Clrfft forward of the float32 windowed frames, synthesis = a float64
evaluation of the overlap-add formula, and torch.stft(center=False) through packed_to_onesided."""
import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from oracle import oracle
from tests import stft_model, util
from tests.pvoc_inputs import hann

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def analyze_dev(size, hop, x_t, w=None):
    st = fa.Stft(0, size, hop, window=w, fwd=True)
    assert st.get_error() == 0, st.get_log()
    F = st.frames(x_t.shape[1])
    out = torch.zeros((x_t.shape[0], F, size // 2), dtype=torch.complex64, device=DEV)
    assert st.analyze_device(x_t, out) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


def check_analysis(x, size, hop, w, spec):
    frames = stft_model.windowed_frames_f32(x, size, hop, w if w is not None else np.ones(size, np.float32))
    want = oracle.rfft_forward(frames.reshape(-1, size)).reshape(spec.shape)
    util.assert_parity(spec, want, what="stft size %d hop %d" % (size, hop))


@pytest.mark.parametrize("size", [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384])
@pytest.mark.parametrize("hopk", ["1", "3", "q", "h", "s"])
def test_analysis_matches_rfft_of_windowed_frames(size, hopk):
    hop = {"1": 1, "3": 3, "q": size // 4, "h": size // 2, "s": size}[hopk]
    F = 40 if hop < 4 else 9
    samples = size + (F - 1) * hop + hop // 2 + 1 if hop > 1 else size + F - 1    # trailing samples that make no frame
    rng = np.random.default_rng(size * 7 + hop)
    x = (rng.random((3, samples), dtype=np.float32) * 2 - 1)
    w = (rng.random(size, dtype=np.float32) + 0.25).astype(np.float32)
    spec, st = analyze_dev(size, hop, torch.from_numpy(x).to(DEV), w)
    assert spec.shape == (3, st.frames(samples), size // 2)
    check_analysis(x, size, hop, w, spec)
    # bit-identical to the library's Clrfft on the pre-windowed frames?  (expected where the same pass chain runs)
    frames = stft_model.windowed_frames_f32(x, size, hop, w).reshape(-1, size)
    d = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    p = fa.Clrfft(0, size, True)
    assert p.exec_device(d, frames.shape[0]) == 0
    torch.cuda.synchronize()
    same = np.array_equal(d.cpu().numpy().view(np.uint32).reshape(-1), spec.view(np.uint32).reshape(-1))
    print("size %d hop %d: bit-identical to Clrfft(%s) on pre-windowed frames: %s" % (size, hop, p.kernel_name(), same))


@pytest.mark.parametrize("size", [64, 2048])
def test_analysis_200_channels_rectangular(size):
    hop = size // 4
    samples = size + 20 * hop + 3
    x = np.random.default_rng(size).standard_normal((200, samples)).astype(np.float32)
    spec, _ = analyze_dev(size, hop, torch.from_numpy(x).to(DEV))
    check_analysis(x, size, hop, None, spec)


@pytest.mark.parametrize("size,hop,pad,shift", [(1024, 256, 100, 0), (512, 3, 1, 1), (2048, 511, 7, 1), (64, 5, 3, 0)])
def test_analysis_strided_and_4_byte_aligned_rows(size, hop, pad, shift):
    """a view with padded rows (stride from the tensor); odd stride with odd hop; a signal starting 4 bytes into a buffer"""
    C, samples = 3, size + 13 * hop + 2
    stride = samples + pad
    buf = torch.zeros(C * stride + shift + 1, device=DEV)
    x_t = buf[shift:shift + C * stride].view(C, stride)[:, :samples]
    x = np.random.default_rng(hop).standard_normal((C, samples)).astype(np.float32)
    x_t.copy_(torch.from_numpy(x))
    w = hann(size)
    spec, _ = analyze_dev(size, hop, x_t, w)
    check_analysis(x, size, hop, w, spec)


def synth_truth(spec, size, hop, w, normalize):
    """float64: r_f = exact Clrfft inverse (unscaled) of every frame, then the overlap-add formula"""
    # Clrfft forward = packed_to_onesided^-1 of rfft, so its unscaled inverse is irfft of the one-sided bins
    r64 = np.fft.irfft(fa.packed_to_onesided(spec.astype(np.complex128)), n=size, axis=-1)
    return stft_model.overlap_add(r64, w.astype(np.float64), hop, normalize)[0]


def synth_dev(size, hop, spec, w, normalize, stride_pad=0):
    st = fa.Stft(0, size, hop, window=w, fwd=False)
    assert st.get_error() == 0, st.get_log()
    C, F, _ = spec.shape
    L = st.samples(F)
    out = torch.full((C, L + stride_pad), 7.0, device=DEV)
    s_t = torch.from_numpy(spec).to(DEV)
    assert st.synthesize_device(s_t, out[:, :L], normalize=normalize) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    if stride_pad:
        assert np.all(o[:, L:] == 7.0), "synthesis wrote past the row"
    return o[:, :L], st, s_t


@pytest.mark.parametrize("size,hop,C,F", [(64, 16, 3, 50), (256, 3, 2, 300), (1024, 256, 3, 40), (2048, 1, 1, 2100),
                                          (4096, 4096, 2, 5), (8192, 2048, 2, 12), (16384, 4096, 2, 9), (512, 128, 200, 6),
                                          # short calls, fewer frames than size / hop: the envelope's difference form
                                          (2048, 16, 1, 8), (256, 3, 2, 10), (64, 1, 1, 5), (2048, 1, 1, 100),
                                          (1024, 256, 3, 2)])
@pytest.mark.parametrize("normalize", [False, True])
def test_synthesis_at_least_as_accurate_as_float32_numpy(size, hop, C, F, normalize):
    rng = np.random.default_rng(size + hop + F)
    spec = (rng.standard_normal((C, F, size // 2)) + 1j * rng.standard_normal((C, F, size // 2))).astype(np.complex64) / size
    w = hann(size) + np.float32(0.01)
    y, _, _ = synth_dev(size, hop, spec, w, normalize, stride_pad=5)
    truth = synth_truth(spec, size, hop, w, normalize)
    # the float32 numpy composition a user would write: the oracle's Clrfft inverse, window, overlap-add in float32
    r32 = oracle.rfft_inverse(spec.reshape(-1, size // 2)).reshape(C, F, size)
    y32 = stft_model.overlap_add(r32, w, hop, normalize, dtype=np.float32)[0]
    eh, eo = util.rel_err(y, truth), util.rel_err(y32, truth)
    print("synth size %d hop %d norm %d: HIP %.3g / %.3g, float32 numpy %.3g / %.3g" % (size, hop, normalize, *eh, *eo))
    # 2, not the 1.2 of tests/test_gpu_conv_accuracy.py: every case but one is within 1.2 x, but at hop 3 with the
    # envelope division (85 frames per sample) the HIP result is 1.43 / 1.75 x the float32 composition's error (relL2 /
    # max: 1.16e-7 against 8.1e-8 / 6.6e-8); without the division the float32 sums dominate and the two agree
    # (2.02e-7 / 2.03e-7).  Not explained yet; the absolute bound below holds everywhere.
    assert eh[0] <= 2.0 * eo[0] + 1e-9 and eh[1] <= 2.0 * eo[1] + 1e-9, (eh, eo)
    assert eh[0] <= 2e-6 and eh[1] <= 4e-6, eh


@pytest.mark.parametrize("size,hop", [(256, 64), (2048, 512), (16384, 4096)])
def test_synthesis_repeatable_and_graph_replay_bit_identical(size, hop):
    C, F = 4, 40
    rng = np.random.default_rng(size)
    spec = (rng.standard_normal((C, F, size // 2)) + 1j * rng.standard_normal((C, F, size // 2))).astype(np.complex64)
    w = hann(size)
    y1, st, s_t = synth_dev(size, hop, spec, w, True)
    L = st.samples(F)
    out = torch.zeros((C, L), device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert st.synthesize_device(s_t, out, normalize=True) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), y1.view(np.uint32))
    g = torch.cuda.CUDAGraph()
    out.zero_()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        assert st.synthesize_device(s_t, out, normalize=True) == 0
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), y1.view(np.uint32))
    # analysis captured and replayed as well
    x_t = torch.randn((C, 10 * size), device=DEV)
    a = fa.Stft(0, size, hop, window=w)
    sp1 = torch.zeros((C, a.frames(10 * size), size // 2), dtype=torch.complex64, device=DEV)
    sp2 = torch.zeros_like(sp1)
    assert a.analyze_device(x_t, sp1) == 0
    g2 = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g2):
        assert a.analyze_device(x_t, sp2) == 0
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(sp1.view(torch.float32), sp2.view(torch.float32))


@pytest.mark.parametrize("size", [64, 512, 2048, 16384])
def test_round_trip_hann_quarter_hop(size):
    hop = size // 4
    C, samples = 3, 12 * size + 5
    x = np.random.default_rng(size).standard_normal((C, samples)).astype(np.float32)
    w = hann(size)
    spec, _ = analyze_dev(size, hop, torch.from_numpy(x).to(DEV), w)
    y, _, _ = synth_dev(size, hop, spec, w, True)
    L = y.shape[1]
    env = stft_model.overlap_add(np.zeros((1, spec.shape[1], size)), w, hop)[1]
    m = env > 1e-3 * env.max()
    err = np.abs(y[:, m] - x[:, :L][:, m]).max() / np.abs(x[:, :L][:, m]).max()
    assert err <= 1e-5, err


@pytest.mark.parametrize("size,hop", [(256, 64), (2048, 512), (1024, 333)])
def test_analysis_matches_torch_stft(size, hop):
    C, samples = 2, 9 * size + 17
    x = np.random.default_rng(hop).standard_normal((C, samples)).astype(np.float32)
    w = hann(size)
    spec, _ = analyze_dev(size, hop, torch.from_numpy(x).to(DEV), w)
    ref = torch.stft(torch.from_numpy(x).double(), n_fft=size, hop_length=hop, window=torch.from_numpy(w).double(),
                     center=False, onesided=True, return_complex=True).numpy()     # (C, M + 1, F)
    got = fa.packed_to_onesided(spec.astype(np.complex128)).transpose(0, 2, 1)
    assert got.shape == ref.shape
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err <= 2e-6, err


def test_errors_and_no_ops():
    size, hop = 256, 64
    a = fa.Stft(0, size, hop)
    s = fa.Stft(0, size, hop, fwd=False)
    x = torch.randn((1, 4 * size), device=DEV)
    F = a.frames(4 * size)
    spec = torch.zeros((1, F, size // 2), dtype=torch.complex64, device=DEV)
    # wrong direction
    assert s.analyze_device(x, spec) == -30
    assert a.synthesize_device(spec, torch.zeros((1, a.samples(F)), device=DEV)) == -30
    # an output that overlaps the input, even partly
    buf = torch.zeros(4 * size + F * size + 64, device=DEV)
    sig = buf[:4 * size].view(1, -1)
    over = buf[4 * size - 2:4 * size - 2 + F * size].view(torch.complex64).view(1, F, size // 2)
    assert a.analyze_device(sig, over) == -30
    sbuf = torch.zeros(F * size, device=DEV)
    sp_in = sbuf.view(torch.complex64).view(1, F, size // 2)
    assert s.synthesize_device(sp_in, sbuf[: s.samples(F)].view(1, -1)) == -30
    # F = 0 and channels = 0: success, nothing written
    short = torch.randn((2, size - 1), device=DEV)
    untouched = torch.full((2, 1, size // 2), 3.0 + 1j, dtype=torch.complex64, device=DEV)
    assert a.analyze_device(short, untouched) == 0
    torch.cuda.synchronize()
    assert bool((untouched == (3.0 + 1j)).all())
    assert a.analyze_device(torch.zeros((0, 4 * size), device=DEV), spec) == 0
    # host forms equal device forms bit for bit
    xh = np.random.default_rng(5).standard_normal((3, 7 * size + 3)).astype(np.float32)
    w = hann(size)
    a2, s2 = fa.Stft(0, size, hop, window=w), fa.Stft(0, size, hop, window=w, fwd=False)
    host_spec = a2.analyze(xh)
    dev_spec, _ = analyze_dev(size, hop, torch.from_numpy(xh).to(DEV), w)
    assert np.array_equal(host_spec.view(np.uint32), dev_spec.view(np.uint32))
    host_y = s2.synthesize(host_spec, normalize=True)
    dev_y, _, _ = synth_dev(size, hop, host_spec, w, True)
    assert np.array_equal(host_y.view(np.uint32), dev_y.view(np.uint32))


def test_full_size_16_channels_2_22_samples():
    size, hop, C, samples = 2048, 512, 16, 1 << 22
    g = torch.Generator(device=DEV).manual_seed(11)
    x_t = torch.rand((C, samples), device=DEV, generator=g) * 2 - 1
    w = hann(size)
    st = fa.Stft(0, size, hop, window=w)
    F = st.frames(samples)
    out = torch.empty((C, F, size // 2), dtype=torch.complex64, device=DEV)
    assert st.analyze_device(x_t, out) == 0
    torch.cuda.synchronize()
    chans, frames = [0, 7, 15], [0, 1, 2, F // 3, F // 2, F - 2, F - 1]
    x = x_t[chans].cpu().numpy()
    got = out[chans][:, frames].cpu().numpy()
    fr = np.stack([np.stack([x[i, f * hop:f * hop + size] * w for f in frames]) for i in range(len(chans))]).astype(np.float32)
    want = oracle.rfft_forward(fr.reshape(-1, size)).reshape(got.shape)
    util.assert_parity(got, want, what="full size")
