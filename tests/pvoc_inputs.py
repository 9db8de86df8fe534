"""The frame inputs of the Pvoc tests, in one place: the Hann window, the two-tone signal, frames analysed from it on the
device, and raw random frames.  numpy only at import: analysed() and make_pvoc() import torch and the library when called,
so the tests that need no device (tests/pvoc_desc_cases.py, tests/test_pvoc_probe_cpu.py) take their inputs from here too.

Every recipe draws from its generator in a fixed order, and the tests' measured margins belong to exactly these values:
the order of the draws is part of each recipe."""
import numpy as np

SR = 48000.0
DEV = "cuda:0"
f32 = np.float32
_FRAMES = {}


def hann(size):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(size) / size)).astype(f32)   # periodic


def two_tones(size, hop, C, F, seed, seeded_tones=False):
    """(C, samples of F frames) float64: noise plus two sinusoids, at bins 10.37 (between bins) and size / 2 - 3.21 (near
    Nyquist), or with seeded_tones at two bins drawn before the noise.  `seed` may be a Generator, which then goes on
    from where the noise ends"""
    rng = np.random.default_rng(seed)
    n = size + (F - 1) * hop
    t = np.arange(n)
    k1, k2 = (rng.uniform(5, 20), rng.uniform(size / 4, size / 2 - 2)) if seeded_tones else (10.37, size / 2 - 3.21)
    return 0.1 * rng.standard_normal((C, n)) + 0.7 * np.cos(2 * np.pi * k1 / size * t + 0.2) \
        + 0.4 * np.cos(2 * np.pi * k2 / size * t)


def analyse_device(x, size, hop):
    """Stft.analyze_device and Pvoc.analyze_device of the signal x (C, n): the frames (C, F, size / 2 + 1, 2), numpy"""
    import torch
    import opencl_fft_amd as fa
    C = x.shape[0]
    st = fa.Stft(0, size, hop, window=hann(size))
    assert st.get_error() == 0, st.get_log()
    F = st.frames(x.shape[1])
    spec = torch.zeros((C, F, size // 2), dtype=torch.complex64, device=DEV)
    assert st.analyze_device(torch.from_numpy(x.astype(f32)).to(DEV), spec) == 0
    fr = torch.zeros((C, F, size // 2 + 1, 2), device=DEV)
    assert fa.Pvoc(0, size, hop, SR, C).analyze_device(spec, fr) == 0
    torch.cuda.synchronize()
    return fr.cpu().numpy()


def analysed(size, C, F, seed, seeded_tones=True):
    """frames of two_tones() at hop size / 4 through Stft + Pvoc.analyze_device (numpy, cached, read-only)"""
    key = ("a", size, C, F, seed, seeded_tones)
    if key not in _FRAMES:
        a = analyse_device(two_tones(size, size // 4, C, F, seed, seeded_tones), size, size // 4)
        assert a.shape[1] == F
        a.setflags(write=False)
        _FRAMES[key] = a
    return _FRAMES[key]


def _amps(rng, C, F, B, tilt, decades, zero):
    if tilt:
        ramp = np.linspace(-decades, decades, B) * rng.choice([-1.0, 1.0], (C, F, 1))
        amp = (10.0 ** (ramp + rng.uniform(-1, 1, (C, F, B)))).astype(f32)
        if zero:
            amp[C - 1, F - 1, B // 3] = 0
    else:
        amp = (10.0 ** rng.uniform(-30, 30, (C, F, B))).astype(f32)
        amp[rng.random((C, F, B)) < 0.02] = 0
    return amp


def _cached(key, frames):
    if key not in _FRAMES:
        a = np.stack(frames(), axis=-1)
        a.setflags(write=False)
        _FRAMES[key] = a
    return _FRAMES[key]


def raw(size, C, F, seed, tilt=False, decades=7.5, zero=True):
    """raw random frames, any freq: amps log-uniform over 1e-30 .. 1e30 and a few zeros.  tilt (the cases of the kernels
    with an envelope): a slope of 2 x `decades` over the bins, up or down by frame, times a random factor 0.1 .. 10, and
    with `zero` one zero amp.  15 decades keep the ratio of two envelopes inside float32 (the vocoder, the warp); the
    formant cases take all 60, since with independent bins amp / env * env would leave float32's range.  The amps are
    drawn before the freqs (numpy, cached, read-only)"""
    def frames():
        rng = np.random.default_rng(seed)
        B = size // 2 + 1
        amp = _amps(rng, C, F, B, tilt, decades, zero)
        return amp, rng.uniform(-SR, SR, (C, F, B)).astype(f32)
    return _cached(("r", size, C, F, seed, tilt, tilt and decades, tilt and zero), frames)


def raw_freq_first(size, C, F, seed, tilt=False):
    """the recipe of tests/test_gpu_pvoc_shape.py: the freqs are drawn before the amps, and the frames without tilt have
    some bins with a NaN amp and some with a NaN freq besides; tilt as in raw(), 15 decades and one zero amp, no NaN"""
    def frames():
        rng = np.random.default_rng(seed)
        B = size // 2 + 1
        freq = rng.uniform(-SR, SR, (C, F, B)).astype(f32)
        amp = _amps(rng, C, F, B, tilt, 7.5, True)
        if not tilt:
            amp[rng.random((C, F, B)) < 0.02] = np.nan
            freq[rng.random((C, F, B)) < 0.02] = np.nan
        return amp, freq
    return _cached(("rf", size, C, F, seed, tilt), frames)


def make_pvoc(size, hop, channels, sr=SR, env=None, monkeypatch=None):
    """a Pvoc object created under the switches `env` ({name: value}; a value of None leaves that switch alone), which
    the library reads at creation: they are gone again when this returns"""
    import opencl_fft_amd as fa
    env = {k: v for k, v in (env or {}).items() if v is not None}
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    pv = fa.Pvoc(0, size, hop, sr, channels)
    for k in env:
        monkeypatch.delenv(k)
    assert pv.get_error() == 0, pv.get_log()
    return pv
