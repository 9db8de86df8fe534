"""Every route of the overlap-add synthesis (k_stft_synth, stft_kernels.hip), checked per sample against an exact model.

The probe.  Every frame's spectrum is zero except its packed bin 0 = (a, b), small integers drawn per (channel, frame).
The c2r pair map turns that into Z[0] = (a + b, a - b), and the inverse transform of an impulse at index 0 multiplies by
twiddle 1 only: r_f[t] = a + b on even t, a - b on odd t, exactly.  The window holds small integers, so every product
and every partial sum of the overlap-add is an exact float32, and the device output with normalize=False must equal the
float64 model (tests/stft_model.overlap_add on np.fft.irfft of the one-sided bins) BIT FOR BIT.  With normalize=True the
only roundings left are the envelope's one and the division's one: |y_dev env64 / y_exact - 1| <= 2^-23 (1 + 1e-6) per
sample, and exactly 0 where y_exact is 0.  The short calls take a wider integer window (wide_top), whose sums of squares
pass 2^24: there the envelope's rounding is a real one, and a table of float32 running sums misses the bound.  A missing, doubled, misplaced or foreign frame changes an integer; a failure
prints the first wrong (channel, sample), its covering frames and the run, group and fw it belongs to, from the mirror of
stft_plan.hpp in tests/stft_model.py.

Isolation.  Three channels, the middle one's spectra all NaN: channels 0 and 2 must be exact and finite, so no clamped
load and no warm-up frame crosses a channel boundary.  Rows have a stride pad and the buffer has guard bands before and
after, all prefilled with a canary that must survive.

Every case asserts from the mirror that it still splits as intended (runs, ragged groups, envelope form 3), so a change
of the launcher cannot quietly turn it into another case."""
import time

import numpy as np
import pytest
import torch

import opencl_fft_amd as fa
from oracle import oracle
from tests import gpu_guard
from tests import stft_model as sm
from tests.gpu_guard import DEV
from tests.test_gpu_stft import analyze_dev, check_analysis

gpu = pytest.mark.gpu
GUARD, PAD = 1024, 5    # floats before and after the buffer; floats between a row's end and the next row
NORM_TOL = 2.0 ** -23 * (1 + 1e-6)   # one rounding of the envelope + one division
SIZES = sorted({s for s, _ in sm.SYNTH_PAIRS})


def int_window(size, top=31):
    """integers 1..top, scattered"""
    d = np.arange(size, dtype=np.int64)
    return (1 + ((d * 40503) >> 4) % top).astype(np.float32)


def wide_top(size, hop, F):
    """the largest window value (at most 1023) that keeps sum |w r| of the frames over one sample below 2^24, |r| <= 6.
    With it the envelope's sums of w^2 pass 2^24, so a table kept in float32 rounds them and the lookup's one float32
    rounding is a real one; the window of the other cases (1..31) keeps every sum of squares exact in float32 as well"""
    return min(1023, (2 ** 24 - 1) // (6 * min(F, -(-size // hop))))


def probe_spectra(C, F, size, seed):
    """(C, F, size/2) complex64, zero but bin 0 = (a, b), integers in -3..3 per (channel, frame)"""
    rng = np.random.default_rng(seed)
    spec = np.zeros((C, F, size // 2), np.complex64)
    spec[:, :, 0] = rng.integers(-3, 4, (C, F)) + 1j * rng.integers(-3, 4, (C, F))
    return spec


def exact_model(spec, size, hop, w):
    """float64 y (unnormalized) and envelope of the probe; asserts the exactness the bit comparison rests on"""
    r64 = np.fft.irfft(fa.packed_to_onesided(spec.astype(np.complex128)), n=size, axis=-1)
    r = np.rint(r64)
    assert np.abs(r64 - r).max() < 1e-9, "the probe's frames are integers (up to irfft's own float64 rounding)"
    a, b = spec[:, :, 0].real.astype(np.float64), spec[:, :, 0].imag.astype(np.float64)
    assert np.array_equal(r[:, :, 0], a + b) and np.array_equal(r[:, :, 1], a - b)
    y, env = sm.overlap_add(r, w.astype(np.float64), hop)
    return r, y, env


def assert_integer_budget(r, y, w, hop):
    """rounding the model to float32 loses nothing, and no partial sum of the overlap-add can round: sum |terms| < 2^24"""
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    mag = sm.overlap_add(np.abs(r), np.abs(w).astype(np.float64), hop)[0]
    assert mag.max() < 2.0 ** 24, mag.max()


def synth_guarded(size, hop, spec, w, normalize, grid_max=None, monkeypatch=None):
    """device synthesis into padded rows inside guard bands; returns the (C, L) rows after checking every canary"""
    if grid_max is not None:
        monkeypatch.setenv("CLFA_STFT_GRID_MAX", str(grid_max))
    st = fa.Stft(0, size, hop, window=w, fwd=False)
    if grid_max is not None:
        monkeypatch.delenv("CLFA_STFT_GRID_MAX")
    assert st.get_error() == 0, st.get_log()
    assert st.workspace_bytes() == 0
    C, F, _ = spec.shape
    L = st.samples(F)
    assert L == (F - 1) * hop + size
    g = gpu_guard.rows(C, L, L + PAD, before=GUARD, after=GUARD)
    assert st.synthesize_device(gpu_guard.dev(spec), g.data, normalize=normalize) == 0
    torch.cuda.synchronize()
    g.check_sides("the buffer")
    return g.host()


def split_of(size, hop, C, F):
    """nf and the runs of the call, from the mirror; the shape keeps nf independent of the kernel's occupancy"""
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    floor_nf = max(8 * -(-size // hop), sm.fpw(size))
    assert C * F <= num_cus * floor_nf, "nf would depend on occupancy"
    nf = sm.run_frames(C * F, num_cus, size, hop, F)
    assert nf == min(F, floor_nf)
    return nf, [sm.run(r, nf, F, size, hop) for r in range(sm.runs_of(F, nf))]


def explain(c, p, size, hop, F, nf, want, got):
    r, fw, group, (f_lo, f_hi) = sm.locate(p, nf, F, size, hop)
    return ("channel %d sample %d: expected %r, received %r; covering frames %d..%d; run %d (nf %d, fw %d), group %d of "
            "%d frames; envelope form %d" % (c, p, want, got, f_lo, f_hi, r, nf, fw, group, sm.fpw(size),
                                             int(sm.env_branch(size, hop, F, p))))


def check_exact(y_dev, y, real, size, hop, F, nf):
    """normalize=False: bit for bit on the real channels"""
    want = y.astype(np.float32)
    for i, c in enumerate(real):
        bad = np.flatnonzero(y_dev[c].view(np.uint32) != want[i].view(np.uint32))
        assert bad.size == 0, "%d samples differ; first: %s" % (
            bad.size, explain(c, int(bad[0]), size, hop, F, nf, want[i, bad[0]], y_dev[c, bad[0]]))


def check_normalized(y_dev, y, env, real, size, hop, F, nf, what):
    """normalize=True: |y_dev env64 / y_exact - 1| <= 2^-23 (1 + 1e-6); exactly 0 where y_exact is 0; where the envelope
    is not above 1e-11 the sample is not divided"""
    worst = 0.0
    div = np.where(env > 1e-11, env, 1.0)
    for i, c in enumerate(real):
        g = y_dev[c].astype(np.float64)
        zero = y[i] == 0
        err = np.zeros_like(g)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            err[~zero] = np.abs(g[~zero] * div[~zero] / y[i][~zero] - 1)
        err[~np.isfinite(g)] = np.inf
        err[zero & (g != 0)] = np.inf
        bad = np.flatnonzero(~(err <= NORM_TOL))
        assert bad.size == 0, "%d samples outside 2^-23; first (error %.3g): %s" % (
            bad.size, err[bad[0]], explain(c, int(bad[0]), size, hop, F, nf, y[i, bad[0]] / div[bad[0]], y_dev[c, bad[0]]))
        worst = max(worst, float(err.max()))
    print("STFTSYNTH %s: largest |y_dev env64 / y_exact - 1| = %.3g (bound %.3g)" % (what, worst, NORM_TOL))
    return worst


_CASES = {}


def case(size, hop, F, channels=3, top=31):
    """spectra with a NaN channel in the middle (after the data channel when there are two), the window and the model of
    the real channels: made once per shape and shared, never written to"""
    key = (size, hop, F, channels, top)
    if key not in _CASES:
        spec = probe_spectra(channels, F, size, seed=size * 131 + hop * 7 + F)
        spec[1] = np.nan + 1j * np.nan
        real = [c for c in range(channels) if c != 1]
        w = int_window(size, top)
        r, y, env = exact_model(spec[real], size, hop, w)
        assert_integer_budget(r, y, w, hop)
        for a in (spec, w, y, env):
            a.setflags(write=False)
        _CASES[key] = (spec, w, real, y, env)
    return _CASES[key]


def run_case(size, hop, F, normalize, channels=3, grid_max=None, monkeypatch=None, top=31):
    spec, w, real, y, env = case(size, hop, F, channels, top)
    nf, runs = split_of(size, hop, channels, F)
    t0 = time.perf_counter()
    y_dev = synth_guarded(size, hop, spec, w, normalize, grid_max, monkeypatch)
    dt = time.perf_counter() - t0
    assert np.all(np.isfinite(y_dev[real])), "a real channel took something from the NaN channel"
    if normalize:
        check_normalized(y_dev, y, env, real, size, hop, F, nf, "size %d hop %d F %d" % (size, hop, F))
    else:
        check_exact(y_dev, y, real, size, hop, F, nf)
    print("STFTSYNTH size %d hop %d F %d norm %d: device call %.3f s" % (size, hop, F, normalize, dt))
    return y_dev, nf, runs


# ---- the probe itself, on the CPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_oracle_inverse_returns_the_probe_frames_exactly(size):
    """the C restatement of Clrfft's inverse gives a + b on even t and a - b on odd t, bit for bit"""
    ab = np.array([(a, b) for a in range(-3, 4) for b in range(-3, 4)], np.float32)
    spec = np.zeros((len(ab), size // 2), np.complex64)
    spec[:, 0] = ab[:, 0] + 1j * ab[:, 1]
    r = oracle.rfft_inverse(spec)
    want = np.empty((len(ab), size), np.float32)
    want[:, 0::2] = (ab[:, 0] + ab[:, 1])[:, None]
    want[:, 1::2] = (ab[:, 0] - ab[:, 1])[:, None]
    assert np.array_equal(r, want)
    _, y, _ = exact_model(spec[None], size, size, int_window(size))
    assert np.array_equal(y[0].reshape(len(ab), size), want.astype(np.float64) * int_window(size))


def test_mirror_locates_a_sample():
    # size 64, hop 16, nf 128: sample 4096 is the first of run 2, whose warm-up starts at frame 253
    assert sm.locate(4096, 128, 300, 64, 16) == (2, 253, 0, (253, 256))
    assert sm.locate(4095, 128, 300, 64, 16) == (1, 125, 1, (252, 255))
    assert list(sm.env_branch(64, 1, 5, [0, 4, 5, 62, 63, 67])) == [2, 2, 3, 3, 1, 1]


# ---- three runs, the last one short, a ragged last group, at every frames-per-workgroup class --------------------------
# (8192, 8191): 8 ceil(size / hop) = 16 frames per run, so three runs need F > 32
THREE_RUNS = [(64, 16, 300), (64, 1, 1100), (256, 3, 1500), (1024, 255, 100), (2048, 64, 600), (4096, 1024, 75),
              (8192, 8191, 36), (16384, 4096, 70)]


def assert_three_ragged_runs(size, hop, F, nf, runs):
    assert len(runs) == 3 and runs[2][1] - runs[2][0] < nf, (nf, runs)
    assert all(fw > 0 and fw <= s for s, _, _, fw in runs[1:]), "the later runs re-transform warm-up frames"
    if sm.fpw(size) > 1:
        assert any((e_end - fw) % sm.fpw(size) for _, e_end, _, fw in runs), "no run ends in a ragged group"


@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size,hop,F", THREE_RUNS)
def test_three_runs_exact_per_sample(size, hop, F, normalize):
    _, nf, runs = run_case(size, hop, F, normalize)
    assert_three_ragged_runs(size, hop, F, nf, runs)


@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size,hop,F", [(64, 64, 300), (4096, 4096, 20)])
def test_no_overlap_exact_per_sample(size, hop, F, normalize):
    _, nf, runs = run_case(size, hop, F, normalize)
    assert len(runs) > 1 and all(fw == s for s, _, _, fw in runs), "hop = size: no warm-up frame"


# ---- short calls: the envelope's third form, F = 1, F = 2, F < FPW -----------------------------------------------------
SHORT_PAIRS = [(64, 1), (64, 3), (256, 3), (2048, 16), (2048, 1)]
SHORT = [(size, hop, F) for size, hop in SHORT_PAIRS
         for F in [1, 2, 5] + [-(-size // hop) + k for k in (-1, 0, 1)]]


@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size,hop,F", SHORT)
def test_short_calls_exact_per_sample(size, hop, F, normalize):
    channels = 2 if (size, hop) == (2048, 1) and F > 5 else 3    # (data, NaN) keeps the largest cases small
    _, nf, runs = run_case(size, hop, F, normalize, channels=channels, top=wide_top(size, hop, F))
    assert len(runs) == 1 and nf == F
    forms = sm.env_branch(size, hop, F, np.arange((F - 1) * hop + size))
    if F in (1, 2, 5):
        assert np.any(forms == 3), "far fewer frames than size / hop: samples cut off on both sides, the difference form"
        assert F < sm.fpw(size) or size == 2048, "one ragged group of clamped loads"
    else:   # ceil(size / hop) - 1 frames and more: every sample is cut off on one side at the most
        assert not np.any(forms == 3)


# ---- the 1e-11 threshold, crossed in both directions ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_envelope_threshold_divides_1e_10_and_keeps_1e_12(normalize):
    """hop = size: env = w^2.  w = 1e-6 (env 1e-12) is kept, w = 1e-5 (env 1e-10) is divided; both far from 1e-11 itself,
    where float32 and float64 may disagree.  The tiny window values round once in fl(w r), so both modes are compared at
    the normalize tolerance"""
    size = hop = 256
    C, F = 3, 70
    w = int_window(size)
    keep, divide = [0, 7, 128, 255], [1, 64, 129, 254]
    w[keep] = np.float32(1e-6)
    w[divide] = np.float32(1e-5)
    spec = probe_spectra(C, F, size, seed=11)
    spec[1] = np.nan + 1j * np.nan
    real = [0, 2]
    _, y, env = exact_model(spec[real], size, hop, w)
    e1 = env.reshape(F, size)
    assert np.all(e1[:, keep] < 2e-12) and np.all((e1[:, divide] > 5e-11) & (e1[:, divide] < 2e-10)) and np.all(np.delete(e1, keep + divide, axis=1) >= 1)
    nf, runs = split_of(size, hop, C, F)
    assert len(runs) > 1
    y_dev = synth_guarded(size, hop, spec, w, normalize)
    assert np.all(np.isfinite(y_dev[real]))
    check_normalized(y_dev, y, env if normalize else np.zeros_like(env), real, size, hop, F, nf,
                     "threshold, norm %d" % normalize)


# ---- the grid-stride loops, with the launch capped at two workgroups --------------------------------------------------
@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size,hop,F", [(64, 16, 300), (2048, 64, 600)])
def test_synthesis_capped_grid_is_bit_identical(size, hop, F, normalize, monkeypatch):
    """9 work items on 2 workgroups: five and four strides, the ring re-zeroed between items"""
    free, nf, runs = run_case(size, hop, F, normalize)
    assert 3 * len(runs) == 9
    capped, nf2, runs2 = run_case(size, hop, F, normalize, grid_max=2, monkeypatch=monkeypatch)
    assert (nf2, runs2) == (nf, runs), "the cap must not enter the run split"
    real = [0, 2]
    assert np.array_equal(capped[real].view(np.uint32), free[real].view(np.uint32))


@gpu
def test_analysis_capped_grid_is_bit_identical(monkeypatch):
    """(256, 64), 3 x 37 frames = 3 groups of 32 and a ragged one of 15, on 2 workgroups"""
    size, hop, C, F = 256, 64, 3, 37
    assert (C * F) % sm.fpw(size) and -(-(C * F) // sm.fpw(size)) == 4
    samples = size + (F - 1) * hop + hop // 2 + 1
    rng = np.random.default_rng(256064)
    x = (rng.random((C, samples), dtype=np.float32) * 2 - 1)
    w = (rng.random(size, dtype=np.float32) + 0.25).astype(np.float32)
    x_t = torch.from_numpy(x).to(DEV)
    free, _ = analyze_dev(size, hop, x_t, w)
    monkeypatch.setenv("CLFA_STFT_GRID_MAX", "2")
    capped, _ = analyze_dev(size, hop, x_t, w)
    monkeypatch.delenv("CLFA_STFT_GRID_MAX")
    assert free.shape == (C, F, size // 2)
    assert np.array_equal(capped.view(np.uint32), free.view(np.uint32))
    check_analysis(x, size, hop, w, capped)
