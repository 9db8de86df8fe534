"""numpy restatement of the analysis of a stored signal at given time points (clfa_pvoc_tanal_dev, include/clfft_amd.h),
for the tests: the slices a frame reads, the float64 truth, the float32 yardstick, the starts the device test uses and
the impulse probe with its analytic spectra.  numpy only; tanal32 alone needs the C oracle.

The float64 analysis of a pair of spectra is pvoc_model.analyze64's formula on complex128 spectra: analyze64 itself rounds
its spectra to complex64 (they are its input), which a truth for the signal must not.

The impulse probe.  Integers from {+-1, +-2, +-3} sit size + hop + 1 samples apart, so at most one lies in any
[s - hop, s + size); the window holds the integers 1..31.  A windowed frame is then one integer impulse (exact in
float32), its packed spectrum is fft_exact.rfft_impulses' closed form, and every frame's truth is analytic.  A frame is of
one of four kinds: the impulse lies in NEITHER window, in A only (the earlier one), in B only, or in BOTH.
"""
import numpy as np

from tests import fft_exact
from tests import pvoc_model as pm
from tests import pvoc_probe as pp
from tests import stft_model

f32 = np.float32
EPS = pp.EPS
NEITHER, A_ONLY, B_ONLY, BOTH = 0, 1, 2, 3
# what tanal32 alone may reach on the impulse probe, per quantity: by the project's rule the next power of two above the
# worst value measured on the CPU (tests/test_pvoc_tanal_cpu.py records the values)
CAPS_TANAL = {"amp": 8.0, "dev": 1.0}
MARGIN = 4.0      # by the rule and the device run in the docstring of tests/test_gpu_pvoc_tanal.py


def slices(x, starts, size, hop):
    """(C, samples) -> (C, Fout, size + hop): x_c[s - hop .. s + size) per start s, +0 outside the rows, in x's dtype"""
    x = np.asarray(x)
    C, n = x.shape
    L = size + hop
    pad = np.zeros((C, n + 2 * L), x.dtype)
    pad[:, L:L + n] = x
    first = np.clip(np.asarray(starts, np.int64) - hop, -L, n) + L      # a window wholly outside reads zeros either way
    return pad[:, first[:, None] + np.arange(L)]


def windowed_pair(x, w, starts, size, hop):
    """(a, b), float32 (C, Fout, size) each: fl(w[t] x[s - hop + t]) and fl(w[t] x[s + t])"""
    sl = slices(np.asarray(x, f32), starts, size, hop)
    w = np.asarray(w, f32)
    a, b = w * sl[..., :size], w * sl[..., hop:hop + size]
    assert a.dtype == f32 and b.dtype == f32
    return a, b


def pack64(frames):
    """real (..., size) -> the packed spectrum of Clrfft (size, forward) in float64: P[0] = (X[0], X[M]) / size,
    P[k] = 2 X[k] / size, P[M/2] conjugated"""
    size = frames.shape[-1]
    M = size // 2
    X = np.fft.rfft(np.asarray(frames, np.float64), axis=-1)
    P = 2.0 * X[..., :M] / size
    P[..., 0] = (X[..., 0].real + 1j * X[..., M].real) / size
    P[..., M // 2] = np.conj(P[..., M // 2])
    return P


def pair64(PA, PB, size, hop, sr):
    """the Analysis formula with z_f = zB, z_{f-1} = zA on complex128 packed spectra (..., M) -> (amp, dev in turns, freq)"""
    zA, zB = pm.bins(np.asarray(PA, np.complex128)), pm.bins(np.asarray(PB, np.complex128))
    d = zB * np.conj(zA) * pm.etab(size, hop).astype(np.complex128)
    dev = np.where(d == 0, 0.0, np.arctan2(d.imag, d.real) / (2 * np.pi))
    k = np.arange(size // 2 + 1, dtype=np.float64)
    return np.abs(zB), dev, (k + dev * (size / hop)) * (sr / size)


def tanal64(x, w, starts, size, hop, sr):
    """the float64 truth: (amp, dev, freq), each (C, Fout, M + 1)"""
    a, b = windowed_pair(x, w, starts, size, hop)
    return pair64(pack64(a), pack64(b), size, hop, sr)


def tanal32(x, w, starts, size, hop, sr):
    """the float32 yardstick: the C oracle's packed transform of the two windowed slices, then pvoc_model.analyze32 on
    the pair -> frames (C, Fout, M + 1, 2) float32"""
    from oracle import oracle
    a, b = windowed_pair(x, w, starts, size, hop)
    C, Fout = a.shape[:2]
    P = oracle.rfft_forward(np.stack([a, b], axis=2).reshape(C * Fout, 2, size))
    fr = pm.analyze32(P, pm.initial_prev(C * Fout, size), size, hop, sr)
    return np.ascontiguousarray(fr[:, 1].reshape(C, Fout, size // 2 + 1, 2))


def centre(size, sr):
    """the bin centres fl(k) fl(sr / size), float32 (M + 1,)"""
    return np.arange(size // 2 + 1, dtype=f32) * f32(sr / size)


# ---- the shapes and starts of the device test --------------------------------------------------------------------------

def samples_of(size):
    return 3 * size + 5


def fout_for(size, C=3):
    """the smallest Fout >= the fixed starts that gives at least seven full groups of fpw frames plus a ragged one over the
    C Fout frames, with Fout no multiple of fpw (fpw = 1: every group is full, and the count alone decides)"""
    fpw = stft_model.fpw(size)
    F = len(fixed_starts(size, size // 4))
    while not (C * F >= 7 * fpw + 1 and (fpw == 1 or (F % fpw and (C * F) % fpw))):
        F += 1
    return F


def fixed_starts(size, hop):
    n = samples_of(size)
    run = [n // 2 + 9 - 3 * i for i in range(5)]                       # a descending run, both parities
    return [-size - hop - 5,                                            # both windows before the row
            -3, hop - 1,                                                # B, then only A, partly before it
            n - size, n - size + 1, n - 1, n + hop + 7,                 # past the end by degrees, up to wholly silent
            size // 3, size // 3, size // 3] + run                      # one start three times


def starts_for(size, hop, Fout, seed=0):
    """int32 (Fout,): the fixed entries, then draws from [-size, samples] of both parities"""
    fixed = fixed_starts(size, hop)
    assert Fout >= len(fixed)
    rng = np.random.default_rng([size, hop, seed])
    rest = rng.integers(-size, samples_of(size) + 1, Fout - len(fixed))
    if rest.size >= 2:
        rest[0] |= 1
        rest[1] &= ~1
    s = np.concatenate([np.array(fixed, np.int64), rest]).astype(np.int32)
    s.setflags(write=False)
    return s


# ---- the impulse probe ---------------------------------------------------------------------------------------------------

def int_window(size):
    """the integers 1..31, float32 (size,)"""
    return (1 + np.arange(size) % 31).astype(f32)


def impulse_row(size, hop, samples, seed):
    """(row float32 (samples,), positions, amplitudes): integers from {+-1, +-2, +-3}, size + hop + 1 apart; one of them
    sits size / 2 + 3 seed behind the first start of the descending run of fixed_starts, so that the run's frames hold
    it in both windows"""
    rng = np.random.default_rng([size, hop, seed, 77])
    gap = size + hop + 1
    pos = np.arange((samples // 2 + 9 + size // 2 + 3 * seed) % gap, samples, gap)
    amps = rng.choice([-3, -2, -1, 1, 2, 3], pos.size)
    row = np.zeros(samples, f32)
    row[pos] = amps
    return row, pos, amps


def impulse_truth(size, hop, sr, w, pos, amps, starts):
    """the analytic truth of one impulse row under the window w (integers): (amp64, dev64, freq64) (Fout, M + 1) and the
    frames' kinds (Fout,)"""
    starts = np.asarray(starts, np.int64)
    M = size // 2
    PA = np.zeros((starts.size, M), np.complex128)
    PB = np.zeros((starts.size, M), np.complex128)
    kind = np.zeros(starts.size, np.int64)
    for P, first, flag in ((PA, starts - hop, A_ONLY), (PB, starts, B_ONLY)):
        off = pos[None, :] - first[:, None]                        # (Fout, impulses): the impulse's place in the window
        hit = (off >= 0) & (off < size)
        assert hit.sum(axis=1).max(initial=0) <= 1
        g, i = np.nonzero(hit)
        if g.size:
            t = off[g, i]
            for a in np.unique(amps[i] * w[t].astype(np.int64)):
                sel = amps[i] * w[t].astype(np.int64) == a
                P[g[sel]] = fft_exact.rfft_impulses(size, t[sel], float(a))
        kind[g] |= flag
    return pair64(PA, PB, size, hop, sr) + (kind,)


def probe_errors(frames, amp64, dev64, kind, size, hop, sr):
    """the worst bin of the frames of kind BOTH, per quantity, in the yardstick's units, and where it sits (frame, bin):
    amp  |amp - amp64| / (2^-24 max_k amp64 of the frame);  dev  the distance on the circle of turns / s_k
    (pvoc_probe.dev_scale).  A NaN counts as an infinite error.  {"amp": (worst, at), "dev": (worst, at)}; 0 without frames"""
    both = np.nonzero(kind == BOTH)[0]
    if both.size == 0:
        return {"amp": (0.0, (0, 0)), "dev": (0.0, (0, 0))}
    fr = np.asarray(frames)[both]
    top = amp64[both].max(axis=-1, keepdims=True)
    ea = np.abs(fr[..., 0].astype(np.float64) - amp64[both]) / (EPS * top)
    d = pm.dev_of(fr[..., 1], size, hop, sr) - dev64[both]
    with np.errstate(all="ignore"):
        ed = np.abs((d + 0.5) - np.floor(d + 0.5) - 0.5) / pp.dev_scale(size, hop)
    out = {}
    for q, e in (("amp", ea), ("dev", ed)):
        e = np.where(np.isnan(e), np.inf, e)
        at = np.unravel_index(int(np.argmax(e)), e.shape)
        out[q] = (float(e[at]), (int(both[at[0]]), int(at[1])))
    return out
