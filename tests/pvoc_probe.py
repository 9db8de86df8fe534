"""Probe spectra and the per-bin yardstick for the core conversion of clfa_pvoc (pvoc_kernels.hip: k_pvoc_analyze,
k_pvoc_sums, k_pvoc_scan, k_pvoc_walk), numpy only: shared by tests/test_gpu_pvoc_bins.py (the device) and
tests/test_pvoc_probe_cpu.py (the float32 model and its mutants).

The ranged probe.  probe_spectra(size, hop, C, F): packed spectra (C, F, M) complex64, M = size / 2.  Bin k = 0..M of
channel c has |z| = 2^L(c, k) 2^u(c, f, k): L an integer uniform in [-40, 40] — every bin has its own level, over 80
octaves, so no bin hides behind a louder one — u uniform in [-4, 4] per frame, the phase uniform in (-pi, pi] (bins 0 and M
are real: a sign).  |z| stays inside 2^+-44, so every product |z| |z_prev| is a normal float32 (2^-88 .. 2^88): neither
overflow (outside the contract) nor underflow.  Three frames are designated:
  ZERO_F    all zero, the last frame of a run of the analysis: it and its successor (the first of the next run, whose lanes
            read it again) have d = (0, 0);
  DOUBLE_F  its predecessor times 2 (d on the positive real axis before the rotation by e[k]);
  NEG_F     its predecessor times -1, the first frame of a run: the cut of atan2 at +-1/2 turn where e[k] = 1.

The yardstick.  Functions of any frames or spectra (device, model or mutant), each returning the worst normalised error
and where it sits (channel, frame, bin):
  amp_worst    |amp - |z|_64| / (2^-24 |z|_64); where |z| is 0 the amp is 0 or the error is infinite;
  dev_worst    dev recovered from freq in float64 (pvoc_model.dev_of), the error the distance on the circle of turns,
               w = |frac(got - truth + 1/2) - 1/2| (+1/2 and -1/2 turn are one answer: the sign of a cancelled imaginary
               part is not defined, k_pvoc_analyze contracts where the model does not), normalised by
               s_k = 2^-24 (1.5 + k hop / size): a size-independent term for the atan2 chain plus the rounding of
               freq ~ (k + dev size / hop) sr / size to float32, which resolves dev to 2^-24 (k hop / size + 1/2) turns;
  synth_worst  |z_got - z_truth| / (2^-24 |amp|), z unpacked with pvoc_model.bins (real parts only at bins 0 and M: all
               the packed layout keeps), z_truth = pvoc_model.synth64 on the exact integer phases; amp == 0 gives exactly 0.
A NaN anywhere counts as an infinite error.

The bound of a case: worst <= MARGIN_BIN x max(U32, 1), U32 the float32 model's worst on the same inputs against the same
truth (bound()).  tests/test_pvoc_probe_cpu.py caps U32 (CAPS), so a probe that inflated the bound would fail there.

The exact probes give values, not tolerances:
  exact_synth(size, C, F)      sr = 65536, hop = size / 4: kf = hop / sr is a power of two; freq = q sr / (4 hop) with
                               integer |q| < 2^20, all four residues of q mod 4 in every bin; amps integers in [-3, 3].
                               Then t = q / 4 exactly, inc = (q mod 4) 2^30, every phase is a multiple of a quarter turn
                               and the spectrum is amp x {1, i, -1, -i} at every element;
  exact_analysis(size, C, F)   hop = size, so e[k] = (1, -0): Gaussian integers with integer moduli, frame f = frame f - 1
                               times 1, 2 or 3 (at most three 3s per bin: every product stays an exact float32), so
                               d = (positive, +0), dev = 0, freq = (float)k (float)(sr / size) and amp the integer modulus,
                               to the bit.
"""
import numpy as np

from tests import pvoc_model as pm

f32 = np.float32
EPS = 2.0 ** -24
SIZES = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)
SR = 48000.0
SR_EXACT = 65536.0
RUN = 4                                # kPvocRun: consecutive frames per lane of k_pvoc_analyze
ZERO_F, DOUBLE_F, NEG_F = 7, 13, 20    # 7 = 2 RUN - 1: the last of a run; 13: inside a run; 20 = 5 RUN: the first of a run
CUT = 5                                # the split of the second analysis: run 1 of the first call has one frame
CAPS = {"amp": 2.0, "dev": 4.0, "synth": 8.0}    # what the float32 model alone may reach on a probe
MARGIN_BIN = 2.0                       # by the rule and the device run in the docstring of tests/test_gpu_pvoc_bins.py


def hops(size):
    """size / 4, size (e[k] = 1), 3 (does not divide the size), size / 4 + 1 (odd: k hop mod size takes every residue)"""
    return (size // 4, size, 3, size // 4 + 1)


_PROBES = {}


def probe_spectra(size, hop, C=2, F=69):
    key = (size, hop, C, F)
    if key not in _PROBES:
        assert F > NEG_F + 1
        B = size // 2 + 1
        rng = np.random.default_rng([size, hop])
        L = rng.integers(-40, 41, (C, 1, B)).astype(np.float64)
        u = rng.uniform(-4.0, 4.0, (C, F, B))
        u[:, DOUBLE_F - 1] = np.minimum(u[:, DOUBLE_F - 1], 3.0)      # twice it stays inside the range
        ph = -rng.uniform(-np.pi, np.pi, (C, F, B))                   # (-pi, pi]
        z = np.exp2(L + u) * np.exp(1j * ph)
        z[..., 0] = np.exp2(L + u)[..., 0] * np.where(ph[..., 0] < 0, -1.0, 1.0)
        z[..., -1] = np.exp2(L + u)[..., -1] * np.where(ph[..., -1] < 0, -1.0, 1.0)
        z = z.astype(np.complex64)
        z[:, ZERO_F] = 0
        z[:, DOUBLE_F] = z[:, DOUBLE_F - 1] * f32(2)
        z[:, NEG_F] = -z[:, NEG_F - 1]
        P = np.ascontiguousarray(pm.unbins(z))
        assert P.dtype == np.complex64
        P.setflags(write=False)
        _PROBES[key] = P
    return _PROBES[key]


def _worst(e):
    e = np.where(np.isnan(e), np.inf, e)
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(e)), e.shape))
    return float(e[at]), at


def amp_worst(frames, amp64):
    got = np.asarray(frames)[..., 0].astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - amp64) / (EPS * amp64)
    return _worst(np.where(amp64 == 0, np.where(got == 0, 0.0, np.inf), e))


def dev_scale(size, hop):
    """s_k, k = 0..M, in turns"""
    return EPS * (1.5 + np.arange(size // 2 + 1, dtype=np.float64) * hop / size)


def dev_worst(frames, dev64, size, hop, sr):
    d = pm.dev_of(np.asarray(frames)[..., 1], size, hop, sr) - dev64
    with np.errstate(all="ignore"):
        w = np.abs((d + 0.5) - np.floor(d + 0.5) - 0.5)
    return _worst(w / dev_scale(size, hop))


def synth_worst(spec, frames, theta):
    amp = np.abs(np.asarray(frames)[..., 0].astype(np.float64))
    zt = pm.bins(pm.synth64(frames, theta))
    zg = pm.bins(np.asarray(spec)).astype(np.complex128)
    with np.errstate(all="ignore"):
        e = np.abs(zg - zt) / (EPS * amp)
    return _worst(np.where(amp == 0, np.where(zg == 0, 0.0, np.inf), e))


def bound(margin, u32):
    return margin * max(u32, 1.0)


def analysis_errors(frames, amp64, dev64, size, hop, sr):
    """{"amp": (worst, at), "dev": (worst, at)}"""
    return {"amp": amp_worst(frames, amp64), "dev": dev_worst(frames, dev64, size, hop, sr)}


# ---- the exact probes ----

_UNITS = np.array([1, 1j, -1, -1j], np.complex64)


def exact_synth(size, C=2, F=131):
    """(frames (C, F, M + 1, 2) float32, the expected spectra (C, F, M) complex64, the expected phase state uint32, hop);
    from the zero state, for sr = SR_EXACT"""
    M = size // 2
    hop = size // 4
    rng = np.random.default_rng([size, 4])
    res = rng.integers(0, 4, (C, F, M + 1))
    c, f, k = np.ogrid[:C, :4, :M + 1]
    res[:, :4] = (c + f + k) % 4                                   # all four residues in every bin
    q = 4 * rng.integers(-2 ** 18 + 1, 2 ** 18 - 1, (C, F, M + 1)) + res
    assert np.abs(q).max() < 2 ** 20
    amp = rng.integers(-3, 4, (C, F, M + 1))
    frames = np.stack([amp.astype(f32), (q * (SR_EXACT / size)).astype(f32)], axis=-1)
    assert np.array_equal(frames[..., 1].astype(np.float64) * size / SR_EXACT, q)
    quarters = np.cumsum(q % 4, axis=1) % 4                        # the phase in quarter turns
    z = (amp.astype(f32) * _UNITS[quarters]).astype(np.complex64)
    want = np.ascontiguousarray(pm.unbins(z))
    state = (quarters[:, -1].astype(np.uint64) << np.uint64(30)).astype(np.uint32)
    for a in (frames, want, state):
        a.setflags(write=False)
    return frames, want, state, hop


_BASES = [(x * sx, y * sy) for a, b in ((3, 4), (5, 12), (8, 15)) for x, y in ((a, b), (b, a)) for sx in (1, -1) for sy in (1, -1)]
_AXIS = [(5, 0), (-13, 0), (0, 17), (0, -5)]
_MODULUS = {b: int(round(np.hypot(*b))) for b in _BASES + _AXIS}


def exact_analysis(size, C=2, F=13):
    """(spectra (C, F, M) complex64, the expected amps (C, F, M + 1) float32, the expected freq row (M + 1,) float32); hop =
    size, sr = SR"""
    M = size // 2
    rng = np.random.default_rng([size, 1])
    both = _BASES + _AXIS
    pick = rng.integers(0, len(both), (C, M))
    pick[:, 0] = rng.integers(0, len(_BASES), C)                   # bins 0 and M: Re and Im of P[0], both non-zero
    base = np.array(both, np.float64)[pick]                        # (C, M, 2)
    m = rng.integers(1, 4, (C, F, M))
    m[:, 0] = 1
    m = np.where((m == 3) & (np.cumsum(m == 3, axis=1) > 3), 2, m)
    scale = np.cumprod(m.astype(np.float64), axis=1)               # exact: < 2^F 27
    re, im = base[:, None, :, 0] * scale, base[:, None, :, 1] * scale               # (C, F, M), integers
    P = (re + 1j * im).astype(np.complex64)
    assert np.array_equal(P.real, re) and np.array_equal(P.imag, im)
    mod = np.array([_MODULUS[b] for b in both], np.float64)[pick][:, None] * scale
    assert np.array_equal(mod * mod, re * re + im * im)
    want = np.concatenate([np.abs(re[..., :1]), mod[..., 1:], np.abs(im[..., :1])], axis=-1).astype(f32)
    assert np.array_equal(want.astype(np.float64)[..., 1:M], mod[..., 1:])
    freq = np.arange(M + 1, dtype=f32) * f32(SR / size)
    for a in (P, want, freq):
        a.setflags(write=False)
    return P, want, freq
