"""Restatement of the oscillator bank's definition (clfa_pvoc_adsyn, include/clfft_amd.h), for the tests, in three forms:
Python integers for the endpoint words, slopes, phases and the state (the scalar functions below, and their numpy uint64
twins, which wrap mod 2^64 as the definition does); float64 for the samples, as the truth; and float32 step by step, every
operation rounded on its own, as the yardstick the GPU's samples are measured beside (tests/test_gpu_pvoc_adsyn.py)."""
import numpy as np

f32 = np.float32
MASK64 = (1 << 64) - 1


# ---- Python integers: one bin, one frame ------------------------------------------------------------------------------

def word(t):
    """the endpoint word of t (a float32 number of turns per sample): (W, good)"""
    t = float(f32(t))
    if not abs(t) < 0.5:          # NaN, infinities, at or above Nyquist
        return 0, False
    return int(np.rint(t * 4294967296.0)), True


def start(a0, w0, wf):
    return wf if a0 == 0 else w0


def slope(w0, wf, hop):
    """D mod 2^64: Python's // floors towards minus infinity"""
    return ((((wf - w0) << 30) // hop) * 4) & MASK64


def phase(p, w0, d, j):
    return (p + j * (w0 << 32) + (j * (j + 1) // 2) * d) & MASK64


def advance(w0, d, hop):
    return phase(0, w0, d, hop)


# ---- numpy: whole calls ----------------------------------------------------------------------------------------------

def initial_state(channels, size):
    B = size // 2 + 1
    return np.zeros((channels, B), np.uint64), np.zeros((channels, B), np.int32), np.zeros((channels, B), f32)


def selection(M, first_bin=0, nbins=None, step=1):
    if nbins is None:
        nbins = (M - first_bin) // step + 1
    bins = first_bin + step * np.arange(nbins)
    assert step >= 1 and nbins >= 1 and first_bin >= 0 and bins[-1] <= M
    return bins


def endpoints(frames, fmod, sr):
    """(W int32, A float32) of every bin of frames (..., F, B, 2); fmod (F,) or None"""
    fr = np.asarray(frames, f32)
    ks = f32(1.0 / sr)
    with np.errstate(invalid="ignore", over="ignore"):
        t = fr[..., 1]
        if fmod is not None:
            t = t * np.asarray(fmod, f32)[:, None]
        t = t * ks
        assert t.dtype == f32
        good = np.abs(t) < f32(0.5)
    W = np.rint(np.where(good, t, f32(0)).astype(np.float64) * 4294967296.0).astype(np.int64).astype(np.int32)
    A = np.where(good, fr[..., 0], f32(0)).astype(f32)
    return W, A


def segments(frames, state, hop, sr, fmod=None, bins=None):
    """the per-frame segment values of the selected bins, (channels, F, nb) each, and the new state"""
    fr = np.asarray(frames, f32)
    C, F, B, _ = fr.shape
    bins = np.arange(B) if bins is None else np.asarray(bins)
    P, Ws, As = (np.array(s, copy=True) for s in state)
    if F == 0:
        return None, (P, Ws, As)
    W, A = endpoints(fr[:, :, bins], fmod, sr)
    W0 = np.concatenate([Ws[:, bins][:, None], W[:, :-1]], axis=1).astype(np.int64)
    A0 = np.concatenate([As[:, bins][:, None], A[:, :-1]], axis=1)
    W1 = W.astype(np.int64)
    W0 = np.where(A0 == 0, W1, W0)
    D = (((W1 - W0) << 30) // hop).astype(np.uint64) << np.uint64(2)
    h = np.uint64(hop)
    with np.errstate(over="ignore"):
        adv = (h * (W0.astype(np.uint64) << np.uint64(32))) + np.uint64(hop * (hop + 1) // 2) * D
        ends = P[:, bins][:, None] + np.cumsum(adv, axis=1, dtype=np.uint64)
    base = np.concatenate([P[:, bins][:, None], ends[:, :-1]], axis=1)
    P[:, bins] = ends[:, -1]
    Ws[:, bins] = W[:, -1]
    As[:, bins] = A[:, -1]
    return dict(A0=A0, A1=A, W0=W0, D=D, base=base, hop=hop), (P, Ws, As)


def _frame_phase(seg, f):
    """phase(j) of frame f as uint64 (channels, hop, nb)"""
    hop = seg["hop"]
    j = np.arange(1, hop + 1, dtype=np.uint64)[None, :, None]
    tri = (j * (j + np.uint64(1))) >> np.uint64(1)
    with np.errstate(over="ignore"):
        return seg["base"][:, f, None, :] + j * (seg["W0"][:, f, None, :].astype(np.uint64) << np.uint64(32)) \
            + tri * seg["D"][:, f, None, :]


def samples64(seg, gain=1.0):
    """the truth: exact phases, everything else in float64 -> (channels, F * hop)"""
    hop = seg["hop"]
    C, F, nb = seg["A0"].shape
    y = np.zeros((C, F, hop))
    w = (np.arange(1, hop + 1) / hop)[None, :, None]
    for f in range(F):
        a0, a1 = seg["A0"][:, f, None, :].astype(np.float64), seg["A1"][:, f, None, :].astype(np.float64)
        ph = _frame_phase(seg, f).astype(np.float64) * (2.0 * np.pi / 18446744073709551616.0)
        with np.errstate(invalid="ignore"):
            y[:, f] = ((a0 + (a1 - a0) * w) * np.cos(ph)).sum(axis=-1)
    return (float(f32(gain)) * y).reshape(C, F * hop)


def samples32(seg, gain=1.0):
    """the yardstick: the definition's float32 steps, each rounded on its own, the sum sequential in ascending bins;
    numpy's float32 cos of pi times the phase's top 32 bits in half turns"""
    hop = seg["hop"]
    C, F, nb = seg["A0"].shape
    y = np.zeros((C, F, hop), f32)
    w = (np.arange(1, hop + 1, dtype=np.float64) / hop).astype(f32)[None, :, None]
    for f in range(F):
        a0, a1 = seg["A0"][:, f, None, :], seg["A1"][:, f, None, :]
        hi = (_frame_phase(seg, f) >> np.uint64(32)).astype(np.uint32).view(np.int32)
        with np.errstate(invalid="ignore"):
            cs = np.cos(f32(np.pi) * (hi.astype(f32) * f32(2.0 ** -31)))
            term = (a0 + (a1 - a0) * w) * cs
            assert term.dtype == f32
            y[:, f] = f32(gain) * np.add.accumulate(term, axis=-1, dtype=f32)[..., -1]
    return y.reshape(C, F * hop)


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a - ref))
