"""numpy restatement of the phase vocoder's definitions (clfa_pvoc, include/clfft_amd.h), for the tests: float64 for the
analysis, exact integer arithmetic for the phase increments and phases, and a float32 evaluation of the same formulas —
the yardstick the GPU results are measured beside (tests/test_gpu_pvoc.py)."""
import numpy as np

TWO32 = 4294967296.0


def bins(P):
    """packed spectra (..., M) -> z (..., M + 1): z[0] = (Re P[0], 0), z[M] = (Im P[0], 0), z[M/2] = conj(P[M/2])"""
    P = np.asarray(P)
    M = P.shape[-1]
    z = np.concatenate([P, P[..., :1].imag.astype(P.dtype)], axis=-1)
    z[..., 0] = P[..., 0].real
    z[..., M // 2] = np.conj(P[..., M // 2])
    return z


def unbins(z):
    """the synthesis' inverse of bins(): Re P[0] = Re z[0], Im P[0] = Re z[M], bin M/2 conjugated back"""
    z = np.asarray(z)
    M = z.shape[-1] - 1
    P = z[..., :M].copy()
    P[..., 0] = z[..., 0].real + 1j * z[..., M].real
    P[..., M // 2] = np.conj(z[..., M // 2])
    return P


def etab(size, hop):
    """e[k] = exp(-2 pi i ((k hop) mod size) / size), k = 0..M: computed in double, stored as float32 pairs"""
    k = np.arange(size // 2 + 1, dtype=np.int64)
    a = -2.0 * np.pi * ((k * hop) % size).astype(np.float64) / size
    return (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32)).astype(np.complex64)


def initial_prev(channels, size):
    return np.ones((channels, size // 2 + 1), np.complex64)


def initial_phase(channels, size):
    return np.zeros((channels, size // 2 + 1), np.uint32)


def _with_prev(z, prev):
    return np.concatenate([np.asarray(prev, z.dtype)[:, None, :], z[:, :-1]], axis=1)


def analyze64(P, prev, size, hop, sr):
    """P (channels, F, M) complex64, prev (channels, M + 1) -> (amp, dev in turns, freq in Hz) in float64, and the new
    prev (complex64: z of the last frame, bit for bit)"""
    z32 = bins(np.asarray(P, np.complex64))
    z = z32.astype(np.complex128)
    d = z * np.conj(_with_prev(z, prev)) * etab(size, hop).astype(np.complex128)
    dev = np.where(d == 0, 0.0, np.arctan2(d.imag, d.real) / (2 * np.pi))
    k = np.arange(size // 2 + 1, dtype=np.float64)
    freq = (k + dev * (size / hop)) * (sr / size)
    return np.abs(z), dev, freq, (z32[:, -1].copy() if z32.shape[1] else np.asarray(prev, np.complex64))


def analyze32(P, prev, size, hop, sr):
    """the same formulas with every operation in float32 -> frames (channels, F, M + 1, 2) float32"""
    f32 = np.float32
    z = bins(np.asarray(P, np.complex64))
    zp = _with_prev(z, prev)
    e = etab(size, hop)
    zx, zy, px, py, ex, ey = z.real, z.imag, zp.real, zp.imag, e.real, e.imag
    amp = np.sqrt(zx * zx + zy * zy)
    tx, ty = zx * px + zy * py, zy * px - zx * py
    dx, dy = tx * ex - ty * ey, tx * ey + ty * ex
    with np.errstate(invalid="ignore"):
        dev = np.where((dx == 0) & (dy == 0), f32(0), np.arctan2(dy, dx) * f32(1.0 / (2 * np.pi))).astype(f32)
    k = np.arange(size // 2 + 1, dtype=f32)
    freq = (k + dev * f32(size / hop)) * f32(sr / size)
    assert amp.dtype == f32 and freq.dtype == f32
    return np.stack([amp, freq], axis=-1)


def dev_of(freq, size, hop, sr):
    """dev in turns recovered from freq (float64)"""
    k = np.arange(size // 2 + 1, dtype=np.float64)
    return (np.asarray(freq, np.float64) * (size / sr) - k) * (hop / size)


def increments(freq, hop, sr):
    """the phase increments as uint32 (exact): t = freq * kf and r = t - rint(t) in float32, each rounded on its own;
    inc = rint(r * 2^32) mod 2^32; 0 where freq or t is not finite"""
    kf = np.float32(hop / sr)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(freq, np.float32) * kf
        r = t - np.rint(t)
        ok = np.abs(r) <= np.float32(0.5)
    q = np.rint(np.where(ok, r, np.float32(0)).astype(np.float64) * TWO32).astype(np.int64)
    return (q & 0xFFFFFFFF).astype(np.uint32)


def phases(freq, theta0, hop, sr):
    """serial sum over the frame axis: theta (channels, F, M + 1) uint32 and the new state"""
    acc = np.cumsum(increments(freq, hop, sr).astype(np.uint64), axis=1) + np.asarray(theta0, np.uint64)[:, None, :]
    theta = (acc & 0xFFFFFFFF).astype(np.uint32)
    return theta, (theta[:, -1].copy() if theta.shape[1] else np.asarray(theta0, np.uint32).copy())


def phases_chunked(freq, theta0, hop, sr, chunk):
    """the device's scan: per-chunk sums, the chunks' bases (the state plus the earlier chunks' sums), a walk from each
    base — all mod 2^32"""
    inc = increments(freq, hop, sr)
    C, F, B = inc.shape
    theta = np.zeros((C, F, B), np.uint32)
    base = np.asarray(theta0, np.uint32).copy()
    with np.errstate(over="ignore"):
        sums = [inc[:, a:a + chunk].sum(axis=1, dtype=np.uint32) for a in range(0, F, chunk)]
        for j, a in enumerate(range(0, F, chunk)):
            run = base.copy()
            for f in range(a, min(a + chunk, F)):
                run = run + inc[:, f]
                theta[:, f] = run
            base = base + sums[j]
    return theta, base


def synth64(frames, theta):
    """spectra (channels, F, M) complex128 from the amplitudes and the exact integer phases"""
    amp = np.asarray(frames, np.float32)[..., 0].astype(np.float64)
    return unbins(amp * np.exp(2j * np.pi * (theta.astype(np.float64) / TWO32)))


def synth32(frames, theta):
    """the same in float32: the phase as a signed number of half turns times pi, numpy's float32 cos / sin, one product"""
    f32 = np.float32
    amp = np.asarray(frames, f32)[..., 0]
    ang = f32(np.pi) * (theta.astype(np.int32).astype(f32) * f32(2.0 ** -31))
    assert ang.dtype == f32
    return unbins(((amp * np.cos(ang)) + 1j * (amp * np.sin(ang))).astype(np.complex64))


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.complex128).ravel(), np.asarray(ref, np.complex128).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a - ref))


def phasors(frames, size, hop, sr):
    """amp * exp(2 pi i dev), dev recovered from freq: the analysis metric that leaves no bin out"""
    fr = np.asarray(frames, np.float64)
    return fr[..., 0] * np.exp(2j * np.pi * dev_of(fr[..., 1], size, hop, sr))
