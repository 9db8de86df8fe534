"""numpy restatement of the operations on (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): pitch scale, frequency
shift and timed read — once in float32, operation by operation (what the device results are compared with bit for bit,
the formant envelope excepted: the device's logf / expf and transform roundings are not numpy's), and once in float64
(the truth the formant amplitudes are measured against).  Frames are (channels, F, M + 1, 2) float32."""
import numpy as np

from oracle import oracle

f32 = np.float32
EMPTY, COPY = -1, -2
FLOOR = f32(1e-20)


def cf_of(size, sr):
    return f32(sr / size)


def bpf_of(size, sr):
    return f32(size / sr)


def scale_j(k, s):
    """j of source k: (int)floorf(fl(k s) + 0.5f)"""
    return np.floor(f32(k) * f32(s) + f32(0.5)).astype(np.int64)


def scale_map_serial(M, s):
    """the definition, k ascending, a later k replacing an earlier one -> src[j]: k, EMPTY or COPY"""
    src = np.full(M + 1, EMPTY, np.int64)
    src[0] = src[M] = COPY
    s = f32(s)
    if not (s >= f32(0.25) and s <= f32(4)):     # outside the range or NaN: what the device form does
        return src
    for k in range(1, M):
        j = int(scale_j(k, s))
        if 1 <= j <= M - 1:
            src[j] = k
    return src


def scale_map_gather(M, s):
    """the kernels' form: k -> j is monotone, so bin j's source is the largest k with j(k) <= j, if that k lands on j"""
    src = np.full(M + 1, EMPTY, np.int64)
    src[0] = src[M] = COPY
    s = f32(s)
    if not (s >= f32(0.25) and s <= f32(4)):
        return src
    for j in range(1, M):
        k = int((f32(j) + f32(0.5)) / s)
        k = min(max(k, 1), M - 1)
        while k < M - 1 and scale_j(k + 1, s) <= j:
            k += 1
        while k >= 1 and scale_j(k, s) > j:
            k -= 1
        if k >= 1 and scale_j(k, s) == j:
            src[j] = k
    return src


def shift_map(M, shift, lowest, bpf):
    """src[j] of the frequency shift: d = (int)rintf(fl(shift bpf)), source j - d inside lowest..M-1"""
    src = np.full(M + 1, EMPTY, np.int64)
    src[0] = src[M] = COPY
    src[1:lowest] = COPY
    with np.errstate(invalid="ignore", over="ignore"):
        t = f32(shift) * f32(bpf)
    if not abs(t) <= f32(M):
        return src
    d = int(np.rint(t))
    j = np.arange(lowest, M)
    k = j - d
    ok = (k >= lowest) & (k <= M - 1)
    src[j[ok]] = k[ok]
    return src


def _ext(L):
    """the even extension of (..., M + 1) to size = 2 M points"""
    M = L.shape[-1] - 1
    return np.concatenate([L, L[..., M - 1:0:-1]], axis=-1)


def env32(amp, coefs):
    """float32: numpy's log / exp around the project's float32 packed real transforms (the C restatement of Clrfft)"""
    amp = np.asarray(amp, f32)
    M = amp.shape[-1] - 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = np.log(np.fmax(amp, FLOOR))
        assert L.dtype == f32
        P = oracle.rfft_forward(_ext(L).reshape(-1, 2 * M))
        P[:, coefs + 1:] = 0
        P[:, 0] = P[:, 0].real
        y = oracle.rfft_inverse(P)[:, :M + 1].reshape(amp.shape)
        return np.exp(y.astype(f32))


def _in64(a):
    """the float64 model's input: float32 data as it is, or float64 data given to it directly (exact test signals)"""
    a = np.asarray(a)
    return a if a.dtype == np.float64 else a.astype(f32)


def env64(amp, coefs):
    """float64, by the cosine sums of the definition"""
    amp = _in64(amp)
    M = amp.shape[-1] - 1
    size = 2 * M
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Lx = _ext(np.log(np.fmax(amp, FLOOR).astype(np.float64))).reshape(-1, size)
        q = np.arange(1, coefs + 1, dtype=np.int64)
        c_in = np.cos(2 * np.pi * ((np.arange(size, dtype=np.int64)[:, None] * q) % size) / size)        # (size, coefs)
        c_out = np.cos(2 * np.pi * ((q[:, None] * np.arange(M + 1, dtype=np.int64)) % size) / size)      # (coefs, M + 1)
        a = (2.0 / size) * (Lx @ c_in)
        logE = Lx.mean(axis=-1, keepdims=True) + a @ c_out
        return np.exp(logE).reshape(amp.shape)


def env64_fft(amp, coefs):
    """float64, by numpy's transforms: the same sums as env64 at any size (env64 builds (size x coefs) cosine matrices,
    1 GB at size 16384 with every coefficient).  env64 stays the definition; this is the truth of the per-bin tests"""
    amp = _in64(amp)
    M = amp.shape[-1] - 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        P = np.fft.rfft(_ext(np.log(np.fmax(amp, FLOOR).astype(np.float64))), axis=-1)
        P[..., coefs + 1:] = 0
        return np.exp(np.fft.irfft(P, n=2 * M, axis=-1)[..., :M + 1])


def _apply(frames, srcs, par, op, gain, cf, env, dtype):
    """srcs: (F, M + 1) source maps; par (F,); env: None or (C, F, M + 1) in `dtype`; amps in `dtype`, freqs in float32"""
    fr = _in64(frames) if dtype == np.float64 else np.asarray(frames, f32)
    C, F, B, _ = fr.shape
    out_a = np.zeros((C, F, B), dtype)
    out_f = np.broadcast_to(np.arange(B, dtype=f32) * f32(cf), (C, F, B)).copy()
    assert out_f.dtype == f32
    g = dtype(gain)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for f in range(F):
            src = srcs[f]
            cp = np.nonzero(src == COPY)[0]
            out_a[:, f, cp] = fr[:, f, cp, 0].astype(dtype)
            out_f[:, f, cp] = fr[:, f, cp, 1].astype(f32)
            j = np.nonzero(src >= 0)[0]
            k = src[j]
            a = g * fr[:, f, k, 0].astype(dtype)
            if env is not None:
                a = (a / env[:, f, k]) * env[:, f, j]
            assert a.dtype == dtype
            out_a[:, f, j] = a
            p = f32(par[f])
            fk = fr[:, f, k, 1].astype(f32)
            out_f[:, f, j] = fk * p if op == "scale" else fk + p
    return out_a, out_f


_MAPS = {}


def maps(op, M, par, lowest=1, bpf=None):
    out = []
    for p in np.asarray(par, f32).reshape(-1):
        key = (op, M, f32(p).tobytes(), lowest, None if bpf is None else f32(bpf).tobytes())
        if key not in _MAPS:
            _MAPS[key] = scale_map_serial(M, p) if op == "scale" else shift_map(M, p, lowest, bpf)
        out.append(_MAPS[key])
    return out


def op32(op, frames, par, size, sr, lowest=1, keepform=False, gain=1.0, coefs=1):
    """float32 model of scale / shift -> frames (C, F, M + 1, 2) float32"""
    fr = np.asarray(frames, f32)
    M = size // 2
    par = np.broadcast_to(np.asarray(par, f32), (fr.shape[1],))
    env = env32(fr[..., 0], coefs) if keepform else None
    a, fq = _apply(fr, maps(op, M, par, lowest, bpf_of(size, sr)), par, op, gain, cf_of(size, sr), env, f32)
    return np.stack([a, fq], axis=-1)


def op64_amps(op, frames, par, size, sr, lowest=1, keepform=False, gain=1.0, coefs=1):
    """float64 amplitudes of scale / shift (the gain as the float32 the call passes)"""
    fr = _in64(frames)
    M = size // 2
    par = np.broadcast_to(np.asarray(par, f32), (fr.shape[1],))
    env = env64(fr[..., 0], coefs) if keepform else None
    return _apply(fr, maps(op, M, par, lowest, bpf_of(size, sr)), par, op, float(f32(gain)), cf_of(size, sr), env, np.float64)[0]


def read32(frames, pos):
    """timed read: (C, Fin, B, 2), pos (Fout,) -> (C, Fout, B, 2), every operation in float32"""
    fr = np.asarray(frames, f32)
    Fin = fr.shape[1]
    pos = np.asarray(pos, f32).reshape(-1)
    out = np.zeros((fr.shape[0], pos.size) + fr.shape[2:], f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g, q in enumerate(pos):
            p = np.fmin(np.fmax(q, f32(0)), f32(Fin - 1))
            i = int(np.floor(p))
            a = f32(p - f32(i))
            i1 = min(i + 1, Fin - 1)
            if a == 0:
                out[:, g] = fr[:, i]
            else:
                x0, x1 = fr[:, i], fr[:, i1]
                out[:, g] = x0 + a * (x1 - x0)
    return out


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a - ref))
