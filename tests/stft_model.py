"""float64 / float32 numpy models of the short-time transforms of clfa_stft (include/clfft_amd.h), for the tests."""
import numpy as np


def frames_of(size, hop, samples):
    return 0 if samples < size else 1 + (samples - size) // hop


def frame_view(x, size, hop):
    """(channels, samples) -> (channels, F, size) strided view of the frames (no copy)"""
    x = np.asarray(x)
    F = frames_of(size, hop, x.shape[-1])
    s = x.strides
    return np.lib.stride_tricks.as_strided(x, (x.shape[0], F, size), (s[0], s[1] * hop, s[1]), writeable=False)


def windowed_frames_f32(x, size, hop, w):
    """fl(w[t] * x[f hop + t]) in float32: the vectors the analysis transforms"""
    return (frame_view(np.asarray(x, np.float32), size, hop) * np.asarray(w, np.float32)).astype(np.float32)


def overlap_add(r, w, hop, normalize=False, dtype=np.float64):
    """y[c, t] = sum_f w[t - f hop] r[c, f, t - f hop], ascending f, in `dtype`; normalize: / env where env > 1e-11"""
    r = np.asarray(r, dtype)
    w = np.asarray(w, dtype)
    C, F, size = r.shape
    L = (F - 1) * hop + size
    y = np.zeros((C, L), dtype)
    env = np.zeros(L, dtype)
    for f in range(F):
        y[:, f * hop:f * hop + size] += (w * r[:, f]).astype(dtype)
        env[f * hop:f * hop + size] += w * w
    if normalize:
        m = env > 1e-11
        y[:, m] = y[:, m] / env[m]
    return y, env
