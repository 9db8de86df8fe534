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


# ---- mirror of opencl_fft_amd/csrc/stft_plan.hpp: the synthesis kernel's run split (tests/test_stft_plan_cpu.py checks
# the header itself; this restatement lets a failing device test name the run, the group and fw of a wrong sample) ------
# the (size, hop) pairs of tests/test_gpu_stft_synth.py, which tests/test_stft_plan_cpu.py also splits on the CPU
SYNTH_PAIRS = [(64, 16), (64, 1), (256, 3), (1024, 255), (2048, 64), (4096, 1024), (8192, 8191), (16384, 4096),
               (64, 64), (4096, 4096), (64, 3), (2048, 16), (2048, 1), (256, 256), (256, 64)]


def fpw(size):
    """frames a workgroup holds at once (stft_fpw)"""
    return 1 if size >= 8192 else 8192 // size


def run_frames(nframes, slots, size, hop, F):
    """nf of stft_run_frames: frames per run"""
    warm = -(-size // hop)
    return min(max(-(-nframes // slots), 8 * warm, fpw(size)), F)


def runs_of(F, nf):
    return -(-F // nf)


def run(r, nf, F, size, hop):
    """(s, e_end, own_lo, fw) of stft_run"""
    s = r * nf
    own_lo = s * hop
    return s, min(s + nf, F), own_lo, ((own_lo - size) // hop + 1 if own_lo >= size else 0)


def locate(p, nf, F, size, hop):
    """where sample p of a channel is made: (run, its fw, the group of fpw frames whose write-out holds p, the covering
    frames [f_lo, f_hi])"""
    r = min(p // (nf * hop), runs_of(F, nf) - 1)
    _, e_end, _, fw = run(r, nf, F, size, hop)
    group = (min(p // hop, e_end - 1) - fw) // fpw(size)
    return r, fw, group, (0 if p < size else (p - size) // hop + 1, min(p // hop, F - 1))


def env_branch(size, hop, F, p):
    """which form of stft_env_at sample p takes (1 tail sum, 2 head sum, 3 difference: stft_env_span); p may be an array"""
    p = np.asarray(p, np.int64)
    fh = np.minimum(p // hop, F - 1)
    fl = np.where(p < size, 0, (p - size) // hop + 1)
    dl, dh = p - fh * hop, p - fl * hop
    return np.where(dh + hop >= size, 1, np.where(dl < hop, 2, 3))
