"""numpy restatement of the operations along a stream of (amp, freq) frames of clfa_pvoc (include/clfft_amd.h): blur,
smooth and freeze — in float32, operation by operation (what the device results are compared with bit for bit; the blur's
sum is an explicit loop over the window's frames, oldest first, never np.sum, which is pairwise), and once more in float64.
Frames are (channels, F, M + 1, 2) float32; per-frame values are numbers or (F,) arrays.  Every function takes the
operation's state and returns (the output frames, the new state); Stream holds the three states as a clfa_pvoc does."""
import numpy as np

from tests import pvoc_pair_model as pp

f32 = np.float32
BLUR, SMOOTH, FREEZE = range(3)
NAMES = ("blur", "smooth", "freeze")


def empty(channels, size, sr, frames=None):
    """EMPTY bins, (0, fl(k cf)) with cf = (float)(sr / size): (channels, M + 1, 2), or (channels, frames, M + 1, 2)"""
    B = size // 2 + 1
    e = np.zeros((B, 2), f32)
    e[:, 1] = np.arange(B, dtype=f32) * f32(sr / size)
    shape = (channels, B, 2) if frames is None else (channels, frames, B, 2)
    return np.ascontiguousarray(np.broadcast_to(e, shape))


def _per_frame(x, F, dtype=f32):
    return np.broadcast_to(np.asarray(x, dtype), (F,))


def blur_n(length, max_frames):
    """the window length of one frame: 1 where length >= 1 does not hold (a NaN included)"""
    length = f32(length)
    if not length >= f32(1):
        return 1
    return int(np.floor(np.fmin(length, f32(max_frames))))


def blur32(frames, length, hist, max_frames):
    """hist: (C, max_frames - 1, M + 1, 2), oldest first -> (out, the new history)"""
    frames, hist = np.ascontiguousarray(frames, f32), np.ascontiguousarray(hist, f32)
    F, L = frames.shape[1], max_frames - 1
    assert hist.shape == (frames.shape[0], L) + frames.shape[2:]
    length = _per_frame(length, F)
    s = np.concatenate([hist, frames], axis=1)
    out = np.empty_like(frames)
    with np.errstate(all="ignore"):
        for f in range(F):
            n = blur_n(length[f], max_frames)
            rn = f32(1.0 / n)
            S = s[:, L + f - n + 1].copy()
            for t in range(L + f - n + 2, L + f + 1):
                S = S + s[:, t]                  # one rounded float32 addition per frame, ascending
            out[:, f] = S * rn
    assert out.dtype == f32
    return out, np.ascontiguousarray(s[:, s.shape[1] - L:])


def blur64(frames, length, hist, max_frames):
    frames, hist = np.asarray(frames, np.float64), np.asarray(hist, np.float64)
    F, L = frames.shape[1], max_frames - 1
    length = _per_frame(length, F)
    s = np.concatenate([hist, frames], axis=1)
    out = np.empty_like(frames)
    for f in range(F):
        n = blur_n(length[f], max_frames)
        out[:, f] = s[:, L + f - n + 1:L + f + 1].sum(axis=1) / n
    return out, s[:, s.shape[1] - L:]


def smooth32(frames, amp, freq, y):
    """y: (C, M + 1, 2) -> (out, the new y); MORPH's rule from y towards the frame, column by column"""
    frames = np.ascontiguousarray(frames, f32)
    F = frames.shape[1]
    ca, cf = pp.clamp(_per_frame(amp, F)), pp.clamp(_per_frame(freq, F))
    y = np.ascontiguousarray(y, f32).copy()
    out = np.empty_like(frames)
    with np.errstate(all="ignore"):
        for f in range(F):
            x = frames[:, f]
            y = np.stack([pp._morph(y[..., 0], x[..., 0], ca[f]), pp._morph(y[..., 1], x[..., 1], cf[f])], axis=-1)
            out[:, f] = y
    assert out.dtype == f32 and y.dtype == f32
    return out, y


def smooth64(frames, amp, freq, y):
    frames = np.asarray(frames, np.float64)
    F = frames.shape[1]
    c = np.stack([pp.clamp(_per_frame(amp, F)), pp.clamp(_per_frame(freq, F))], axis=-1).astype(np.float64)
    y = np.asarray(y, np.float64).copy()
    out = np.empty_like(frames)
    for f in range(F):
        y = y + c[f] * (frames[:, f] - y)
        out[:, f] = y
    return out, y


def freeze32(frames, amp, freq, held, dtype=f32):
    """held: (C, M + 1, 2) -> (out, the new held); a column is frozen where its flag != 0 (a NaN freezes).  Only bits move."""
    frames = np.ascontiguousarray(frames, dtype)
    F = frames.shape[1]
    flags = np.stack([_per_frame(amp, F), _per_frame(freq, F)], axis=-1)
    held = np.ascontiguousarray(held, dtype).copy()
    out = np.empty_like(frames)
    for f in range(F):
        for col in range(2):
            if flags[f, col] == 0:
                held[..., col] = frames[:, f, :, col]
            out[:, f, :, col] = held[..., col]
    return out, held


def freeze64(frames, amp, freq, held):
    return freeze32(frames, amp, freq, held, np.float64)


def freeze_gather(frames, amp, freq, start):
    """the equivalent statement: out[f] = in[g], g the last frame <= f whose flag is 0, else `start` (C, M + 1, 2)"""
    frames = np.ascontiguousarray(frames, f32)
    F = frames.shape[1]
    out = np.empty_like(frames)
    for col, flag in enumerate((_per_frame(amp, F), _per_frame(freq, F))):
        for f in range(F):
            g = [i for i in range(f + 1) if flag[i] == 0]
            out[:, f, :, col] = frames[:, g[-1], :, col] if g else start[..., col]
    return out


class Stream:
    """the three states of one clfa_pvoc, and the calls that advance them"""

    def __init__(self, channels, size, sr, max_frames=None):
        self.channels, self.size, self.sr, self.max_frames = channels, size, sr, max_frames
        self.reset()

    def reset(self):
        self.y = empty(self.channels, self.size, self.sr)
        self.held = empty(self.channels, self.size, self.sr)
        if self.max_frames is not None:
            self.hist = empty(self.channels, self.size, self.sr, self.max_frames - 1)

    def state(self, op):
        return self.hist if op == BLUR else (self.y if op == SMOOTH else self.held)

    def run(self, op, frames, p, q=None):
        if op == BLUR:
            out, self.hist = blur32(frames, p, self.hist, self.max_frames)
        elif op == SMOOTH:
            out, self.y = smooth32(frames, p, q, self.y)
        elif op == FREEZE:
            out, self.held = freeze32(frames, p, q, self.held)
        else:
            raise ValueError(op)
        return out
