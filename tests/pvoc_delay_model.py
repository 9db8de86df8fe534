"""numpy restatement of the per-bin delay with feedback of clfa_pvoc (include/clfft_amd.h), in float32, operation by
operation: what the device results are compared with bit for bit.  Frames are (channels, F, M + 1, 2) float32; the tables
are (M + 1,) arrays or numbers, shared by the channels.  delay32 takes the two histories and returns (the output frames, the
new xhist, the new yhist); Stream holds the histories as a clfa_pvoc does."""
import numpy as np

from tests.pvoc_time_model import empty

f32 = np.float32


def clamp_delays(delays, L, B):
    """the device form's delays: (B,) int64 in 0..L"""
    return np.clip(np.broadcast_to(np.asarray(delays, np.int64), (B,)), 0, L)


def delay32(frames, delays, feedback, xhist, yhist):
    """xhist, yhist: (C, L, M + 1, 2), oldest frame first; feedback None: none -> (out, the new xhist, the new yhist)"""
    frames = np.ascontiguousarray(frames, f32)
    C, F, B = frames.shape[:3]
    L = xhist.shape[1]
    assert xhist.shape == yhist.shape == (C, L, B, 2)
    d = clamp_delays(delays, L, B)
    xs = np.concatenate([np.ascontiguousarray(xhist, f32), frames], axis=1)
    ys = np.concatenate([np.ascontiguousarray(yhist, f32), np.zeros_like(frames)], axis=1)
    bins = np.arange(B)
    if feedback is not None:
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(feedback, f32), (B,)))
        fb = d > 0                                      # a loop without a delay is not defined: d == 0 copies
    with np.errstate(all="ignore"):
        for f in range(F):
            j = L + f - d
            x = xs[:, j, bins]                          # (C, B, 2): bin b of frame j[b]
            if feedback is None:
                ys[:, L + f] = x
                continue
            y = ys[:, j, bins]                          # j < L + f wherever fb holds: already final
            a1 = x[..., 0]
            a2 = g * y[..., 0]                          # one rounded float32 product,
            amp = a1 + a2                               # one rounded float32 sum
            freq = np.where(np.abs(a2) > np.abs(a1), y[..., 1], x[..., 1])    # a NaN on either side: the input's freq
            ys[:, L + f] = np.where(fb[:, None], np.stack([amp, freq], axis=-1), x)
    assert ys.dtype == f32 and xs.dtype == f32
    n = xs.shape[1]
    return np.ascontiguousarray(ys[:, L:]), np.ascontiguousarray(xs[:, n - L:]), np.ascontiguousarray(ys[:, n - L:])


def delay_take(frames, delays, xhist):
    """the equivalent statement without feedback: np.take along the frames of the history-padded input, bin by bin"""
    frames = np.ascontiguousarray(frames, f32)
    C, F, B = frames.shape[:3]
    L = xhist.shape[1]
    d = clamp_delays(delays, L, B)
    xs = np.concatenate([xhist, frames], axis=1)
    out = np.empty_like(frames)
    for b in range(B):
        out[:, :, b] = np.take(xs[:, :, b], L - d[b] + np.arange(F), axis=1)
    return out


class Stream:
    """the two histories of one clfa_pvoc after delay_setup(max_delay), and the call that advances them"""

    def __init__(self, channels, size, sr, max_delay):
        self.channels, self.size, self.sr, self.max_delay = channels, size, sr, max_delay
        self.reset()

    def reset(self):
        self.xhist = empty(self.channels, self.size, self.sr, self.max_delay)
        self.yhist = empty(self.channels, self.size, self.sr, self.max_delay)

    def state(self):
        return self.xhist, self.yhist

    def run(self, frames, delays, feedback=None):
        out, self.xhist, self.yhist = delay32(frames, delays, feedback, self.xhist, self.yhist)
        return out
